// check_core_check.cpp -- TEST ARTEFACT.  The solution check's arithmetic (diffqcqp_amd/csrc/check_core.h) for the CPU: the L
// lanes of a problem are an array here, the DPP exchange of check.hip an index j ^ step, everything else the very functions
// the kernel calls.  tests/test_check_hostcore.py compares it with the numpy restatement of the definitions,
// tests/test_gpu_check.py with the device, bit for bit.  plan_check (route.cpp) is behind the same face for
// tests/test_check_routes.py.  Nothing in the product links or loads this file.
#include "../../diffqcqp_amd/csrc/check_core.h"
#include "../../diffqcqp_amd/csrc/route.cpp"

using namespace dqq;

namespace {

struct Problem {
    int n;
    const double *P, *q, *a, *b, *c, *x;
};

template <int KIND>
void coords(CheckAcc& acc, const Problem& p, int i, const double* s, const double* ab)
{
    if constexpr (KIND == 1) {
        const double xx[2] = {p.x[i], p.x[i + 1]}, qq[2] = {p.q[i], p.q[i + 1]};
        const double ss[2] = {s[0], s[1]}, aa[2] = {ab[0], ab[1]};
        check_contact(acc, xx, ss, aa, qq, p.a[i / 2] * p.b[i / 2]);
    } else {
        const bool box = KIND == 2 || KIND == 3;
        check_coord<KIND>(acc, p.x[i], s[0], ab[0], p.q[i], box ? p.a[i] : 0.0, box ? p.b[i] : 0.0,
                          KIND == 3 ? check_sign(p.c[i]) : 0.0);
    }
}

template <int KIND, int W>
int run(const Problem& p, bool diag, bool has_iters, int iters, int max_iter, double* resid)
{
    const int n = p.n, L = check_lanes(n), span = L * W;
    CheckAcc acc[64];
    for (int j = 0; j < L; ++j) acc[j].init();
    if (diag) {
        for (int j = 0; j < L; ++j)
            for (int c = j * W; c < n; c += span) {
                double s[W], ab[W];
                for (int w = 0; w < W; ++w) {
                    s[w] = ab[w] = 0.0;
                    const double p1[1] = {p.P[c + w]}, x1[1] = {p.x[c + w]};
                    check_row_terms<1>(p1, x1, s[w], ab[w]);
                }
                if (KIND == 1) coords<KIND>(acc[j], p, c, s, ab);
                else
                    for (int w = 0; w < W; ++w) coords<KIND>(acc[j], p, c + w, s + w, ab + w);
            }
    } else {
        double keep_s = 0.0, keep_ab = 0.0;   // a contact's first row
        for (int i = 0; i < n; ++i) {
            double s[64], ab[64], t[64];
            for (int j = 0; j < L; ++j) {
                s[j] = ab[j] = 0.0;
                for (int c = j * W; c < n; c += span) {
                    double pp[W], xx[W];
                    for (int w = 0; w < W; ++w) { pp[w] = p.P[(long)i * n + c + w]; xx[w] = p.x[c + w]; }
                    check_row_terms<W>(pp, xx, s[j], ab[j]);
                }
            }
            for (int step = 1; step < L; step *= 2) {
                for (int j = 0; j < L; ++j) t[j] = s[j] + s[j ^ step];
                for (int j = 0; j < L; ++j) s[j] = t[j];
                for (int j = 0; j < L; ++j) t[j] = ab[j] + ab[j ^ step];
                for (int j = 0; j < L; ++j) ab[j] = t[j];
            }
            const int j = (i & (span - 1)) >> (W - 1);   // the lane that owns column i
            if (KIND == 1) {
                if ((i & 1) == 0) { keep_s = s[j]; keep_ab = ab[j]; continue; }
                const double ss[2] = {keep_s, s[j]}, aa[2] = {keep_ab, ab[j]};
                coords<KIND>(acc[j], p, i - 1, ss, aa);
            } else {
                coords<KIND>(acc[j], p, i, s + j, ab + j);
            }
        }
    }
    for (int step = 1; step < L; step *= 2) {
        CheckAcc old[64];
        for (int j = 0; j < L; ++j) old[j] = acc[j];
        for (int j = 0; j < L; ++j) check_merge(acc[j], old[j ^ step]);
    }
    resid[0] = acc[0].nat;
    resid[1] = acc[0].inf;
    resid[2] = acc[0].obj;
    resid[3] = acc[0].scl;
    return check_status(acc[0], has_iters, iters, max_iter);
}

} // namespace

extern "C" {

// one problem: kind 0..3, diag: P is the n diagonal entries; a, b, c the kind's extras; -> status, resid[4]
__attribute__((visibility("default"))) int hostcheck(int kind, int diag, int n, const double* P, const double* q,
                                                     const double* a, const double* b, const double* c, const double* x,
                                                     int has_iters, int iters, int max_iter, double* resid)
{
    const Problem p{n, P, q, a, b, c, x};
    const bool even = check_cols_per_lane(n) == 2;
    switch (kind) {
    case 0: return even ? run<0, 2>(p, diag, has_iters, iters, max_iter, resid) : run<0, 1>(p, diag, has_iters, iters, max_iter, resid);
    case 1: return even ? run<1, 2>(p, diag, has_iters, iters, max_iter, resid) : -1;
    case 2: return even ? run<2, 2>(p, diag, has_iters, iters, max_iter, resid) : run<2, 1>(p, diag, has_iters, iters, max_iter, resid);
    case 3: return even ? run<3, 2>(p, diag, has_iters, iters, max_iter, resid) : run<3, 1>(p, diag, has_iters, iters, max_iter, resid);
    default: return -1;
    }
}

// route.cpp: plan_check -> out[3] = err, family, lanes
__attribute__((visibility("default"))) void hostcheck_plan(int kind, int n, long long B, int p_layout, int* out)
{
    const CheckPlan p = plan_check(kind, n, B, p_layout);
    out[0] = p.err;
    out[1] = (int)p.family;
    out[2] = p.lanes;
}

} // extern "C"
