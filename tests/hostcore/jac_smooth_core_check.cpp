// jac_smooth_core_check.cpp -- TEST ARTEFACT.  smooth_core.h's newton_jac_problem_smooth on one CPU thread over a batch.
// tests/jac_smooth_cases.py builds it as a shared library (loaded through ctypes: the yardstick of the device tests) and, with
// -DJAC_SMOOTH_CHECK_MAIN, as a stand-alone program, plain and with the address and undefined-behaviour sanitizers, that
// tests/test_jac_smooth_hostcore.py runs.  tests/test_jac_smooth_hostcore.py holds it to the numpy restatement
// (tests/jac_smooth_reference.py) bit for bit, tests/test_gpu_jac_smooth.py holds the kernels to it.
// Nothing in the product links or loads this file.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../diffqcqp_amd/csrc/smooth_core.h"

using namespace dqq;

namespace {

const double* at(const double* p, size_t off) { return p != nullptr ? p + off : nullptr; }
double* at(double* p, size_t off) { return p != nullptr ? p + off : nullptr; }

// doubles per problem of output `which` (0 Jq, 1 Ja, 2 Jb)
size_t out_size(int kind, int n, int diag, int which)
{
    if (diag) return kind == 1 && which == 0 ? 2 * (size_t)n : (size_t)n;
    return (size_t)n * (which == 0 ? n : newton_jac_extra_cols(kind, n));
}

} // namespace

extern "C" {

// P (B n n; diag: B n), q, x (B n), a, b, c: the kind's extras (B ne; c (B n)); Jq, Ja, Jb as include/diffqcqp_hip.h shapes them,
// each may be NULL
__attribute__((visibility("default"))) int jac_smooth_batch(int kind, int B, int n, int diag, const double* P, const double* q,
                                                            const double* a, const double* b, const double* c, const double* x,
                                                            double* Jq, double* Ja, double* Jb, int* status, double reg, double kappa)
{
    if (kind < 0 || kind > 3 || B < 0 || n < 1) return 2;
    const size_t np = diag ? (size_t)n : (size_t)n * n, ne = newton_jac_extra_cols(kind, n);
    std::vector<double> work(newton_jac_work_doubles(kind, n));
    for (int p = 0; p < B; ++p) {
        const size_t v = (size_t)p * n;
#define JAC_SMOOTH(K) newton_jac_problem_smooth<K>(P + p * np, diag != 0, q + v, at(a, p * ne), at(b, p * ne), at(c, v), x + v, \
                                                   at(Jq, p * out_size(kind, n, diag, 0)), at(Ja, p * out_size(kind, n, diag, 1)), \
                                                   at(Jb, p * out_size(kind, n, diag, 2)), n, work.data(), reg, kappa)
        const int s = kind == 0 ? JAC_SMOOTH(0) : kind == 1 ? JAC_SMOOTH(1) : kind == 2 ? JAC_SMOOTH(2) : JAC_SMOOTH(3);
#undef JAC_SMOOTH
        if (status != nullptr) status[p] = s;
    }
    return 0;
}

// newton_jvp_problem_smooth over the batch with one tangent (which: 0 dq, 1 da, 2 db) and every other NULL
__attribute__((visibility("default"))) int jvp_smooth_unit_batch(int kind, int B, int n, int diag, const double* P, const double* q,
                                                                 const double* a, const double* b, const double* c, const double* x,
                                                                 int which, const double* tan, double* dx, int* status, double reg,
                                                                 double kappa)
{
    const size_t np = diag ? (size_t)n : (size_t)n * n, ne = newton_jac_extra_cols(kind, n);
    std::vector<double> work((size_t)n * n + newton_vec_doubles(n));
    for (int p = 0; p < B; ++p) {
        const size_t v = (size_t)p * n;
        const double* dq = which == 0 ? tan + v : nullptr;
        const double* da = which == 1 ? tan + p * ne : nullptr;
        const double* db = which == 2 ? tan + p * ne : nullptr;
#define JVP_SMOOTH(K) newton_jvp_problem_smooth<K>(P + p * np, diag != 0, q + v, at(a, p * ne), at(b, p * ne), at(c, v), x + v, nullptr, dq, \
                                                   da, db, dx + v, n, work.data(), reg, kappa)
        status[p] = kind == 0 ? JVP_SMOOTH(0) : kind == 1 ? JVP_SMOOTH(1) : kind == 2 ? JVP_SMOOTH(2) : JVP_SMOOTH(3);
#undef JVP_SMOOTH
    }
    return 0;
}

} // extern "C"

#if defined(JAC_SMOOTH_CHECK_MAIN)
// Every kind, both layouts and kappa in {0, 1e-4, 1e-2, 1}, reg in {0, 1e-3}, on a small fixed batch with a NaN problem and an
// infinite bound in the middle of it; each output alone and all together.  Checks every column against
// newton_jvp_problem_smooth with the unit tangent bit for bit, the statuses and the NaN rows; what it is run for is the sanitizers.
int main()
{
    const int B = 6, n = 6;
    int fails = 0;
    const double kappas[4] = {0.0, 1e-4, 1e-2, 1.0}, regs[2] = {0.0, 1e-3};
    for (int kind = 0; kind < 4; ++kind)
        for (int diag = 0; diag < 2; ++diag)
            for (double kappa : kappas)
                for (double reg : regs) {
                    const size_t np = diag ? (size_t)n : (size_t)n * n, ne = newton_jac_extra_cols(kind, n);
                    std::vector<double> P(B * np), q((size_t)B * n), a(B * ne), b(B * ne), c((size_t)B * n), x((size_t)B * n);
                    unsigned long long r = 8765 + 17 * kind + diag;
                    auto rnd = [&]() { r = r * 6364136223846793005ull + 1442695040888963407ull; return (double)(r >> 11) / 9007199254740992.0 - 0.5; };
                    for (int p = 0; p < B; ++p) {
                        for (int i = 0; i < n; ++i) {
                            if (diag) P[p * np + i] = 1.0 + rnd();
                            else for (int j = 0; j < n; ++j) P[p * np + i * n + j] = (i == j ? 2.0 : 0.0) + 0.2 * rnd();
                            q[p * n + i] = 2.0 * rnd();
                            x[p * n + i] = rnd();
                            c[p * n + i] = rnd();
                        }
                        for (size_t i = 0; i < ne; ++i) {
                            a[p * ne + i] = kind == 1 ? 0.5 + rnd() : -0.3 + 0.2 * rnd();
                            b[p * ne + i] = kind == 1 ? 0.6 : 0.3 + 0.2 * rnd();
                        }
                    }
                    q[2 * n + 2] = std::nan("");                        // problem 2: not finite
                    if (kind >= 1) b[3 * ne + 1] = INFINITY;            // problem 3: an infinite bound / friction coefficient
                    else x[3 * n + 1] = INFINITY;
                    const double* pa = ne ? a.data() : nullptr;
                    const double* pb = ne ? b.data() : nullptr;
                    const double* pc = kind == 3 ? c.data() : nullptr;
                    const size_t sz[3] = {out_size(kind, n, diag, 0), out_size(kind, n, diag, 1), out_size(kind, n, diag, 2)};
                    std::vector<double> J[3], one[3];
                    for (int w = 0; w < 3; ++w) { J[w].assign(B * sz[w], 7.0); one[w].assign(B * sz[w], 7.0); }
                    std::vector<int> st(B, -1), st1(B, -1);
                    const int nout = kind == 0 ? 1 : 3;
                    jac_smooth_batch(kind, B, n, diag, P.data(), q.data(), pa, pb, pc, x.data(), J[0].data(), nout > 1 ? J[1].data() : nullptr,
                                     nout > 1 ? J[2].data() : nullptr, st.data(), reg, kappa);
                    for (int w = 0; w < nout; ++w) {   // each output alone: the same bits, the same status
                        jac_smooth_batch(kind, B, n, diag, P.data(), q.data(), pa, pb, pc, x.data(), w == 0 ? one[0].data() : nullptr,
                                         w == 1 ? one[1].data() : nullptr, w == 2 ? one[2].data() : nullptr, st1.data(), reg, kappa);
                        if (std::memcmp(one[w].data(), J[w].data(), sizeof(double) * J[w].size()) != 0 || st1 != st) {
                            printf("kind %d diag %d kappa %g: output %d alone differs from the full call\n", kind, diag, kappa, w); ++fails;
                        }
                    }
                    for (int p = 0; p < B; ++p) {
                        const int want = p == 2 || p == 3 ? 2 : 0;
                        if (st[p] != want) { printf("kind %d diag %d kappa %g problem %d: status %d, expected %d\n", kind, diag, kappa, p, st[p], want); ++fails; }
                        for (int w = 0; w < nout; ++w)
                            for (size_t i = 0; i < sz[w]; ++i)
                                if ((want != 0) != std::isnan(J[w][p * sz[w] + i])) { printf("kind %d diag %d kappa %g problem %d: NaN rows are wrong\n", kind, diag, kappa, p); ++fails; i = sz[w]; }
                    }
                    // every column against the smoothed JVP of the unit tangent, bit for bit
                    std::vector<double> dx((size_t)B * n), tan((size_t)B * n);
                    for (int w = 0; w < nout; ++w) {
                        const int cols = w == 0 ? n : (int)ne;
                        for (int j = 0; j < cols; ++j) {
                            std::fill(tan.begin(), tan.end(), 0.0);
                            const size_t tw = w == 0 ? (size_t)n : ne;
                            for (int p = 0; p < B; ++p) tan[p * tw + j] = 1.0;
                            std::vector<int> sj(B);
                            jvp_smooth_unit_batch(kind, B, n, diag, P.data(), q.data(), pa, pb, pc, x.data(), w, tan.data(), dx.data(), sj.data(), reg, kappa);
                            for (int p = 0; p < B; ++p)
                                for (int i = 0; i < n; ++i) {
                                    double got;
                                    if (!diag) got = J[w][p * sz[w] + (size_t)i * cols + j];
                                    else if (kind == 1) { if (w == 0 ? i / 2 != j / 2 : i / 2 != j) continue; got = w == 0 ? J[0][p * sz[0] + 2 * i + (j & 1)] : J[w][p * sz[w] + i]; }
                                    else { if (i != j) continue; got = J[w][p * sz[w] + i]; }
                                    const double ref = dx[(size_t)p * n + i];
                                    if (std::memcmp(&got, &ref, sizeof(double)) != 0 && !(std::isnan(got) && std::isnan(ref))) {
                                        printf("kind %d diag %d kappa %g reg %g problem %d output %d (%d,%d): %a, the JVP gives %a\n", kind, diag, kappa, reg, p, w, i, j, got, ref);
                                        ++fails;
                                    }
                                }
                        }
                    }
                }
    printf("jac_smooth_core_check: %d failures\n", fails);
    return fails == 0 ? 0 : 1;
}
#endif
