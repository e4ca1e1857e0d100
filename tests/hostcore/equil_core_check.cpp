// equil_core_check.cpp -- TEST ARTEFACT.  The power-of-two equilibration's arithmetic (diffqcqp_amd/csrc/equil_core.h) for the
// CPU: one problem at a time, plain loops over the coordinates where equil.hip has lanes, every exponent and every scaled value
// from the very functions the kernels call.  tests/test_equil_hostcore.py compares it with the numpy restatement
// (tests/equil_ref.py), tests/test_gpu_equil.py compares that with the device, bit for bit.  Nothing in the product links or
// loads this file.
#include "../../diffqcqp_amd/csrc/equil_core.h"

using namespace dqq;

namespace {

struct Problem {
    int n;
    bool diag;
    const double *P, *q, *a, *b, *c, *x0;
    double *P_out, *q_out, *a_out, *b_out, *c_out, *x0_out;
    int* e_out;
};

template <int KIND>
void run(const Problem& p)
{
    const int n = p.n;
    const auto d = [&p, n](int i) { return p.diag ? p.P[i] : p.P[(long)i * n + i]; };
    for (int i = 0; i < n; ++i) {
        const int e = equil_coord_exp<KIND>(d, i);
        p.e_out[i] = e;
        p.q_out[i] = equil_scale_q(p.q[i], e);
        if (p.x0_out != nullptr) p.x0_out[i] = equil_scale_bound(p.x0[i], e);
        if (KIND == 1 && (i & 1) == 0) {
            if (p.a_out != nullptr) p.a_out[i / 2] = equil_scale_bound(p.a[i / 2], e);
            if (p.b_out != nullptr) p.b_out[i / 2] = p.b[i / 2];
        }
        if (KIND == 2 || KIND == 3) {
            if (p.a_out != nullptr) p.a_out[i] = equil_scale_bound(p.a[i], e);
            if (p.b_out != nullptr) p.b_out[i] = equil_scale_bound(p.b[i], e);
        }
        if (KIND == 3 && p.c_out != nullptr) p.c_out[i] = p.c[i];
        if (p.diag) {
            p.P_out[i] = equil_scale_p(p.P[i], e, e);
        } else {
            for (int j = 0; j < n; ++j) p.P_out[(long)i * n + j] = equil_scale_p(p.P[(long)i * n + j], e, equil_coord_exp<KIND>(d, j));
        }
    }
}

} // namespace

extern "C" {

// one problem: kind 0..3, diag: P and P_out are the n diagonal entries; an output that is NULL is skipped; -> 0, or -1 for a
// kind or size the entry refuses
__attribute__((visibility("default"))) int hostequil(int kind, int diag, int n, const double* P, const double* q, const double* a,
                                                     const double* b, const double* c, const double* x0, double* P_out,
                                                     double* q_out, double* a_out, double* b_out, double* c_out, double* x0_out,
                                                     int* e_out)
{
    const Problem p{n, diag != 0, P, q, a, b, c, x0, P_out, q_out, a_out, b_out, c_out, x0_out, e_out};
    switch (kind) {
    case 0: run<0>(p); return 0;
    case 1: if (n % 2 != 0) return -1; run<1>(p); return 0;
    case 2: run<2>(p); return 0;
    case 3: run<3>(p); return 0;
    default: return -1;
    }
}

// equil_exp over n diagonal entries
__attribute__((visibility("default"))) void hostequil_exp(const double* p, int n, int* e)
{
    for (int i = 0; i < n; ++i) e[i] = equil_exp(p[i]);
}

__attribute__((visibility("default"))) void hostunscale(const double* y, const int* e, int n, double* x)
{
    for (int i = 0; i < n; ++i) x[i] = equil_unscale(y[i], e[i]);
}

} // extern "C"
