// warm_check.cpp -- TEST ARTEFACT.  What tests/test_warm_routes.py needs of the warm-started forward on a machine without a
// GPU: the route plan (route.cpp: plan_fwd_warm next to plan_fwd, in route_check.cpp's rendering) and the warm prologues of
// the diagonal path (admm_core.h, one "lane" per problem) and of the lane-per-problem kernel (warm_start.h), compiled for
// the host.  Nothing in the product links or loads this file.
#include "../../diffqcqp_amd/csrc/route.cpp"
#include "../../diffqcqp_amd/csrc/admm_core.h"
#include "../../diffqcqp_amd/csrc/warm_start.h"

using namespace dqq;

template <int KIND, int E>
static int diag_one(const double* p, const double* q, const double* a, const double* b, const double* c, const double* x0,
                    double eps, double mu, int max_iter, double* x)
{
    double pp[E], qq[E], xx[E], rr[E / 2], lo[E], hi[E], sg[E], xs[E];
    for (int e = 0; e < E; ++e) {
        pp[e] = p[e]; qq[e] = q[e]; xs[e] = x0[e];
        lo[e] = KIND >= 2 ? a[e] : 0.0;
        hi[e] = KIND >= 2 ? b[e] : 0.0;
        sg[e] = KIND == 3 ? (double)((c[e] > 0) - (c[e] < 0)) : 0.0;
    }
    for (int k = 0; k < E / 2; ++k) rr[k] = KIND == 1 ? a[k] * b[k] : 0.0;
    const int it = admm_fwd_diag<KIND, E, HostGroup, true>(pp, qq, rr, E, eps, mu, max_iter, 1, true, xx, lo, hi, sg, xs);
    for (int e = 0; e < E; ++e) x[e] = xx[e];
    return it;
}

extern "C" {

// route_check.cpp's route_plan, with warm != 0: plan_fwd_warm
__attribute__((visibility("default"))) void warm_route_plan(int warm, int kind, int N, long long B, int p_layout,
                                                            const int* knobs, int* out)
{
    const Knobs k{knobs[0], knobs[1], knobs[2], knobs[3], knobs[4], knobs[5], knobs[6], knobs[7]};
    Plan p;
    if ((p.err = check_call(kind, B, N, p_layout)) == 0)
        p = warm ? plan_fwd_warm(kind, N, B, p_layout, k) : plan_fwd(kind, N, B, p_layout, k);
    int* o = out;
    *o++ = p.err;
    *o++ = p.keep;
    *o++ = p.worklist;
    *o++ = p.scratch;
    const Launch* launches[] = {&p.first, &p.drain};
    for (const Launch* l : launches) {
        *o++ = (int)l->family;
        *o++ = l->lpp;
        *o++ = l->fuse;
        *o++ = l->lane_mode;
        *o++ = (int)l->counter;
    }
}

__attribute__((visibility("default"))) int warm_family_built(int family) { return fwd_family_warm((Family)family) ? 1 : 0; }

// the warm diagonal forward of one N = 8 problem (a, b, c: the kind's extras) -> iterations executed
__attribute__((visibility("default"))) int warm_diag_fwd8(int kind, const double* p, const double* q, const double* a,
                                                          const double* b, const double* c, const double* x0, double eps,
                                                          double mu, int max_iter, double* x)
{
    switch (kind) {
    case 0: return diag_one<0, 8>(p, q, a, b, c, x0, eps, mu, max_iter, x);
    case 1: return diag_one<1, 8>(p, q, a, b, c, x0, eps, mu, max_iter, x);
    case 2: return diag_one<2, 8>(p, q, a, b, c, x0, eps, mu, max_iter, x);
    case 3: return diag_one<3, 8>(p, q, a, b, c, x0, eps, mu, max_iter, x);
    default: return -1;
    }
}

// the lane-per-problem kernel's warm state of one dense N = 8 problem: out = l2 (8), u (8), q_prox (8) -> bad
__attribute__((visibility("default"))) int warm_lane_state8(const double* P, const double* q, const double* x0, double mu,
                                                            double* out)
{
    double Pm[8][8], qq[8], xs[8], qp[8], l2[8], u[8];
    for (int i = 0; i < 8; ++i) {
        qq[i] = q[i]; xs[i] = x0[i];
        for (int j = 0; j < 8; ++j) Pm[i][j] = P[i * 8 + j];
    }
    bool bad = false;
    lane_warm_state<8>(Pm, qq, xs, mu, qp, l2, u, bad);
    for (int i = 0; i < 8; ++i) { out[i] = l2[i]; out[8 + i] = u[i]; out[16 + i] = qp[i]; }
    return bad ? 1 : 0;
}

} // extern "C"
