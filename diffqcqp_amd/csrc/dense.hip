// dense.hip -- stand-alone kernels of the general (non-diagonal P) path: one wave64 per problem
// (dense_core.h), persistent over the batch or over the fallback work-list the diagonal fast paths
// fill for the tiles they cannot take.
#include "dense_core.h"
#include "launch.h"
#include "worklist.h"

namespace dqq {

// Workgroups hold `wpb` independent waves (wave-private LDS slices, no workgroup barrier): more waves
// per dispatched workgroup keeps the launch cheap when the work-list turns out to be empty.
template <int KIND>
__global__ __launch_bounds__(256) void fwd_dense_kernel(const double* __restrict__ P, const double* __restrict__ q,
                                                        const double* __restrict__ l_n,
                                                        const double* __restrict__ mu_c,
                                                        const double* __restrict__ v_sign, double* __restrict__ x, long B,
                                                        int n, double eps, double mu, int max_iter, int adaptive,
                                                        int* __restrict__ iters, int* __restrict__ ws, int use_worklist,
                                                        int lds_per_wave, const double* __restrict__ x0)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    double* sw = smem + wave * lds_per_wave;
    const long count = use_worklist ? worklist_count(ws, n, B) : B;
    const long nwaves = (long)gridDim.x * wpb;
    for (long w = (long)blockIdx.x * wpb + wave; w < count; w += nwaves) {
        const long prob = use_worklist ? worklist_entry(ws, n, B, w) : w;
        dense_fwd_problem<KIND>(P, q, l_n, mu_c, v_sign, x, iters, prob, n, eps, mu, max_iter, adaptive, sw, lane, x0);
    }
    if (use_worklist && lane == 0) worklist_release(ws, count, (int)nwaves);
}

// Backward: 64/T problems per wave (dense_core.h: team width T), each team in its own LDS slice.
template <int KIND, int T>
__global__ __launch_bounds__(256) void bwd_dense_kernel(
    const double* __restrict__ P, const double* __restrict__ q, const double* __restrict__ l_n,
    const double* __restrict__ mu_c, const double* __restrict__ x, const double* __restrict__ grad_x,
    double* __restrict__ grad_P, double* __restrict__ grad_q, double* __restrict__ grad_l_n,
    double* __restrict__ grad_mu, double* __restrict__ gamma_out, double* __restrict__ dgamma_out, long B, int n,
    double dual_eps, int* __restrict__ ir_steps, int* __restrict__ ws, int use_worklist, int lds_per_team,
    const double* __restrict__ v_sign)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int TP = 64 / T; // teams per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int team = lane / T, tl = lane % T;
    double* sw = smem + (wave * TP + team) * lds_per_team;
    const long count = use_worklist ? worklist_count(ws, n, B) : B;
    const long nteams = (long)gridDim.x * wpb * TP;
    for (long w = ((long)blockIdx.x * wpb + wave) * TP + team; w < count; w += nteams) {
        const long prob = use_worklist ? worklist_entry(ws, n, B, w) : w;
        dense_bwd_problem<KIND, T>(P, q, l_n, mu_c, x, grad_x, grad_P, grad_q, grad_l_n, grad_mu, gamma_out, dgamma_out,
                                   ir_steps, prob, n, dual_eps, sw, tl, v_sign);
    }
    if (use_worklist && lane == 0) worklist_release(ws, count, (int)(gridDim.x * wpb));
}

// ---------------------------------------------------------------- launchers
// waves per workgroup: as many (<= 4) as fit in 64 KiB of LDS; doubles per wave rounded to 16 B
struct DenseGeom {
    int wpb, lds_per_wave;
    size_t lds_bytes;
    unsigned grid;
};
static DenseGeom dense_geom(int lds_doubles, long B, bool use_worklist)
{
    DenseGeom g;
    g.lds_per_wave = (lds_doubles + 1) & ~1;
    const size_t per_wave = sizeof(double) * (size_t)g.lds_per_wave;
    g.wpb = (int)((64 * 1024) / per_wave);
    if (g.wpb > 4) g.wpb = 4;
    if (g.wpb < 1) g.wpb = 1;
    g.lds_bytes = per_wave * g.wpb;
    // persistent waves loop over the problems; in work-list mode the size of the list is only known on
    // the device, so a fixed 512 workgroups are dispatched (an empty list costs one short launch)
    const long cap = 256L * 16 / g.wpb * (g.wpb > 1 ? 2 : 1);
    const long need = (B + g.wpb - 1) / g.wpb;
    g.grid = (unsigned)(need < (use_worklist ? 512L : cap) ? (need > 0 ? need : 1) : (use_worklist ? 512L : cap));
    return g;
}

template <int KIND>
static hipError_t launch_fwd_wave(const FwdArgs& a, bool use_worklist, hipStream_t s)
{
    const DenseGeom g = dense_geom(dense_fwd_lds_doubles(a.N), a.B, use_worklist);
    return launch_lds(fwd_dense_kernel<KIND>, dim3(g.grid), dim3(64 * g.wpb), g.lds_bytes, s, a.P, a.q, a.l_n, a.mu, a.v,
                       a.x, a.B, a.N, a.eps, a.mu_prox, a.max_iter, a.adaptive, a.iters, a.ws, use_worklist ? 1 : 0,
                       g.lds_per_wave, a.x0);
}

hipError_t launch_fwd_dense(int kind, const FwdArgs& a, bool use_worklist, hipStream_t s)
{
    switch (kind) {
    case 0: return launch_fwd_wave<0>(a, use_worklist, s);
    case 1: return launch_fwd_wave<1>(a, use_worklist, s);
    case 2: return launch_fwd_wave<2>(a, use_worklist, s);
    case 3: return launch_fwd_wave<3>(a, use_worklist, s);
    default: return hipErrorInvalidValue;
    }
}

template <int KIND, int T>
static hipError_t launch_bwd_team(const BwdArgs& a, bool use_worklist, hipStream_t s)
{
    constexpr int TP = 64 / T;
    const int lds_per_team = (dense_bwd_lds_doubles(KIND, a.N) + 1) & ~1;
    const size_t per_wave = sizeof(double) * (size_t)lds_per_team * TP;
    int wpb = (int)((64 * 1024) / per_wave);
    wpb = wpb > 4 ? 4 : (wpb < 1 ? 1 : wpb);
    const size_t lds_bytes = per_wave * wpb;
    const long per_block = (long)wpb * TP;
    const long need = (a.B + per_block - 1) / per_block;
    const long cap = 256L * 8;
    const unsigned grid = (unsigned)(need < (use_worklist ? 512L : cap) ? (need > 0 ? need : 1) : (use_worklist ? 512L : cap));
    return launch_lds(bwd_dense_kernel<KIND, T>, dim3(grid), dim3(64 * wpb), lds_bytes, s, a.P, a.q, a.l_n, a.mu, a.x, a.grad_x, a.grad_P,
                       a.grad_q, a.grad_l_n, a.grad_mu, a.gamma, a.dgamma, a.B, a.N, a.epsilon, a.ir_steps, a.ws,
                       use_worklist ? 1 : 0, lds_per_team, a.v);
}

template <int KIND>
static hipError_t launch_bwd_kind(const BwdArgs& a, bool use_worklist, hipStream_t s)
{
    const int rows = bwd_system_rows(KIND, a.N); // lanes a problem needs
    if (knob_dense_teams() != 0) {
        if (rows <= 8) return launch_bwd_team<KIND, 8>(a, use_worklist, s);
        if (rows <= 16) return launch_bwd_team<KIND, 16>(a, use_worklist, s);
        if (rows <= 32) return launch_bwd_team<KIND, 32>(a, use_worklist, s);
    }
    return launch_bwd_team<KIND, 64>(a, use_worklist, s);
}

hipError_t launch_bwd_dense(int kind, const BwdArgs& a, bool use_worklist, hipStream_t s)
{
    if (kind == kKindBox) return launch_bwd_kind<2>(a, use_worklist, s);
    if (kind == kKindSignedBox) return launch_bwd_kind<3>(a, use_worklist, s);
    return kind == 0 ? launch_bwd_kind<0>(a, use_worklist, s) : launch_bwd_kind<1>(a, use_worklist, s);
}

} // namespace dqq
