// polish_dense.hip -- dqq_polish_f64 on a general P (B,N,N): polish_core.h's Newton iteration (polish_problem) by team_dense.h's
// teams on polish_team.h's slice, one template with an LDS / global switch.
//   PolishTeam (LDS = true, N <= 64): T = 8 .. 64 lanes, 64/T problems per wave, the slice in LDS.
//   PolishAny (LDS = false, N > 64): a 256-thread workgroup per problem on a slice of the caller's scratch
//     (dqq_polish_scratch_bytes); the persistent grid of any_grid.
#include "polish_team.h"

// The proximal weight (polish_core.h): REG is a template parameter of every kernel here.  This file compiles the REG = false
// instantiations, which never read `reg`; polish_dense_reg.hip defines DQQ_REG_UNIT and includes this file for the REG = true ones,
// which add reg to the diagonal entries of P where the thread that owns the entry forms M.
#ifndef DQQ_REG_UNIT
#define DQQ_REG_UNIT 0
#endif

namespace dqq {

constexpr bool kRegUnit = DQQ_REG_UNIT != 0;

// One problem by one team.  M: n x ld; vec: polish_vec_doubles(n).
template <int KIND, int T, bool REG>
static DQQ_D void team_polish_problem(const PolishArgs& a, double reg, long prob, double* M, double* vec, int lane)
{
#pragma clang fp contract(off)
    const int n = a.N, nc = n / 2;
    const idx_t<T> ld = n | 1;
    double* xc = vec;
    double* xn = xc + n;
    double* F = xn + n;
    double* z = F + n;
    double* d = z + n;
    double* dj = d + n;
    const double* Pg = a.P + prob * (long)n * n;
    bool bad = false, ignore = false;
    team_load_matrix<T>(M, ld, Pg, n, lane, bad);
    for (int i = lane; i < n; i += T) {
        const double xi = a.x[prob * n + i];
        xc[i] = xi;
        bad = bad || !__builtin_isfinite(xi) || !__builtin_isfinite(a.q[prob * n + i]);
        if constexpr (KIND >= 2)
            bad = bad || polish_lo_bad(a.a[prob * n + i], a.inf_bounds != 0) || polish_hi_bad(a.b[prob * n + i], a.inf_bounds != 0);
        if constexpr (KIND == 3) bad = bad || !__builtin_isfinite(a.c[prob * n + i]);
    }
    if constexpr (KIND == 1)
        for (int k = lane; k < nc; k += T) bad = bad || !__builtin_isfinite(a.a[prob * nc + k]) || !__builtin_isfinite(a.b[prob * nc + k]);
    bad = team_any<T>(bad);
    team_sync<T>();
    const double r0 = team_eval<KIND, T>(a, prob, n, M, ld, xc, z, F, dj, lane);
    double r = r0;
    int steps = 0;
    const bool run = !bad && __builtin_isfinite(r0);
    while (run && steps < a.max_steps && r != 0.0) {
        // M in place of P, and the right-hand side
        if constexpr (KIND == 1) {
            for (idx_t<T> idx = lane; idx < (idx_t<T>)nc * n; idx += T) {
                const int k = (int)(idx / n), j = (int)(idx % n);
                const double* D = dj + 3 * k;
                double pa = M[(2 * k) * ld + j], pb = M[(2 * k + 1) * ld + j];
                if constexpr (REG) {   // the contact's own two diagonal entries of P
                    if (j == 2 * k) pa = polish_reg_add(pa, reg);
                    if (j == 2 * k + 1) pb = polish_reg_add(pb, reg);
                }
                const double c0 = j == 2 * k ? D[0] : (j == 2 * k + 1 ? D[1] : 0.0);
                const double c1 = j == 2 * k ? D[1] : (j == 2 * k + 1 ? D[2] : 0.0);
                M[(2 * k) * ld + j] = polish_contact_entry(j == 2 * k, c0, D[0], D[1], pa, pb);
                M[(2 * k + 1) * ld + j] = polish_contact_entry(j == 2 * k + 1, c1, D[1], D[2], pa, pb);
            }
        } else {
            for (idx_t<T> idx = lane; idx < (idx_t<T>)n * n; idx += T) {
                const int i = (int)(idx / n), j = (int)(idx % n);
                if (dj[i] == 0.0) M[i * ld + j] = i == j ? 1.0 : 0.0;
                else if constexpr (REG) { if (i == j) M[i * ld + j] = polish_reg_add(M[i * ld + j], reg); }
            }
        }
        for (int i = lane; i < n; i += T) d[i] = -F[i];
        team_sync<T>();
        if (!team_solve<T>(M, ld, d, z, n, lane)) break;
        // the candidate, and P back into the matrix
        if constexpr (KIND == 1) {
            for (int k = lane; k < nc; k += T) {
                double ta = xc[2 * k] + z[2 * k], tb = xc[2 * k + 1] + z[2 * k + 1];
                check_proj_circle(ta, tb, a.a[prob * nc + k] * a.b[prob * nc + k]);
                xn[2 * k] = ta;
                xn[2 * k + 1] = tb;
            }
        } else {
            for (int i = lane; i < n; i += T) {
                double lo, hi;
                polish_bounds<KIND>(KIND >= 2 ? a.a[prob * n + i] : 0.0, KIND >= 2 ? a.b[prob * n + i] : 0.0,
                                    KIND == 3 ? a.c[prob * n + i] : 0.0, lo, hi);
                xn[i] = polish_proj<KIND>(xc[i] + z[i], lo, hi);
            }
        }
        team_load_matrix<T>(M, ld, Pg, n, lane, ignore);
        team_sync<T>();
        const double rn = team_eval<KIND, T>(a, prob, n, M, ld, xn, z, F, dj, lane);
        if (!(rn < r)) break;
        for (int i = lane; i < n; i += T) xc[i] = xn[i];
        r = rn;
        ++steps;
        team_sync<T>();
    }
    team_sync<T>();
    for (int i = lane; i < n; i += T) a.x_out[prob * n + i] = xc[i];
    if (lane == 0) {
        if (a.resid != nullptr) { a.resid[2 * prob] = r0; a.resid[2 * prob + 1] = r; }
        if (a.steps != nullptr) a.steps[prob] = steps;
        if (a.status != nullptr) a.status[prob] = polish_status(bad, r0, steps);
    }
    team_sync<T>();   // the slice is the next problem's
}

template <int KIND, int T, bool LDS, bool REG>
__global__ __launch_bounds__(256) void polish_dense_kernel(const PolishArgs a, int lds_per_team, long scratch_stride, const double reg)
{
    const int n = a.N;
    const long mat = (long)n * (n | 1);
    if constexpr (LDS) {
        extern __shared__ __attribute__((aligned(16))) double smem[];
        constexpr int TP = 64 / T; // teams per wave
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
        const int team = lane / T, tl = lane % T;
        double* sw = smem + (wave * TP + team) * lds_per_team;
        const long nteams = (long)gridDim.x * wpb * TP;
        // (a team past the end of the batch idles through the wave's fences: they are wave-wide, never team-wide)
        for (long w = ((long)blockIdx.x * wpb + wave) * TP + team; w < a.B; w += nteams)
            team_polish_problem<KIND, T, REG>(a, reg, w, sw, sw + mat, tl);
    } else {
        double* scr = a.scratch + (long)blockIdx.x * scratch_stride;
        for (long w = blockIdx.x; w < a.B; w += gridDim.x) team_polish_problem<KIND, T, REG>(a, reg, w, scr, scr + mat, (int)threadIdx.x);
    }
}

#if !DQQ_REG_UNIT
size_t polish_scratch_bytes(int N, long B) { return team_any_scratch_bytes(polish_any_stride(N), B); }
#endif

#if DQQ_REG_UNIT
hipError_t launch_polish_dense_reg(int kind, const PolishArgs& a, double reg, bool any, hipStream_t s)
{
#else
hipError_t launch_polish_dense(int kind, const PolishArgs& a, bool any, hipStream_t s)
{
    const double reg = 0.0;
#endif
    return dispatch_kind(kind, [&](auto k) {
        return launch_team(a.N, a.B, any, polish_slice_doubles(a.N), a.scratch, true, s, [&](auto t, auto lds, auto go, int lds_per_team, long stride) {
            return go(polish_dense_kernel<decltype(k)::value, decltype(t)::value, decltype(lds)::value, kRegUnit>, a, lds_per_team, stride, reg);
        });
    });
}

} // namespace dqq
