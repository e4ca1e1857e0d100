// polish_dense.hip -- dqq_polish_f64 on a general P (B,N,N): polish_core.h's Newton iteration by a team of T threads per
// problem, one template with an LDS / global switch.
//   PolishTeam (LDS = true, N <= 64): dense.hip's backward teams -- T = 8 .. 64 lanes, 64/T problems per wave, the team's
//     matrix and vectors in its LDS slice, wave fences between the phases; the launch geometry of launch_bwd_team.
//   PolishAny (LDS = false, N > 64): a 256-thread workgroup per problem on a slice of the caller's scratch
//     (dqq_polish_scratch_bytes), workgroup barriers between the phases; the persistent grid of any_grid.
// The slice: the matrix (N x (N|1): P while x is evaluated, then M in place, reloaded from P after the solve), then x, x+, F,
// z (the solution d after the solve), the right-hand side and the Jacobian (2N).
//
// Every value is computed by exactly one thread with polish_core.h's element functions in polish_problem's order; what a
// team shares goes through the slice: each thread takes the maximum of F, and the pivot of a column, by its own scan in
// index order, so no reduction tree is involved and the bits are the host core's.  Unit rows and exact zeros are skipped
// where polish_solve skips them.
#include <type_traits>

#include "launch.h"
#include "polish_core.h"

// The proximal weight (polish_core.h): REG is a template parameter of every kernel here.  This file compiles the REG = false
// instantiations, which never read `reg`; polish_dense_reg.hip defines DQQ_REG_UNIT and includes this file for the REG = true ones,
// which add reg to the diagonal entries of P where the thread that owns the entry forms M.
#ifndef DQQ_REG_UNIT
#define DQQ_REG_UNIT 0
#endif

namespace dqq {

constexpr bool kRegUnit = DQQ_REG_UNIT != 0;

constexpr int kPolishAnyT = 256;

// element indices into a team's slice: int for the LDS teams (N <= 64), long for PolishAny, whose N has no bound but memory
template <int T>
using idx_t = std::conditional_t<(T <= 64), int, long>;

template <int T>
static DQQ_D void team_sync()
{
    if constexpr (T <= 64) wave_lds_fence();
    else __syncthreads();
}

template <int T>
static DQQ_D bool team_any(bool pred)
{
    if constexpr (T == 64) return __ballot(pred) != 0ull;
    else if constexpr (T < 64) return ((__ballot(pred) >> (((threadIdx.x & 63) / T) * T)) & ((1ull << T) - 1ull)) != 0ull;
    else return __syncthreads_or(pred ? 1 : 0) != 0;
}

static DQQ_HD long polish_slice_doubles(int n) { return ((long)n * (n | 1) + polish_vec_doubles(n) + 1) & ~1L; }

// z, F, the Jacobian and r at xv; M holds P.  Every thread returns r.
template <int KIND, int T>
static DQQ_D double team_eval(const PolishArgs& a, long prob, int n, const double* M, idx_t<T> ld, const double* xv, double* z,
                              double* F, double* dj, int lane)
{
#pragma clang fp contract(off)
    for (int i = lane; i < n; i += T) {
        double s = 0.0;
        for (int j = 0; j < n; ++j) s = polish_acc(s, M[i * ld + j], xv[j]);
        z[i] = polish_z(xv[i], s, a.q[prob * n + i]);
    }
    team_sync<T>();
    if constexpr (KIND == 1) {
        const int nc = n / 2;
        for (int k = lane; k < nc; k += T) {
            const double rad = a.a[prob * nc + k] * a.b[prob * nc + k];
            polish_F_contact(xv[2 * k], xv[2 * k + 1], z[2 * k], z[2 * k + 1], rad, F[2 * k], F[2 * k + 1]);
            double D[3];
            polish_disc_jacobian(z[2 * k], z[2 * k + 1], rad, D);
            dj[3 * k] = D[0]; dj[3 * k + 1] = D[1]; dj[3 * k + 2] = D[2];
        }
    } else {
        for (int i = lane; i < n; i += T) {
            double lo, hi;
            polish_bounds<KIND>(KIND >= 2 ? a.a[prob * n + i] : 0.0, KIND >= 2 ? a.b[prob * n + i] : 0.0,
                                KIND == 3 ? a.c[prob * n + i] : 0.0, lo, hi);
            F[i] = polish_F<KIND>(xv[i], z[i], lo, hi);
            dj[i] = polish_free(z[i], lo, hi) ? 1.0 : 0.0;
        }
    }
    team_sync<T>();
    double r = 0.0;
    for (int i = 0; i < n; ++i) r = nmax(r, F[i]);
    return r;
}

// polish_solve by a team: M d = rhs in place, the solution into sol.  Team-uniform result.
template <int T>
static DQQ_D bool team_solve(double* M, idx_t<T> ld, double* d, double* sol, int n, int lane)
{
#pragma clang fp contract(off)
    for (int k = 0; k < n; ++k) {
        double best = fabs(M[k * ld + k]);
        int piv = k;
        for (int i = k + 1; i < n; ++i) {
            const double v = fabs(M[i * ld + k]);
            if (v > best) { best = v; piv = i; }
        }
        if (!polish_pivot_ok(best)) return false;
        team_sync<T>();   // the column has been read by everybody
        if (piv != k) {
            for (int j = k + lane; j < n; j += T) { const double t = M[k * ld + j]; M[k * ld + j] = M[piv * ld + j]; M[piv * ld + j] = t; }
            if (lane == 0) { const double t = d[k]; d[k] = d[piv]; d[piv] = t; }
            team_sync<T>();
        }
        const double pv = M[k * ld + k], dk = d[k];
        for (int i = k + 1 + lane; i < n; i += T) {
            const double f = M[i * ld + k] / pv;
            M[i * ld + k] = f;
            if (!polish_zero(f)) d[i] = d[i] - f * dk;
        }
        team_sync<T>();
        const idx_t<T> w = n - k - 1;
        for (idx_t<T> idx = lane; idx < w * w; idx += T) {
            const int i = k + 1 + (int)(idx / w), j = k + 1 + (int)(idx % w);
            const double f = M[i * ld + k];
            if (!polish_zero(f)) M[i * ld + j] = M[i * ld + j] - f * M[k * ld + j];
        }
        team_sync<T>();
    }
    for (int k = n - 1; k >= 0; --k) {
        const double dk = d[k] / M[k * ld + k];
        if (lane == 0) sol[k] = dk;
        for (int i = lane; i < k; i += T) {   // (d[k] itself is not written: no fence between its read and these)
            const double m = M[i * ld + k];
            if (!polish_zero(m)) d[i] = d[i] - m * dk;
        }
        team_sync<T>();
    }
    return true;
}

template <int T>
static DQQ_D void team_load_matrix(double* M, idx_t<T> ld, const double* __restrict__ src, int n, int lane, bool& bad)
{
    for (idx_t<T> idx = lane; idx < (idx_t<T>)n * n; idx += T) {
        const double v = src[idx];
        bad = bad || !__builtin_isfinite(v);
        M[(idx / n) * ld + idx % n] = v;
    }
}

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

static long polish_any_stride(int N) { return polish_slice_doubles(N); }

#if !DQQ_REG_UNIT && !defined(DQQ_POLISH_LS_UNIT)
size_t polish_scratch_bytes(int N, long B)
{
    if (B <= 0) return 0;
    const long stride = polish_any_stride(N);
    return sizeof(double) * (size_t)stride * any_grid(B, stride);
}
#endif

// the geometry of dense.hip: launch_bwd_team
template <int KIND, int T>
static hipError_t launch_polish_team(const PolishArgs& a, double reg, hipStream_t s)
{
    constexpr int TP = 64 / T;
    const int lds_per_team = (int)polish_slice_doubles(a.N);
    const size_t per_wave = sizeof(double) * (size_t)lds_per_team * TP;
    int wpb = (int)((64 * 1024) / per_wave);
    wpb = wpb > 4 ? 4 : (wpb < 1 ? 1 : wpb);
    const size_t lds_bytes = per_wave * wpb;
    const long per_block = (long)wpb * TP;
    const long need = (a.B + per_block - 1) / per_block;
    const long cap = 256L * 8;
    const unsigned grid = (unsigned)(need < cap ? (need > 0 ? need : 1) : cap);
    return launch_lds(polish_dense_kernel<KIND, T, true, kRegUnit>, dim3(grid), dim3(64 * wpb), lds_bytes, s, a, lds_per_team, 0L, reg);
}

template <int KIND>
static hipError_t launch_polish_kind(const PolishArgs& a, double reg, bool any, hipStream_t s)
{
    if (any) {
        if (a.scratch == nullptr) return hipErrorInvalidValue; // capi.hip checks the workspace before it gets here
        const long stride = polish_any_stride(a.N);
        return launch(polish_dense_kernel<KIND, kPolishAnyT, false, kRegUnit>, dim3(any_grid(a.B, stride)), dim3(kPolishAnyT), 0, s,
                      a, 0, stride, reg);
    }
    if (a.N <= 8) return launch_polish_team<KIND, 8>(a, reg, s);
    if (a.N <= 16) return launch_polish_team<KIND, 16>(a, reg, s);
    if (a.N <= 32) return launch_polish_team<KIND, 32>(a, reg, s);
    if (a.N <= 64) return launch_polish_team<KIND, 64>(a, reg, s);
    return hipErrorInvalidValue;
}

// (polish_dense_ls.hip includes this file for the helpers above and has its own kernel and entry point)
#ifndef DQQ_POLISH_LS_UNIT
#if DQQ_REG_UNIT
hipError_t launch_polish_dense_reg(int kind, const PolishArgs& a, double reg, bool any, hipStream_t s)
{
#else
hipError_t launch_polish_dense(int kind, const PolishArgs& a, bool any, hipStream_t s)
{
    const double reg = 0.0;
#endif
    switch (kind) {
    case kKindQP: return launch_polish_kind<0>(a, reg, any, s);
    case kKindQCQP: return launch_polish_kind<1>(a, reg, any, s);
    case kKindBox: return launch_polish_kind<2>(a, reg, any, s);
    case kKindSignedBox: return launch_polish_kind<3>(a, reg, any, s);
    default: return hipErrorInvalidValue;
    }
}
#endif

} // namespace dqq
