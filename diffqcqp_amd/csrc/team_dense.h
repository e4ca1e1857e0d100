// team_dense.h -- the dense team of the Newton family (polish_dense*.hip, newton_dense*.hip, newton_jac_dense.hip,
// active_dense.hip), stated once: a team of T threads works on one problem of a general P (B,N,N) in a slice of memory of its own.
//   T = 8 .. 64 (N <= 64): T adjacent lanes of a wave64, 64/T teams and problems per wave, the slice in LDS.  Lane l of the
//     team owns the elements l, l + T, .. of whatever is being formed.  What orders the phases is wave_lds_fence(): a fence is
//     wave-wide, never team-wide, so a team past the end of the batch idles through the fences of its wave's other teams, and
//     no team waits for another wave.
//   T = 256 ("Any", N > 64): a workgroup per problem on a slice of the caller's scratch, workgroup barriers between the phases.
// Every value is computed by exactly one thread.  What a team shares goes through the slice, and a value that depends on
// several elements -- the maximum of F, the pivot of a column -- is taken by EVERY thread with its own scan in index order: no
// reduction tree is involved, so the bits are the host core's (polish_core.h) whatever T is.
// The one launch of the eight dense units (launch_team) is here too; its geometry is that of dense.hip: launch_bwd_team.
#pragma once

#include <type_traits>

#include "launch.h"
#include "polish_core.h"

namespace dqq {

constexpr int kTeamAnyT = 256;

// element indices into a team's slice: int for the LDS teams (N <= 64), long for the Any team, whose N has no bound but memory
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

// P (n x n, dense) into the team's matrix (n x ld); bad: whether this thread met an element that is not finite
template <int T>
static DQQ_D void team_load_matrix(double* M, idx_t<T> ld, const double* __restrict__ src, int n, int lane, bool& bad)
{
    for (idx_t<T> idx = lane; idx < (idx_t<T>)n * n; idx += T) {
        const double v = src[idx];
        bad = bad || !__builtin_isfinite(v);
        M[(idx / n) * ld + idx % n] = v;
    }
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

// polish_solve_multi by a team: M R' = R in place (R: n x nc, row stride nc), the pivot rule of team_solve.  The elimination
// forms column k's multipliers in place, then updates the trailing matrix and R together, a thread per (row, column) element
// and consecutive threads on consecutive columns.  Team-uniform result.
template <int T>
static DQQ_D bool team_solve_multi(double* M, idx_t<T> ld, double* R, int nc, int n, int lane)
{
#pragma clang fp contract(off)
    using ix = idx_t<T>;
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
            for (int c = lane; c < nc; c += T) {
                const double t = R[(ix)k * nc + c];
                R[(ix)k * nc + c] = R[(ix)piv * nc + c];
                R[(ix)piv * nc + c] = t;
            }
            team_sync<T>();
        }
        const double pv = M[k * ld + k];
        for (int i = k + 1 + lane; i < n; i += T) M[i * ld + k] = M[i * ld + k] / pv;   // the multipliers, kept in place
        team_sync<T>();
        const ix rows = n - k - 1, wm = n - k - 1, w = wm + nc;   // a row of the update: the trailing matrix, then R
        for (ix idx = lane; idx < rows * w; idx += T) {
            const int i = k + 1 + (int)(idx / w), jj = (int)(idx % w);
            const double f = M[i * ld + k];
            if (polish_zero(f)) continue;
            if (jj < wm) {
                const int j = k + 1 + jj;
                M[i * ld + j] = M[i * ld + j] - f * M[k * ld + j];
            } else {
                const int c = jj - (int)wm;
                R[(ix)i * nc + c] = R[(ix)i * nc + c] - f * R[(ix)k * nc + c];
            }
        }
        team_sync<T>();
    }
    for (int k = n - 1; k >= 0; --k) {
        const double pv = M[k * ld + k];
        for (int c = lane; c < nc; c += T) R[(ix)k * nc + c] = R[(ix)k * nc + c] / pv;
        team_sync<T>();
        for (ix idx = lane; idx < (ix)k * nc; idx += T) {
            const int i = (int)(idx / nc), c = (int)(idx % nc);
            const double m = M[i * ld + k];
            if (!polish_zero(m)) R[(ix)i * nc + c] = R[(ix)i * nc + c] - m * R[(ix)k * nc + c];
        }
        team_sync<T>();
    }
    return true;
}

// The launch of the LDS teams for slices of `slice_doubles` doubles: as many waves per workgroup as fit 64 KiB of LDS (1 .. 4),
// a persistent grid of at most 256 * 8 workgroups.
struct TeamGeometry {
    int wpb;
    size_t lds_bytes;
    unsigned grid;
};

static inline TeamGeometry team_geometry(long slice_doubles, int T, long B)
{
    const int TP = 64 / T;
    const size_t per_wave = sizeof(double) * (size_t)slice_doubles * TP;
    int wpb = (int)((64 * 1024) / per_wave);
    wpb = wpb > 4 ? 4 : (wpb < 1 ? 1 : wpb);
    const long per_block = (long)wpb * TP;
    const long need = (B + per_block - 1) / per_block;
    const long cap = 256L * 8;
    return TeamGeometry{wpb, per_wave * wpb, (unsigned)(need < cap ? (need > 0 ? need : 1) : cap)};
}

// The team width of N: f(std::integral_constant<int, T>) with the smallest T = 8 .. 64 that is >= N.
static inline int team_width(int N) { return N <= 8 ? 8 : N <= 16 ? 16 : N <= 32 ? 32 : N <= 64 ? 64 : 0; }

template <typename F>
static inline hipError_t dispatch_team(int N, F&& f)
{
    switch (team_width(N)) {
    case 8: return f(std::integral_constant<int, 8>{});
    case 16: return f(std::integral_constant<int, 16>{});
    case 32: return f(std::integral_constant<int, 32>{});
    case 64: return f(std::integral_constant<int, 64>{});
    default: return hipErrorInvalidValue;
    }
}

// The launch of a dense unit, the dense analogue of diag_tile.h's launch_diag.  any: a kTeamAnyT-thread workgroup per problem on
// any_grid's persistent grid, each on a slice of `slice_doubles` doubles of the caller's scratch (any_scratch; without it the
// any-N form keeps nothing in global memory and its grid is any_grid(B, 1)); else the LDS teams of N's width on team_geometry.
// f(t, lds, go, lds_per_team, scratch_stride) names the kernel instantiation for the two integral constants and hands it, with
// the kernel's arguments, to go:
//   [&](auto t, auto lds, auto go, int lds_per_team, long stride) { return go(x_kernel<KIND, t(), lds()>, a, lds_per_team, stride); }
template <typename F>
static inline hipError_t launch_team(int N, long B, bool any, long slice_doubles, const double* scratch, bool any_scratch,
                                     hipStream_t s, F&& f)
{
    if (any) {
        if (any_scratch && scratch == nullptr) return hipErrorInvalidValue; // capi.hip checks the workspace before it gets here
        const long stride = any_scratch ? slice_doubles : 0;
        auto go = [&](auto kernel, const auto&... args) {
            return launch(kernel, dim3(any_grid(B, any_scratch ? stride : 1)), dim3(kTeamAnyT), 0, s, args...);
        };
        return f(std::integral_constant<int, kTeamAnyT>{}, std::false_type{}, go, 0, stride);
    }
    return dispatch_team(N, [&](auto t) {
        const TeamGeometry g = team_geometry(slice_doubles, t, B);
        auto go = [&](auto kernel, const auto&... args) {
            return launch_lds(kernel, dim3(g.grid), dim3(64 * g.wpb), g.lds_bytes, s, args...);
        };
        return f(t, std::true_type{}, go, (int)slice_doubles, 0L);
    });
}

// bytes of scratch the any-N form of a unit needs for slices of `stride` doubles: one per workgroup of any_grid (0 for B <= 0)
static inline size_t team_any_scratch_bytes(long stride, long B)
{
    return B <= 0 ? 0 : sizeof(double) * (size_t)stride * any_grid(B, stride);
}

} // namespace dqq
