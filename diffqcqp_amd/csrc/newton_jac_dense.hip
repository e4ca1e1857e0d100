// newton_jac_dense.hip -- dqq_newton_jac_f64 on a general P (B,N,N): newton_core.h's newton_jac_problem by team_dense.h's
// teams and its multi-column elimination, one template with an LDS / global switch.
//   NewtonJacTeam (LDS = true, N <= 64): the slice in LDS.
//   NewtonJacAny (LDS = false, N > 64): a slice of the caller's scratch (dqq_newton_jac_scratch_bytes); the grid of any_grid.
// The slice: the matrix (N x (N|1): P while z is evaluated, then M in place), the block R of right-hand sides (N x C, row-major:
// row i, then the requested outputs' columns side by side -- Jq's N, Ja's and Jb's N or N/2), then x, z and the Jacobian.  All
// requested columns ride through one elimination: at N = 64 the box kinds' 3N columns make the slice 64 x 65 + 64 x 192 + 7 x 64
// doubles = 132.5 KB, one wave's workgroup in the 160 KB of LDS.
// R is row-major as J[b,i,:] is in memory, so the elimination's updates are conflict-free in LDS and coalesced in scratch, and
// the solution leaves with consecutive threads reading consecutive LDS words and writing consecutive addresses: no transpose.
#include "newton_core.h"
#include "team_dense.h"

// The proximal weight (polish_core.h): REG is a template parameter of every kernel here.  This file compiles the REG = false
// instantiations, which never read `reg`; newton_jac_dense_reg.hip defines DQQ_REG_UNIT and includes this file for the REG = true ones,
// which add reg to the diagonal entries of P where the thread that owns the entry forms M.
#ifndef DQQ_REG_UNIT
#define DQQ_REG_UNIT 0
#endif

namespace dqq {

constexpr bool kRegUnit = DQQ_REG_UNIT != 0;

// requested columns of (kind, N): Jq's N, Ja's and Jb's ne each
static DQQ_HD int jac_cols(const NewtonJacArgs& a, int ne)
{
    return (a.Jq != nullptr ? a.N : 0) + (a.Ja != nullptr ? ne : 0) + (a.Jb != nullptr ? ne : 0);
}
static DQQ_HD long jac_slice_doubles(int n, int ncol) { return ((long)n * (n | 1) + (long)n * ncol + newton_vec_doubles(n) + 1) & ~1L; }

// One problem by one team.  M: n x ld; R: n x nc; vec: newton_vec_doubles(n).
template <int KIND, int T, bool REG>
static DQQ_D void team_jac_problem(const NewtonJacArgs& a, double reg, long prob, double* M, double* R, double* vec, int nc, int lane)
{
#pragma clang fp contract(off)
    using ix = idx_t<T>;
    const int n = a.N, hc = n / 2;
    const ix ld = n | 1;
    const int ne = KIND == 0 ? 0 : (KIND == 1 ? hc : n);   // entries of an extra
    double* xc = vec;
    double* z = xc + n;
    double* dj = z + n;        // 2n
    double* ea = dj + 2 * n;   // the extras a, b, c as the core's functions read them (n each)
    double* eb = ea + n;
    double* ec = eb + n;
    const double* Pg = a.P + prob * (long)n * n;
    const long vo = prob * n, eo = prob * (long)ne;
    bool bad = false;
    for (ix idx = lane; idx < (ix)n * n; idx += T) {
        const double v = Pg[idx];
        bad = bad || !__builtin_isfinite(v);
        M[(idx / n) * ld + idx % n] = v;
    }
    for (int i = lane; i < n; i += T) {
        const double xi = a.x[vo + i];
        xc[i] = xi;
        bad = bad || !__builtin_isfinite(xi) || !__builtin_isfinite(a.q[vo + i]);
        if constexpr (KIND == 3) {
            const double ci = a.c[vo + i];
            ec[i] = ci;
            bad = bad || !__builtin_isfinite(ci);
        }
    }
    if constexpr (KIND >= 1)
        for (int k = lane; k < ne; k += T) {
            const double ak = a.a[eo + k], bk = a.b[eo + k];
            ea[k] = ak;
            eb[k] = bk;
            if constexpr (KIND >= 2) bad = bad || polish_lo_bad(ak, a.inf_bounds != 0) || polish_hi_bad(bk, a.inf_bounds != 0);
            else bad = bad || !__builtin_isfinite(ak) || !__builtin_isfinite(bk);
        }
    bad = team_any<T>(bad);
    team_sync<T>();
    for (int i = lane; i < n; i += T) {   // z: a row per thread
        double s = 0.0;
        for (int j = 0; j < n; ++j) s = polish_acc(s, M[i * ld + j], xc[j]);
        z[i] = polish_z(xc[i], s, a.q[vo + i]);
    }
    team_sync<T>();
    // the Jacobian as polish_eval leaves it (box-like: 1.0 where free)
    if constexpr (KIND == 1) {
        for (int k = lane; k < hc; k += T) {
            double D[3];
            polish_disc_jacobian(z[2 * k], z[2 * k + 1], ea[k] * eb[k], D);
            dj[3 * k] = D[0]; dj[3 * k + 1] = D[1]; dj[3 * k + 2] = D[2];
        }
    } else {
        for (int i = lane; i < n; i += T) {
            const int st = newton_box_state<KIND>(z[i], KIND >= 2 ? ea[i] : 0.0, KIND >= 2 ? eb[i] : 0.0, KIND == 3 ? ec[i] : 0.0);
            dj[i] = st == kNewtonFree ? 1.0 : 0.0;
        }
    }
    team_sync<T>();
    // the right-hand sides: an element per thread, consecutive threads on consecutive columns
    const int wq = a.Jq != nullptr ? n : 0, wa = a.Ja != nullptr ? ne : 0;
    for (ix idx = lane; idx < (ix)n * nc; idx += T) {
        const int i = (int)(idx / nc), c = (int)(idx % nc);
        const int which = c < wq ? 0 : (c < wq + wa ? 1 : 2), j = c < wq ? c : (c < wq + wa ? c - wq : c - wq - wa);
        R[idx] = newton_jac_rhs<KIND>(z, dj, ea, eb, ec, i, which, j);
    }
    // M in place of P (it does not read R)
    if constexpr (KIND == 1) {
        for (ix idx = lane; idx < (ix)hc * n; idx += T) {
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
        for (ix idx = lane; idx < (ix)n * n; idx += T) {
            const int i = (int)(idx / n), j = (int)(idx % n);
            if (dj[i] == 0.0) M[i * ld + j] = i == j ? 1.0 : 0.0;
            else if constexpr (REG) { if (i == j) M[i * ld + j] = polish_reg_add(M[i * ld + j], reg); }
        }
    }
    team_sync<T>();
    const bool ok = !bad && team_solve_multi<T>(M, ld, R, nc, n, lane);   // (bad is team-uniform: the team skips the solve together)
    team_sync<T>();
    const double nan = newton_nan();
    if (lane == 0 && a.status != nullptr) a.status[prob] = bad ? 2 : (ok ? 0 : 1);
    if (a.Jq != nullptr) {
        double* G = a.Jq + prob * (long)n * n;
        for (ix idx = lane; idx < (ix)n * n; idx += T)
            __builtin_nontemporal_store(ok ? R[(idx / n) * nc + idx % n] : nan, G + idx);
    }
    if constexpr (KIND >= 1) {
        if (a.Ja != nullptr) {
            double* G = a.Ja + prob * (long)n * ne;
            for (ix idx = lane; idx < (ix)n * ne; idx += T)
                __builtin_nontemporal_store(ok ? R[(idx / ne) * nc + wq + idx % ne] : nan, G + idx);
        }
        if (a.Jb != nullptr) {
            double* G = a.Jb + prob * (long)n * ne;
            for (ix idx = lane; idx < (ix)n * ne; idx += T)
                __builtin_nontemporal_store(ok ? R[(idx / ne) * nc + wq + wa + idx % ne] : nan, G + idx);
        }
    }
    team_sync<T>();   // the slice is the next problem's
}

template <int KIND, int T, bool LDS, bool REG>
__global__ __launch_bounds__(256) void newton_jac_dense_kernel(const NewtonJacArgs a, int nc, int lds_per_team, long scratch_stride,
                                                                       const double reg)
{
    const int n = a.N;
    const long mat = (long)n * (n | 1), blk = (long)n * nc;
    if constexpr (LDS) {
        extern __shared__ __attribute__((aligned(16))) double smem[];
        constexpr int TP = 64 / T; // teams per wave
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
        const int team = lane / T, tl = lane % T;
        double* sw = smem + (wave * TP + team) * lds_per_team;
        const long nteams = (long)gridDim.x * wpb * TP;
        // (a team past the end of the batch idles through the wave's fences: they are wave-wide, never team-wide)
        for (long w = ((long)blockIdx.x * wpb + wave) * TP + team; w < a.B; w += nteams)
            team_jac_problem<KIND, T, REG>(a, reg, w, sw, sw + mat, sw + mat + blk, nc, tl);
    } else {
        double* scr = a.scratch + (long)blockIdx.x * scratch_stride;
        for (long w = blockIdx.x; w < a.B; w += gridDim.x)
            team_jac_problem<KIND, T, REG>(a, reg, w, scr, scr + mat, scr + mat + blk, nc, (int)threadIdx.x);
    }
}

// NewtonJacAny's slice holds every column the kind has, whatever is requested: the scratch size depends on (kind, N, B) only
static long jac_any_stride(int kind, int N) { return jac_slice_doubles(N, N + 2 * newton_jac_extra_cols(kind, N)); }

#if !DQQ_REG_UNIT
size_t newton_jac_scratch_bytes(int kind, int N, long B) { return team_any_scratch_bytes(jac_any_stride(kind, N), B); }
#endif

#if DQQ_REG_UNIT
hipError_t launch_newton_jac_dense_reg(int kind, const NewtonJacArgs& a, double reg, bool any, hipStream_t s)
{
#else
hipError_t launch_newton_jac_dense(int kind, const NewtonJacArgs& a, bool any, hipStream_t s)
{
    const double reg = 0.0;
#endif
    // team_dense.h's launch: the LDS teams on the slice of the requested columns, the any-N form on the slice of all
    return dispatch_kind(kind, [&](auto k) {
        constexpr int KIND = decltype(k)::value;
        const int nc = jac_cols(a, newton_jac_extra_cols(KIND, a.N));
        const long slice = any ? jac_any_stride(KIND, a.N) : jac_slice_doubles(a.N, nc);
        return launch_team(a.N, a.B, any, slice, a.scratch, true, s, [&](auto t, auto lds, auto go, int lds_per_team, long stride) {
            return go(newton_jac_dense_kernel<KIND, decltype(t)::value, decltype(lds)::value, kRegUnit>, a, nc, lds_per_team, stride, reg);
        });
    });
}

} // namespace dqq
