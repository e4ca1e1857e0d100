// newton_jac_dense_smooth.hip -- dqq_newton_jac_smooth_f64 (kappa > 0) on a general P (B,N,N): smooth_core.h's
// newton_jac_problem_smooth by team_dense.h's teams and its multi-column elimination.  newton_jac_dense.hip's template (an LDS /
// global switch), slice, launch geometry, persistence loop and scratch (dqq_newton_jac_scratch_bytes):
//   NewtonJacSmoothTeam (LDS = true, N <= 64): the slice in LDS.
//   NewtonJacSmoothAny (LDS = false, N > 64): a slice of the caller's scratch; the grid of any_grid.
// The slice: the matrix (N x (N|1): P while z is evaluated, then the smoothed M in place), the block R of right-hand sides
// (N x C, row-major: the requested outputs' columns side by side), then x, z, the Jacobian of PI_k (2N: D_i, or three per contact)
// and the extras -- not a double more than the hard kernel's (132.5 KB at N = 64 for the box kinds).  E is not kept: the thread
// that writes a right-hand-side entry takes it again from z (smooth_box_at / smooth_disc are functions of z, the extras and
// kappa alone, so the bits are the first evaluation's); a thread walks the rows and evaluates a row's D and E once for all the
// columns it owns in that row: n evaluations on each of the first min(T, C) threads, against n C / T on every thread for an
// element per thread -- fewer where C >= T (every LDS team with all outputs requested but the QP's below N = T), more for the
// any-N form's 256 threads while C < 256 (N = 66: 66 against about 51 for the box kinds); neither form has been timed.
// M is dense in every row; kappa and the proximal weight are read at run time from the second kernel argument (polish_reg).
// kappa == 0 never gets here: capi.hip sends it to newton_jac_dense*.hip.
#include "smooth_core.h"
#include "team_dense.h"

namespace dqq {

// newton_jac_dense.hip's: requested columns of (kind, N), and the slice
static DQQ_HD int jac_smooth_cols(const NewtonJacArgs& a, int ne)
{
    return (a.Jq != nullptr ? a.N : 0) + (a.Ja != nullptr ? ne : 0) + (a.Jb != nullptr ? ne : 0);
}
static DQQ_HD long jac_smooth_slice_doubles(int n, int ncol) { return ((long)n * (n | 1) + (long)n * ncol + newton_vec_doubles(n) + 1) & ~1L; }

// One problem by one team.  M: n x ld; R: n x nc; vec: newton_vec_doubles(n).
template <int KIND, int T>
static DQQ_D void team_jac_smooth_problem(const NewtonJacArgs& a, const NewtonJacSmoothOpts& o, long prob, double* M, double* R,
                                          double* vec, int nc, int lane)
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
    const double reg = o.reg, kappa = o.kappa;
    bool bad = false;
    team_load_matrix<T>(M, ld, Pg, n, lane, bad);
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
            bad = bad || !__builtin_isfinite(ak) || !__builtin_isfinite(bk);   // (no one-sided boxes under smoothing)
        }
    bad = team_any<T>(bad);
    team_sync<T>();
    for (int i = lane; i < n; i += T) {   // z: a row per thread
        double s = 0.0;
        for (int j = 0; j < n; ++j) s = polish_acc(s, M[i * ld + j], xc[j]);
        z[i] = polish_z(xc[i], s, a.q[vo + i]);
    }
    team_sync<T>();
    // the Jacobian of PI_k as smooth_eval leaves it
    if constexpr (KIND == 1) {
        for (int k = lane; k < hc; k += T) {
            const SmoothDisc s = smooth_disc(z[2 * k], z[2 * k + 1], ea[k] * eb[k], kappa);
            dj[3 * k] = s.D[0]; dj[3 * k + 1] = s.D[1]; dj[3 * k + 2] = s.D[2];
        }
    } else {
        for (int i = lane; i < n; i += T)
            dj[i] = smooth_box_at<KIND>(z[i], KIND >= 2 ? ea[i] : 0.0, KIND >= 2 ? eb[i] : 0.0, KIND == 3 ? ec[i] : 0.0, kappa).D;
    }
    // the right-hand sides (they read z and the extras, not dj): row by row, consecutive threads on consecutive columns
    const int wq = a.Jq != nullptr ? n : 0, wa = a.Ja != nullptr ? ne : 0;
    if (lane < nc)
        for (int i = 0; i < n; ++i) {
            if constexpr (KIND == 1) {
                const int k = i / 2;
                const double ln = ea[k], mc = eb[k];
                const SmoothDisc s = smooth_disc(z[2 * k], z[2 * k + 1], ln * mc, kappa);
                for (int c = lane; c < nc; c += T) {
                    const int which = c < wq ? 0 : (c < wq + wa ? 1 : 2), j = c < wq ? c : (c < wq + wa ? c - wq : c - wq - wa);
                    const bool ha = which == 0 ? j == 2 * k : j == k, hb = which == 0 && j == 2 * k + 1;
                    R[(ix)i * nc + c] = smooth_jac_contact_rhs(s, i & 1, ln, mc, which, ha, hb);
                }
            } else {
                const SmoothBox s = smooth_box_at<KIND>(z[i], KIND >= 2 ? ea[i] : 0.0, KIND >= 2 ? eb[i] : 0.0, KIND == 3 ? ec[i] : 0.0, kappa);
                for (int c = lane; c < nc; c += T) {
                    const int which = c < wq ? 0 : (c < wq + wa ? 1 : 2), j = c < wq ? c : (c < wq + wa ? c - wq : c - wq - wa);
                    R[(ix)i * nc + c] = smooth_jac_box_rhs(s, which, i == j);
                }
            }
        }
    team_sync<T>();
    // M in place of P (it does not read R)
    if constexpr (KIND == 1) {
        for (ix idx = lane; idx < (ix)hc * n; idx += T) {
            const int k = (int)(idx / n), j = (int)(idx % n);
            const double* D = dj + 3 * k;
            double pa = M[(2 * k) * ld + j], pb = M[(2 * k + 1) * ld + j];
            if (j == 2 * k) pa = polish_reg(pa, reg);   // the contact's own two diagonal entries of P
            if (j == 2 * k + 1) pb = polish_reg(pb, reg);
            const double c0 = j == 2 * k ? D[0] : (j == 2 * k + 1 ? D[1] : 0.0);
            const double c1 = j == 2 * k ? D[1] : (j == 2 * k + 1 ? D[2] : 0.0);
            M[(2 * k) * ld + j] = polish_contact_entry(j == 2 * k, c0, D[0], D[1], pa, pb);
            M[(2 * k + 1) * ld + j] = polish_contact_entry(j == 2 * k + 1, c1, D[1], D[2], pa, pb);
        }
    } else {
        for (ix idx = lane; idx < (ix)n * n; idx += T) {
            const int i = (int)(idx / n), j = (int)(idx % n);
            const double pij = M[i * ld + j];
            M[i * ld + j] = smooth_box_entry(i == j, dj[i], i == j ? polish_reg(pij, reg) : pij);
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

template <int KIND, int T, bool LDS>
__global__ __launch_bounds__(256) void newton_jac_dense_smooth_kernel(const NewtonJacArgs a, const NewtonJacSmoothOpts o, int nc,
                                                                      int lds_per_team, long scratch_stride)
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
            team_jac_smooth_problem<KIND, T>(a, o, w, sw, sw + mat, sw + mat + blk, nc, tl);
    } else {
        double* scr = a.scratch + (long)blockIdx.x * scratch_stride;
        for (long w = blockIdx.x; w < a.B; w += gridDim.x)
            team_jac_smooth_problem<KIND, T>(a, o, w, scr, scr + mat, scr + mat + blk, nc, (int)threadIdx.x);
    }
}

hipError_t launch_newton_jac_dense_smooth(int kind, const NewtonJacArgs& a, const NewtonJacSmoothOpts& o, bool any, hipStream_t s)
{
    // team_dense.h's launch, as newton_jac_dense.hip's: the LDS teams on the slice of the requested columns, the any-N form on the
    // slice of all (dqq_newton_jac_scratch_bytes sizes its scratch)
    return dispatch_kind(kind, [&](auto k) {
        constexpr int KIND = decltype(k)::value;
        const int ne = newton_jac_extra_cols(KIND, a.N);
        const int nc = jac_smooth_cols(a, ne);
        const long slice = any ? jac_smooth_slice_doubles(a.N, a.N + 2 * ne) : jac_smooth_slice_doubles(a.N, nc);
        return launch_team(a.N, a.B, any, slice, a.scratch, true, s, [&](auto t, auto lds, auto go, int lds_per_team, long stride) {
            return go(newton_jac_dense_smooth_kernel<KIND, decltype(t)::value, decltype(lds)::value>, a, o, nc, lds_per_team, stride);
        });
    });
}

} // namespace dqq
