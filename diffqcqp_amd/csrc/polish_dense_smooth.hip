// polish_dense_smooth.hip -- dqq_polish_smooth_f64 (kappa > 0) on a general P (B,N,N): the smoothed damped polish
// (smooth_core.h: polish_problem_smooth) by team_dense.h's teams on polish_team.h's slice, with polish_dense_ls.hip's step, launch
// geometry and scratch: the LDS teams (N <= 64) and a 256-thread workgroup per problem on the caller's scratch beyond.
//
// The slice is polish_dense_ls.hip's, double for double; dj holds the Jacobian of PI_k at the last evaluated point (box-like
// kinds: D_i; QCQP: three per contact).  What differs is team_eval_smooth (F_k, D) and that M is dense in every row: row i of a
// box-like kind is (delta_ij - delta_ij D_i) + D_i P'_ij, there are no unit rows for team_solve's zero-skip rule to pass over --
// the cost of smoothing on this route.  kappa == 0 never gets here: capi.hip sends it to polish_dense_ls.hip.
// team_eval_smooth is in smooth_team.h: polish_dense_path.hip evaluates with it too.
#include "smooth_team.h"

namespace dqq {

// One problem by one team.  M: n x ld; vec: polish_vec_doubles(n).
template <int KIND, int T>
static DQQ_D void team_polish_smooth_problem(const PolishArgs& a, const PolishSmoothOpts& o, long prob, double* M, double* vec, int lane)
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
    const double reg = o.reg, kappa = o.kappa;
    bool bad = false, ignore = false;
    team_load_matrix<T>(M, ld, Pg, n, lane, bad);
    for (int i = lane; i < n; i += T) {
        const double xi = a.x[prob * n + i];
        xc[i] = xi;
        bad = bad || !__builtin_isfinite(xi) || !__builtin_isfinite(a.q[prob * n + i]);
        if constexpr (KIND >= 2) bad = bad || !__builtin_isfinite(a.a[prob * n + i]) || !__builtin_isfinite(a.b[prob * n + i]);
        if constexpr (KIND == 3) bad = bad || !__builtin_isfinite(a.c[prob * n + i]);
    }
    if constexpr (KIND == 1)
        for (int k = lane; k < nc; k += T) bad = bad || !__builtin_isfinite(a.a[prob * nc + k]) || !__builtin_isfinite(a.b[prob * nc + k]);
    bad = team_any<T>(bad);
    team_sync<T>();
    const double r0 = team_eval_smooth<KIND, T>(a, prob, n, kappa, M, ld, xc, z, F, dj, lane);
    double r = r0;
    int steps = 0, halvings = 0;
    const bool run = !bad && __builtin_isfinite(r0);
    while (run && steps < a.max_steps && r != 0.0) {
        // M in place of P, and the right-hand side
        if constexpr (KIND == 1) {
            for (idx_t<T> idx = lane; idx < (idx_t<T>)nc * n; idx += T) {
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
            for (idx_t<T> idx = lane; idx < (idx_t<T>)n * n; idx += T) {
                const int i = (int)(idx / n), j = (int)(idx % n);
                const double pij = M[i * ld + j];
                M[i * ld + j] = smooth_box_entry(i == j, dj[i], i == j ? polish_reg(pij, reg) : pij);
            }
        }
        for (int i = lane; i < n; i += T) d[i] = -F[i];
        team_sync<T>();
        if (!team_solve<T>(M, ld, d, z, n, lane)) break;
        // the direction out of z, which every evaluation writes, and P back into the matrix: once for all trials of the step
        for (int i = lane; i < n; i += T) d[i] = z[i];
        team_load_matrix<T>(M, ld, Pg, n, lane, ignore);
        team_sync<T>();
        double t = 1.0, rn = r;
        int k = 0;
        bool accepted = false;
        for (; k <= o.max_halvings && !accepted; ++k, t = polish_half(t)) {
            if constexpr (KIND == 1) {
                for (int c = lane; c < nc; c += T) {
                    double ta = polish_trial(xc[2 * c], t, d[2 * c]), tb = polish_trial(xc[2 * c + 1], t, d[2 * c + 1]);
                    check_proj_circle(ta, tb, a.a[prob * nc + c] * a.b[prob * nc + c]);
                    xn[2 * c] = ta;
                    xn[2 * c + 1] = tb;
                }
            } else {
                for (int i = lane; i < n; i += T) {
                    double lo, hi;
                    polish_bounds<KIND>(KIND >= 2 ? a.a[prob * n + i] : 0.0, KIND >= 2 ? a.b[prob * n + i] : 0.0,
                                        KIND == 3 ? a.c[prob * n + i] : 0.0, lo, hi);
                    xn[i] = polish_proj<KIND>(polish_trial(xc[i], t, d[i]), lo, hi);
                }
            }
            team_sync<T>();
            rn = team_eval_smooth<KIND, T>(a, prob, n, kappa, M, ld, xn, z, F, dj, lane);   // (its fences stand between this trial's reads and the next one's writes)
            accepted = rn < r;
        }
        if (!accepted) break;
        for (int i = lane; i < n; i += T) xc[i] = xn[i];
        r = rn;
        ++steps;
        halvings += k - 1;
        team_sync<T>();
    }
    team_sync<T>();
    for (int i = lane; i < n; i += T) a.x_out[prob * n + i] = xc[i];
    if (lane == 0) {
        if (a.resid != nullptr) { a.resid[2 * prob] = r0; a.resid[2 * prob + 1] = r; }
        if (a.steps != nullptr) a.steps[prob] = steps;
        if (a.status != nullptr) a.status[prob] = polish_status(bad, r0, steps);
        if (o.halvings != nullptr) o.halvings[prob] = halvings;
    }
    team_sync<T>();   // the slice is the next problem's
}

template <int KIND, int T, bool LDS>
__global__ __launch_bounds__(256) void polish_dense_smooth_kernel(const PolishArgs a, const PolishSmoothOpts o, int lds_per_team,
                                                                  long scratch_stride)
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
            team_polish_smooth_problem<KIND, T>(a, o, w, sw, sw + mat, tl);
    } else {
        double* scr = a.scratch + (long)blockIdx.x * scratch_stride;
        for (long w = blockIdx.x; w < a.B; w += gridDim.x) team_polish_smooth_problem<KIND, T>(a, o, w, scr, scr + mat, (int)threadIdx.x);
    }
}

hipError_t launch_polish_dense_smooth(int kind, const PolishArgs& a, const PolishSmoothOpts& o, bool any, hipStream_t s)
{
    return dispatch_kind(kind, [&](auto k) {
        return launch_team(a.N, a.B, any, polish_slice_doubles(a.N), a.scratch, true, s, [&](auto t, auto lds, auto go, int lds_per_team, long stride) {
            return go(polish_dense_smooth_kernel<decltype(k)::value, decltype(t)::value, decltype(lds)::value>, a, o, lds_per_team, stride);
        });
    });
}

} // namespace dqq
