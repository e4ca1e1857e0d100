// polish_dense_path.hip -- dqq_polish_path_f64 on a general P (B,N,N): the polish path (path_core.h: polish_problem_path -- the
// chain of smoothed damped polishes over a schedule of (kappa_s, steps_s), bit for bit) in one launch, by team_dense.h's teams on
// polish_team.h's slice, with polish_dense_smooth.hip's step, launch geometry, persistence loop and scratch: PolishPathTeam (LDS,
// N <= 64) and PolishPathAny (a 256-thread workgroup per problem on the caller's scratch).
//
// What the one launch saves over the chain: P is loaded from global memory into the slice and the inputs are classified once, and
// the current point xc stays in the slice from stage to stage -- a stage's x_out is never written, the next stage's x never read.
// What stays the parents': inside a step P is still reloaded into the matrix after each elimination, and a stage opens by
// evaluating its own r at xc in its own kappa, as the call it stands for does.  A stage with kappa_s == 0 is polish_dense_ls.hip's
// step: team_eval, and M formed by the hard entry functions, so team_solve's zero-skip rule passes over its unit rows; a stage
// with kappa_s > 0 is polish_dense_smooth.hip's: team_eval_smooth and the dense M.  The branch is uniform over the launch.
// A failed elimination leaves the matrix eliminated; the next stage reloads P before it evaluates (`dirty`).
// The teams of a wave run their stages independently: the fences are wave-wide, never team-wide, and a team past the end of the
// batch idles through them, as in the parents.
#include "smooth_team.h"
#include "path_core.h"

namespace dqq {

// One problem by one team.  M: n x ld; vec: polish_vec_doubles(n).
template <int KIND, int T>
static DQQ_D void team_polish_path_problem(const PolishArgs& a, const PolishPathOpts& o, long prob, double* M, double* vec, int lane)
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
    const double reg = o.reg;
    const int S = o.n_stages;
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
    double first = 0.0, r = 0.0;
    int status0 = 1, steps_total = 0, halvings_total = 0;
    bool dirty = false;   // the matrix holds an abandoned elimination, not P
    for (int s = 0; s < S; ++s) {
        const double kappa = o.kappa[s];
        const bool hard = kappa == 0.0;
        const int budget = o.budget[s];
        if (dirty) {
            team_load_matrix<T>(M, ld, Pg, n, lane, ignore);
            team_sync<T>();
            dirty = false;
        }
        const double r0 = hard ? team_eval<KIND, T>(a, prob, n, M, ld, xc, z, F, dj, lane)
                               : team_eval_smooth<KIND, T>(a, prob, n, kappa, M, ld, xc, z, F, dj, lane);
        r = r0;
        int steps = 0, halvings = 0;
        const bool run = !bad && __builtin_isfinite(r0);
        while (run && steps < budget && r != 0.0) {
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
            } else if (hard) {
                for (idx_t<T> idx = lane; idx < (idx_t<T>)n * n; idx += T) {
                    const int i = (int)(idx / n), j = (int)(idx % n);
                    if (dj[i] == 0.0) M[i * ld + j] = i == j ? 1.0 : 0.0;
                    else if (i == j) M[i * ld + j] = polish_reg(M[i * ld + j], reg);
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
            if (!team_solve<T>(M, ld, d, z, n, lane)) { dirty = true; break; }
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
                // (the evaluation's fences stand between this trial's reads and the next one's writes)
                rn = hard ? team_eval<KIND, T>(a, prob, n, M, ld, xn, z, F, dj, lane)
                          : team_eval_smooth<KIND, T>(a, prob, n, kappa, M, ld, xn, z, F, dj, lane);
                accepted = rn < r;
            }
            if (!accepted) break;
            for (int i = lane; i < n; i += T) xc[i] = xn[i];
            r = rn;
            ++steps;
            halvings += k - 1;
            team_sync<T>();
        }
        team_sync<T>();   // every thread has left the stage: the matrix may be reloaded, z and F written again
        if (s == 0) { first = r0; status0 = polish_status(bad, r0, steps); }
        steps_total += steps;
        halvings_total += halvings;
        if (lane == 0) {
            if (o.stage_resid != nullptr) { o.stage_resid[2 * (prob * S + s)] = r0; o.stage_resid[2 * (prob * S + s) + 1] = r; }
            if (o.stage_steps != nullptr) o.stage_steps[prob * S + s] = steps;
        }
    }
    for (int i = lane; i < n; i += T) a.x_out[prob * n + i] = xc[i];
    if (lane == 0) {
        if (a.resid != nullptr) { a.resid[2 * prob] = first; a.resid[2 * prob + 1] = r; }
        if (a.steps != nullptr) a.steps[prob] = steps_total;
        if (a.status != nullptr) a.status[prob] = path_status(status0, steps_total);
        if (o.halvings != nullptr) o.halvings[prob] = halvings_total;
    }
    team_sync<T>();   // the slice is the next problem's
}

template <int KIND, int T, bool LDS>
__global__ __launch_bounds__(256) void polish_dense_path_kernel(const PolishArgs a, const PolishPathOpts o, int lds_per_team,
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
            team_polish_path_problem<KIND, T>(a, o, w, sw, sw + mat, tl);
    } else {
        double* scr = a.scratch + (long)blockIdx.x * scratch_stride;
        for (long w = blockIdx.x; w < a.B; w += gridDim.x) team_polish_path_problem<KIND, T>(a, o, w, scr, scr + mat, (int)threadIdx.x);
    }
}

hipError_t launch_polish_dense_path(int kind, const PolishArgs& a, const PolishPathOpts& o, bool any, hipStream_t s)
{
    return dispatch_kind(kind, [&](auto k) {
        return launch_team(a.N, a.B, any, polish_slice_doubles(a.N), a.scratch, true, s, [&](auto t, auto lds, auto go, int lds_per_team, long stride) {
            return go(polish_dense_path_kernel<decltype(k)::value, decltype(t)::value, decltype(lds)::value>, a, o, lds_per_team, stride);
        });
    });
}

} // namespace dqq
