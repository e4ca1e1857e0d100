// polish_diag_path.hip -- dqq_polish_path_f64 with DQQ_P_DIAG: the polish path (path_core.h: polish_problem_path -- the chain of
// smoothed damped polishes over a schedule of (kappa_s, steps_s), bit for bit) in one launch on the compact diagonal (B,N).
// The tile, the inputs and the launch are diag_tile.h's; every piece of arithmetic is a function of polish_tile.h, the ones
// polish_diag_ls.hip (hard) and polish_diag_smooth.hip (smoothed) call.  This file holds the stage loop, the uniform branch
// between the two evaluators and direction blocks, the trial loop over them, and the per-stage stores.
//
// The inputs are loaded and classified once and x stays in registers from stage to stage.  The stage loop is the outer loop and
// its index, kappa_s and steps_s are kernel-uniform, so the branch between the two evaluators -- kappa_s == 0: PolishCell::eval's
// hard F and, where the block is formed, the hard Jacobian of the kept z; kappa_s > 0: eval_smooth's F_k and D kept
// next to z -- is uniform over the wave.  What diverges is per lane, as in the parents: a problem that has used its stage's
// budget, reached r == 0, failed or found no step idles, masked, through the rest of the stage's steps while its tile neighbours
// go on, and enters the next stage with them by evaluating its own r there; a problem whose inputs are bad, or a tile slot past
// the end of the batch, idles through every stage.  A stage ends for the wave when none of its problems is live (or at the
// budget).  Ballots and fences are wave-wide and are reached by every lane of the wave in every trip: no lane leaves a loop
// that its neighbours still run.  Nothing here waits for another wave.
#include "polish_tile.h"
#include "path_core.h"

namespace dqq {

template <int KIND, int N, int WPB>
__global__ __launch_bounds__(64 * WPB) void polish_diag_path_kernel(const PolishArgs a, const PolishPathOpts o)
{
#pragma clang fp contract(off)
    using Tile = DiagTile<N, WPB>;
    __shared__ __attribute__((aligned(16))) double s_rs[WPB][Tile::T * N];

    const Tile t(a.B);
    if (t.first >= a.B) return; // whole wave leaves; no workgroup barrier is used below
    double* rs = s_rs[t.wave] + t.pl * N;
    const int S = o.n_stages;
    const DiagInputs<KIND> in(t, a, false, 1.0, false);   // one-sided boxes are not admitted by this entry
    const bool bad = t.any(in.bad);
    const PolishCell<KIND> c(in, diag_pm(in.pv, o.reg));

    // hard: polish_tile.h's F, D left alone (the hard Jacobian is taken from z where the block is formed); else F_k and D
    auto eval = [&](bool hard, double kappa, double x0, double x1, double& z0, double& z1, double& F0, double& F1, double (&D)[3]) {
        if (hard) c.eval(x0, x1, z0, z1, F0, F1);
        else c.eval_smooth(kappa, x0, x1, z0, z1, F0, F1, D);
    };

    double x0 = in.xv.x, x1 = in.xv.y, z0 = 0.0, z1 = 0.0, F0 = 0.0, F1 = 0.0, D[3] = {0.0, 0.0, 0.0};
    double r_first = 0.0, r = 0.0;
    int status0 = 1, steps_total = 0, halvings_total = 0;
    for (int s = 0; s < S; ++s) {   // kernel-uniform
        const double kappa = o.kappa[s];
        const bool hard = kappa == 0.0;
        const int budget = o.budget[s];
        // the stage opens as the call it stands for does: its own r at the current point
        eval(hard, kappa, x0, x1, z0, z1, F0, F1, D);
        const double r0 = polish_tile_residual<N>(rs, t.j, F0, F1, t.valid);
        r = r0;
        int steps = 0, halvings = 0;
        bool live = t.valid && !bad && __builtin_isfinite(r0);
        for (int it = 0; it < budget; ++it) {
            live = live && r != 0.0;
            if (__all(!live)) break;
            // the direction of the lane's block, once per step
            double d0 = -F0, d1 = -F1;
            bool ok = true;
            if (live) ok = hard ? c.direction(z0, z1, d0, d1) : c.direction_smooth(D, d0, d1);
            const bool failed = t.any(live && !ok);   // a failed block fails the problem's step
            bool search = live && !failed;
            double tk = 1.0;
            for (int k = 0; k <= o.max_halvings; ++k, tk = polish_half(tk)) {
                if (__all(!search)) break;
                double xn0 = 0.0, xn1 = 0.0, zn0 = 0.0, zn1 = 0.0, Fn0 = 0.0, Fn1 = 0.0, Dn[3] = {0.0, 0.0, 0.0};
                if (search) {
                    xn0 = polish_trial(x0, tk, d0);
                    xn1 = polish_trial(x1, tk, d1);
                    c.project(xn0, xn1);
                    eval(hard, kappa, xn0, xn1, zn0, zn1, Fn0, Fn1, Dn);
                }
                const double rn = polish_tile_residual<N>(rs, t.j, Fn0, Fn1, search);
                if (search && rn < r) {   // accepted at this k: the problem idles through its neighbours' further trials
                    x0 = xn0; x1 = xn1; z0 = zn0; z1 = zn1; F0 = Fn0; F1 = Fn1;
                    D[0] = Dn[0]; D[1] = Dn[1]; D[2] = Dn[2];
                    r = rn;
                    ++steps;
                    halvings += k;
                    search = false;
                }
            }
            // a failed elimination, or no trial point accepted (`search` still set): the problem keeps x and stops this stage
            if (failed || search) live = false;
        }
        if (s == 0) { r_first = r0; status0 = polish_status(bad, r0, steps); }
        steps_total += steps;
        halvings_total += halvings;
        if (t.valid && t.j == 0) {
            const long e = (t.first + t.pl) * S + s;
            if (o.stage_resid != nullptr) { o.stage_resid[2 * e] = r0; o.stage_resid[2 * e + 1] = r; }
            if (o.stage_steps != nullptr) o.stage_steps[e] = steps;
        }
    }
    polish_tile_store(t, a, x0, x1, r_first, r, steps_total, [&] { return path_status(status0, steps_total); }, o.halvings,
                      halvings_total);
}

hipError_t launch_polish_diag_path(int kind, const PolishArgs& a, const PolishPathOpts& o, hipStream_t s)
{
    return launch_diag(kind, a.N, a.B, s,
                       [](auto k, auto n) { return polish_diag_path_kernel<decltype(k)::value, decltype(n)::value, kDiagWPB>; }, a, o);
}

} // namespace dqq
