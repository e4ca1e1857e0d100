// polish_diag_smooth.hip -- dqq_polish_smooth_f64 (kappa > 0) with DQQ_P_DIAG: the smoothed damped polish (smooth_core.h:
// polish_problem_smooth) on the compact diagonal (B,N).  The tile, the inputs and the launch are diag_tile.h's, the pieces of the step
// polish_tile.h's (eval_smooth, direction_smooth, project, polish_tile_residual, polish_tile_store); the trial loop is written
// as in polish_diag_ls.hip: a wave64 owns 128/N consecutive problems, lane = (problem, coordinate pair / contact), the problem's
// r_k taken by every one of its lanes from the wave's LDS slice in index order, a failed block found by a ballot.
//
// What differs is the evaluation of a point: F_k = x - PI_k(z) and the Jacobian D of PI_k (smooth_box / smooth_disc) instead
// of the hard ones; the block of M is still 1 x 1 or 2 x 2.  The Jacobian of the last evaluated point is kept in registers next
// to z and F (two doubles, three for a contact).  The trial point is PI(x + t d) with the hard projection.  kappa == 0 never gets
// here: capi.hip sends it to polish_diag_ls.hip.
#include "polish_tile.h"

namespace dqq {

template <int KIND, int N, int WPB>
__global__ __launch_bounds__(64 * WPB) void polish_diag_smooth_kernel(const PolishArgs a, const PolishSmoothOpts o)
{
#pragma clang fp contract(off)
    using Tile = DiagTile<N, WPB>;
    __shared__ __attribute__((aligned(16))) double s_rs[WPB][Tile::T * N];

    const Tile t(a.B);
    if (t.first >= a.B) return; // whole wave leaves; no workgroup barrier is used below
    double* rs = s_rs[t.wave] + t.pl * N;
    const double kappa = o.kappa;
    const DiagInputs<KIND> in(t, a, false, 1.0, false);   // one-sided boxes are not admitted under smoothing
    const bool bad = t.any(in.bad);
    const PolishCell<KIND> c(in, diag_pm(in.pv, o.reg));

    double x0 = in.xv.x, x1 = in.xv.y, z0, z1, F0, F1, D[3];
    c.eval_smooth(kappa, x0, x1, z0, z1, F0, F1, D);
    const double r0 = polish_tile_residual<N>(rs, t.j, F0, F1, t.valid);
    double r = r0;
    int steps = 0, halvings = 0;
    bool live = t.valid && !bad && __builtin_isfinite(r0);
    for (int it = 0; it < a.max_steps; ++it) {
        live = live && r != 0.0;
        if (__all(!live)) break;
        // the direction of the lane's block, once per step
        double d0 = -F0, d1 = -F1;
        bool ok = true;
        if (live) ok = c.direction_smooth(D, d0, d1);
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
                c.eval_smooth(kappa, xn0, xn1, zn0, zn1, Fn0, Fn1, Dn);
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
        // a failed elimination, or no trial point accepted (`search` still set): the problem keeps x and stops
        if (failed || search) live = false;
    }
    polish_tile_store(t, a, x0, x1, r0, r, steps, [&] { return polish_status(bad, r0, steps); }, o.halvings, halvings);
}

hipError_t launch_polish_diag_smooth(int kind, const PolishArgs& a, const PolishSmoothOpts& o, hipStream_t s)
{
    return launch_diag(kind, a.N, a.B, s,
                       [](auto k, auto n) { return polish_diag_smooth_kernel<decltype(k)::value, decltype(n)::value, kDiagWPB>; }, a, o);
}

} // namespace dqq
