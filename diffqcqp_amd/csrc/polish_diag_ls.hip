// polish_diag_ls.hip -- dqq_polish_ls_f64 with DQQ_P_DIAG: the damped polish (polish_core.h: polish_problem_ls) on the compact
// diagonal (B,N).  The tile and the inputs are diag_tile.h's, the step's pieces polish_tile.h's: a wave64 owns 128/N consecutive
// problems, lane = (problem, coordinate pair / contact), the lane's block of M solved in registers, the problem's r taken by
// every one of its lanes from the wave's LDS slice in index order, a failed block found by a ballot.
//
// What is new is the trial loop inside a Newton step.  The direction (d0, d1) is solved for once and stays in registers; trial
// k evaluates PI(x + 2^-k d).  The loop counter k and the step length t are wave-uniform: every problem of the tile that
// searches started its search at k = 0 in this very step, so the wave's k is the problem's k.  A problem that has accepted (or
// has stopped for good) idles, masked, while its tile neighbours go on halving; the loop ends when no problem of the wave
// searches any more or k passes max_halvings, and a problem still searching then has found no step and stops.  Nothing here
// waits for another wave.  The proximal weight is looked at at run time (polish_reg: reg = 0 adds nothing), so one instantiation
// per (KIND, N) serves dqq_polish_f64's and dqq_polish_reg_f64's arithmetic.
#include "polish_tile.h"

namespace dqq {

template <int KIND, int N, int WPB>
__global__ __launch_bounds__(64 * WPB) void polish_diag_ls_kernel(const PolishArgs a, const PolishLsOpts o)
{
#pragma clang fp contract(off)
    using Tile = DiagTile<N, WPB>;
    __shared__ __attribute__((aligned(16))) double s_rs[WPB][Tile::T * N];

    const Tile t(a.B);
    if (t.first >= a.B) return; // whole wave leaves; no workgroup barrier is used below
    double* rs = s_rs[t.wave] + t.pl * N;
    const DiagInputs<KIND> in(t, a, a.inf_bounds != 0, 1.0, false);
    const bool bad = t.any(in.bad);
    const PolishCell<KIND> c(in, diag_pm(in.pv, o.reg));

    double x0 = in.xv.x, x1 = in.xv.y, z0, z1, F0, F1;
    c.eval(x0, x1, z0, z1, F0, F1);
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
        if (live) ok = c.direction(z0, z1, d0, d1);
        const bool failed = t.any(live && !ok);   // a failed block fails the problem's step
        bool search = live && !failed;
        double tk = 1.0;
        for (int k = 0; k <= o.max_halvings; ++k, tk = polish_half(tk)) {
            if (__all(!search)) break;
            double xn0 = 0.0, xn1 = 0.0, zn0 = 0.0, zn1 = 0.0, Fn0 = 0.0, Fn1 = 0.0;
            if (search) {
                xn0 = polish_trial(x0, tk, d0);
                xn1 = polish_trial(x1, tk, d1);
                c.project(xn0, xn1);
                c.eval(xn0, xn1, zn0, zn1, Fn0, Fn1);
            }
            const double rn = polish_tile_residual<N>(rs, t.j, Fn0, Fn1, search);
            if (search && rn < r) {   // accepted at this k: the problem idles through its neighbours' further trials
                x0 = xn0; x1 = xn1; z0 = zn0; z1 = zn1; F0 = Fn0; F1 = Fn1;
                r = rn;
                ++steps;
                halvings += k;
                search = false;
            }
        }
        // a failed elimination, or no trial point accepted (`search` still set): the problem keeps x and stops
        if (failed || search) live = false;
    }
    polish_tile_store(t, a, x0, x1, r0, r, steps, [&] { return polish_status(bad, r0, steps); }, o.halvings,
                      halvings);
}

hipError_t launch_polish_diag_ls(int kind, const PolishArgs& a, const PolishLsOpts& o, hipStream_t s)
{
    return launch_diag(kind, a.N, a.B, s,
                       [](auto k, auto n) { return polish_diag_ls_kernel<decltype(k)::value, decltype(n)::value, kDiagWPB>; }, a, o);
}

} // namespace dqq
