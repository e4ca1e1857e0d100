// polish_tile.h -- the polish step on the diagonal tile, stated once for polish_diag.hip, polish_diag_ls.hip,
// polish_diag_smooth.hip and polish_diag_path.hip, as polish_team.h / smooth_team.h state it for the dense units.  With P diagonal
// the Newton matrix M of polish_core.h is diagonal (QP, box kinds) or 2 x 2 per contact (QCQP): a lane evaluates its two
// coordinates (PolishCell::eval / eval_smooth), solves its own block in registers with polish_solve1 / polish_solve2
// (direction / direction_smooth) -- the general elimination's pivot rule and operations on that block, so a diagonal P handed to
// the dense units as (B,N,N) gives the same bits -- and projects its trial point (project).  What the lanes of a problem share
// is the residual r (polish_tile_residual: the |F| of a problem go through the wave's LDS slice and every lane takes their
// maximum in index order) and whether a block's pivot failed (DiagTile::any).  The kernels keep their loops: no search, the
// halving loop, the stage loop around it.
#pragma once

#include "diag_tile.h"
#include "smooth_core.h"

namespace dqq {

// The lane's block of a problem: what the evaluation and the direction read.
template <int KIND>
struct PolishCell {
    double2 pv, qv;
    double pm0, pm1;                         // the diagonal of P' for the block of M; z and F read pv
    double lo0, hi0, lo1, hi1, rad;          // the box-like kinds' effective intervals; a contact's radius

    DQQ_D PolishCell(const DiagInputs<KIND>& in, double2 pm)
    {
        pv = in.pv;
        qv = in.qv;
        pm0 = pm.x;
        pm1 = pm.y;
        lo0 = 0.0; hi0 = 0.0; lo1 = 0.0; hi1 = 0.0; rad = 0.0;
        if constexpr (KIND == 1) {
            rad = in.ln * in.mc;
        } else {
            polish_bounds<KIND>(in.av.x, in.bv.x, in.cv.x, lo0, hi0);
            polish_bounds<KIND>(in.av.y, in.bv.y, in.cv.y, lo1, hi1);
        }
    }

    // z and F of the lane's two coordinates at (x0, x1)
    DQQ_D void eval(double x0, double x1, double& z0, double& z1, double& F0, double& F1) const
    {
        z0 = polish_z(x0, polish_acc(0.0, pv.x, x0), qv.x);
        z1 = polish_z(x1, polish_acc(0.0, pv.y, x1), qv.y);
        if constexpr (KIND == 1) {
            polish_F_contact(x0, x1, z0, z1, rad, F0, F1);
        } else {
            F0 = polish_F<KIND>(x0, z0, lo0, hi0);
            F1 = polish_F<KIND>(x1, z1, lo1, hi1);
        }
    }
    // z, F_k and the Jacobian of PI_k (box-like: D of the two coordinates in D[0], D[1]; a contact: d00, d01, d11) at (x0, x1)
    DQQ_D void eval_smooth(double kappa, double x0, double x1, double& z0, double& z1, double& F0, double& F1, double (&D)[3]) const
    {
        z0 = polish_z(x0, polish_acc(0.0, pv.x, x0), qv.x);
        z1 = polish_z(x1, polish_acc(0.0, pv.y, x1), qv.y);
        if constexpr (KIND == 1) {
            const SmoothDisc s = smooth_disc(z0, z1, rad, kappa);
            F0 = smooth_F(x0, s.pa);
            F1 = smooth_F(x1, s.pb);
            D[0] = s.D[0]; D[1] = s.D[1]; D[2] = s.D[2];
        } else {
            const SmoothBox s0 = smooth_box<KIND>(z0, lo0, hi0, kappa), s1 = smooth_box<KIND>(z1, lo1, hi1, kappa);
            F0 = smooth_F(x0, s0.pi);
            F1 = smooth_F(x1, s1.pi);
            D[0] = s0.D; D[1] = s1.D; D[2] = 0.0;
        }
    }
    // The direction of the lane's block from (d0, d1) = -F: the hard Jacobian is taken from z.  false: a pivot failed.
    DQQ_D bool direction(double z0, double z1, double& d0, double& d1) const
    {
        if constexpr (KIND == 1) {
            double D[3];
            polish_disc_jacobian(z0, z1, rad, D);
            return polish_solve2(polish_contact_entry(true, D[0], D[0], D[1], pm0, 0.0),
                                 polish_contact_entry(false, D[1], D[0], D[1], 0.0, pm1),
                                 polish_contact_entry(false, D[1], D[1], D[2], pm0, 0.0),
                                 polish_contact_entry(true, D[2], D[1], D[2], 0.0, pm1), d0, d1);
        } else {
            bool ok = polish_solve1(polish_free(z0, lo0, hi0) ? pm0 : 1.0, d0);
            ok = polish_solve1(polish_free(z1, lo1, hi1) ? pm1 : 1.0, d1) && ok;
            return ok;
        }
    }
    // The same from the Jacobian D of PI_k that eval_smooth left.
    DQQ_D bool direction_smooth(const double (&D)[3], double& d0, double& d1) const
    {
        if constexpr (KIND == 1) {
            double m[4];
            newton_contact_block(D, pm0, pm1, m);
            return polish_solve2(m[0], m[1], m[2], m[3], d0, d1);
        } else {
            bool ok = polish_solve1(smooth_box_entry(true, D[0], pm0), d0);
            ok = polish_solve1(smooth_box_entry(true, D[1], pm1), d1) && ok;
            return ok;
        }
    }
    // the hard projection of a trial point
    DQQ_D void project(double& x0, double& x1) const
    {
        if constexpr (KIND == 1) {
            check_proj_circle(x0, x1, rad);
        } else {
            x0 = polish_proj<KIND>(x0, lo0, hi0);
            x1 = polish_proj<KIND>(x1, lo1, hi1);
        }
    }
};

// The problem's r: every lane of the problem for which `on`, from the problem's LDS slice rs (N doubles) in index order.
// Every lane of the wave comes here: the fences are wave-wide.
template <int N>
static DQQ_D double polish_tile_residual(double* rs, int j, double F0, double F1, bool on)
{
    if (on) { rs[2 * j] = F0; rs[2 * j + 1] = F1; }
    wave_lds_fence();
    double r = 0.0;
    if (on)
        for (int i = 0; i < N; ++i) r = nmax(r, rs[i]);
    wave_lds_fence();
    return r;
}

// What a polish writes per problem: x_out by every lane, the rest by the problem's first lane.  halvings_out: the damped
// entries' optional output, NULL where the entry has none.  status() is the problem's status word; only the lane that stores
// it forms it (formed by every lane ahead of the call it costs the kernels registers).
template <typename Tile, typename Status>
static DQQ_D void polish_tile_store(const Tile& t, const PolishArgs& a, double x0, double x1, double r0, double r, int steps,
                                    Status&& status, int* halvings_out, int halvings)
{
    if (t.valid) {
        *reinterpret_cast<double2*>(a.x_out + t.co) = make_double2(x0, x1);
        if (t.j == 0) {
            const long b = t.first + t.pl;
            if (a.resid != nullptr) { a.resid[2 * b] = r0; a.resid[2 * b + 1] = r; }
            if (a.steps != nullptr) a.steps[b] = steps;
            if (a.status != nullptr) a.status[b] = status();
            if (halvings_out != nullptr) halvings_out[b] = halvings;
        }
    }
}

} // namespace dqq
