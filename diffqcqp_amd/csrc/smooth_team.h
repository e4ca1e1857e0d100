// smooth_team.h -- the evaluation of a point by a team on the central path, shared by polish_dense_smooth.hip
// (dqq_polish_smooth_f64) and polish_dense_path.hip (dqq_polish_path_f64): polish_team.h's team_eval with PI_k, F_k and D of
// smooth_core.h in place of the hard ones.
#pragma once

#include "polish_team.h"
#include "smooth_core.h"

namespace dqq {

// z, F_k, the Jacobian and r_k at xv; M holds P.  Every thread returns r_k.
template <int KIND, int T>
static DQQ_D double team_eval_smooth(const PolishArgs& a, long prob, int n, double kappa, const double* M, idx_t<T> ld, const double* xv,
                                     double* z, double* F, double* dj, int lane)
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
            const SmoothDisc s = smooth_disc(z[2 * k], z[2 * k + 1], a.a[prob * nc + k] * a.b[prob * nc + k], kappa);
            F[2 * k] = smooth_F(xv[2 * k], s.pa);
            F[2 * k + 1] = smooth_F(xv[2 * k + 1], s.pb);
            dj[3 * k] = s.D[0]; dj[3 * k + 1] = s.D[1]; dj[3 * k + 2] = s.D[2];
        }
    } else {
        for (int i = lane; i < n; i += T) {
            double lo, hi;
            polish_bounds<KIND>(KIND >= 2 ? a.a[prob * n + i] : 0.0, KIND >= 2 ? a.b[prob * n + i] : 0.0,
                                KIND == 3 ? a.c[prob * n + i] : 0.0, lo, hi);
            const SmoothBox s = smooth_box<KIND>(z[i], lo, hi, kappa);
            F[i] = smooth_F(xv[i], s.pi);
            dj[i] = s.D;
        }
    }
    team_sync<T>();
    double r = 0.0;
    for (int i = 0; i < n; ++i) r = nmax(r, F[i]);
    return r;
}

} // namespace dqq
