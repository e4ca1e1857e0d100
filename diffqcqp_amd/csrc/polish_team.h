// polish_team.h -- what polish_dense.hip (dqq_polish_f64) and polish_dense_ls.hip (dqq_polish_ls_f64) share on top of
// team_dense.h: the slice and the evaluation of a point.
// The slice: the matrix (N x (N|1): P while x is evaluated, then M in place, reloaded from P after the solve), then x, x+, F,
// z (the solution d after the solve), the right-hand side and the Jacobian (2N) -- polish_vec_doubles.  Unit rows and exact
// zeros are skipped where polish_solve skips them.
#pragma once

#include "team_dense.h"

namespace dqq {

static DQQ_HD long polish_slice_doubles(int n) { return ((long)n * (n | 1) + polish_vec_doubles(n) + 1) & ~1L; }

// PolishAny's and PolishLsAny's slice of the caller's scratch (polish_scratch_bytes: polish_dense.hip)
static inline long polish_any_stride(int N) { return polish_slice_doubles(N); }

// z, F, the Jacobian and r at xv; M holds P.  Every thread returns r.
template <int KIND, int T>
static DQQ_D double team_eval(const PolishArgs& a, long prob, int n, const double* M, idx_t<T> ld, const double* xv, double* z,
                              double* F, double* dj, int lane)
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
            const double rad = a.a[prob * nc + k] * a.b[prob * nc + k];
            polish_F_contact(xv[2 * k], xv[2 * k + 1], z[2 * k], z[2 * k + 1], rad, F[2 * k], F[2 * k + 1]);
            double D[3];
            polish_disc_jacobian(z[2 * k], z[2 * k + 1], rad, D);
            dj[3 * k] = D[0]; dj[3 * k + 1] = D[1]; dj[3 * k + 2] = D[2];
        }
    } else {
        for (int i = lane; i < n; i += T) {
            double lo, hi;
            polish_bounds<KIND>(KIND >= 2 ? a.a[prob * n + i] : 0.0, KIND >= 2 ? a.b[prob * n + i] : 0.0,
                                KIND == 3 ? a.c[prob * n + i] : 0.0, lo, hi);
            F[i] = polish_F<KIND>(xv[i], z[i], lo, hi);
            dj[i] = polish_free(z[i], lo, hi) ? 1.0 : 0.0;
        }
    }
    team_sync<T>();
    double r = 0.0;
    for (int i = 0; i < n; ++i) r = nmax(r, F[i]);
    return r;
}

} // namespace dqq
