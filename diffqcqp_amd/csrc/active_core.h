// active_core.h -- the arithmetic of dqq_newton_active_f64, host/device and without a lane notion: per problem, the active set
// the Newton family (dqq_polish_f64, dqq_newton_bwd_f64 / _jvp_f64, dqq_newton_jac_f64) works on at x, the multipliers of the
// active elements, and how far z may move before that active set changes.  It sits on polish_core.h / newton_core.h and calls
// their element functions: "state says free" means exactly "the Newton kernels used D_ii = 1".  active_diag.hip and
// active_dense.hip run these functions with their own thread mappings; active_problem below runs them on one thread
// (tests/hostcore/active_core_check.cpp) and is what the kernels must reproduce bit for bit.  tests/active_reference.py is the
// same definition in numpy.  No fused multiply-add is formed but the one of the contact's squared norm.
//
// Per problem, float64, at the x given.  An element is a coordinate (QP, box, signed box) or a contact (QCQP).
//   z      polish_core.h's: the row sum from 0 in index order by polish_acc (DQQ_P_DIAG: 0 + p_i x_i), then polish_z(x, s, q);
//          bounds (lo, hi) from polish_bounds<KIND> (the signed box: sbox_bounds.h's effective bounds).
//   state  box-like element: newton_box_state<KIND>(z_i, a_i, b_i, c_i): 0 free, 1 on the caller's lower bound, 2 on the
//          caller's upper bound, 3 on a constant (the QP's 0, the sign constraint's 0).  Contact, rad = l_n mu,
//          n2 = fma(z_b, z_b, z_a z_a): 0 inside the disc (polish_disc_jacobian's not (n2 > rad |rad|): D = I_2); 1 outside with
//          rad > 0 (newton_disc_u is on); 3 outside with rad <= 0 (D = 0).
//   mult   the multiplier of the element in the normal-cone sense, one rounded operation: box-like +0.0 where free, lo - z where
//          z <= lo (tested first, as newton_box_state does), z - hi where z >= hi; contact +0.0 inside, outside nrm - rad if
//          rad > 0, else nrm, with nrm = sqrt(n2).  At a solution z = x - g, so this is |g_i| on an active coordinate and
//          ||g_c|| on a sliding contact.  The reference's contact dual belongs to the squared form of the constraint,
//          |x_c|^2 <= rad^2, whose gradient is 2 x_c with |x_c| = rad:  gamma = mult / (2 rad).
//   margin, where   how far z can move, in the max norm per element, before `state` changes: box-like element
//          e_i = min(|z - lo|, |z - hi|), written t_hi < t_lo ? t_hi : t_lo (an infinite side gives +inf); contact
//          e_c = rad > 0 ? |nrm - rad| : nrm.  margin is the first smallest e in index order (a scan with strict < from element
//          0), where its index -- a coordinate, or a contact.  A fully unbounded box: +inf and 0.
//   status 2 if polish_inputs_bad holds (P, q, the extras, x; inf_ok: DQQ_F_INFINITE_BOUNDS of the box kinds) or a z_i is not
//          finite; else 0.  There is no status 1: nothing is eliminated.  With 2 the problem's state and where are -1, its mult
//          and margin NaN; no other problem's rows are touched.
//
// What margin is for.  Let Jq be dqq_newton_jac_f64's dx/dq at x, dx = Jq dq and dz = dx - P dx - dq.  For the box-like kinds
// the solution map is piecewise linear and PI acts coordinate by coordinate, so max_i |dz_i| < margin implies that x + dx
// solves the problem at q + dq with the same `state`, exactly (to rounding).  For the QCQP the disc's boundary is curved: the
// same holds to first order in dq only, and |dz| of a contact is to be read as the larger of its two components.
#pragma once

#include "newton_core.h"

namespace dqq {

constexpr int kActiveInside = 0, kActiveSliding = 1, kActiveZeroDisc = 3;

// (value, index) of the margin scan.  active_min: the first smallest in index order whatever the order of the comparisons --
// b takes a's place iff it is smaller, or equal at a lower index -- so a reduction of any shape gives the scan's answer.
struct ActiveMin {
    double v;
    int i;
};
DQQ_HD ActiveMin active_min(ActiveMin a, ActiveMin b) { return (b.v < a.v || (b.v == a.v && b.i < a.i)) ? b : a; }

// box-like element on its effective interval
DQQ_HD double active_box_mult(double z, double lo, double hi)
{
#pragma clang fp contract(off)
    if (polish_free(z, lo, hi)) return 0.0;
    if (z <= lo) return lo - z;
    if (z >= hi) return z - hi;
    return 0.0;
}
DQQ_HD double active_box_margin(double z, double lo, double hi)
{
#pragma clang fp contract(off)
    const double t_lo = fabs(z - lo), t_hi = fabs(z - hi);
    return t_hi < t_lo ? t_hi : t_lo;
}
template <int KIND>
DQQ_HD void active_box(double z, double a, double b, double c, int& state, double& mult, double& e)
{
    double lo, hi;
    polish_bounds<KIND>(a, b, c, lo, hi);
    state = newton_box_state<KIND>(z, a, b, c);
    mult = active_box_mult(z, lo, hi);
    e = active_box_margin(z, lo, hi);
}

// a contact: polish_disc_jacobian's n2 and test, newton_disc_u's rad > 0
DQQ_HD void active_contact(double za, double zb, double rad, int& state, double& mult, double& e)
{
#pragma clang fp contract(off)
    const double n2 = __builtin_fma(zb, zb, za * za);
    const double nrm = sqrt(n2);
    const bool outside = n2 > rad * fabs(rad), pos = rad > 0.0;
    state = !outside ? kActiveInside : (pos ? kActiveSliding : kActiveZeroDisc);
    mult = !outside ? 0.0 : (pos ? nrm - rad : nrm);
    e = pos ? fabs(nrm - rad) : nrm;
}

DQQ_HD int active_elements(int kind, int n) { return kind == 1 ? n / 2 : n; }

// ---- one problem on one thread -----------------------------------------------------------------------------------------
// P: (n,n), or the n diagonal entries with diag.  state, mult: active_elements(KIND, n) entries; margin, where: one.  Each
// output may be NULL.  z: n doubles of work.  inf_ok: the flag.  -> status
template <int KIND>
DQQ_HD int active_problem(const double* P, bool diag, const double* q, const double* a, const double* b, const double* c,
                          const double* x, int n, int* state, double* mult, double* margin, int* where, double* z,
                          bool inf_ok = false)
{
#pragma clang fp contract(off)
    const int ne = active_elements(KIND, n);
    bool bad = polish_inputs_bad<KIND>(P, diag, q, a, b, c, x, n, inf_ok);
    for (int i = 0; i < n; ++i) {
        double s = 0.0;
        if (diag) s = polish_acc(s, P[i], x[i]);
        else for (int j = 0; j < n; ++j) s = polish_acc(s, P[(long)i * n + j], x[j]);
        z[i] = polish_z(x[i], s, q[i]);
        bad |= !__builtin_isfinite(z[i]);
    }
    if (bad) {
        for (int k = 0; k < ne; ++k) {
            if (state != nullptr) state[k] = -1;
            if (mult != nullptr) mult[k] = newton_nan();
        }
        if (margin != nullptr) *margin = newton_nan();
        if (where != nullptr) *where = -1;
        return 2;
    }
    double best = 0.0;
    int at = 0;
    for (int k = 0; k < ne; ++k) {
        int st;
        double m, e;
        if (KIND == 1) active_contact(z[2 * k], z[2 * k + 1], a[k] * b[k], st, m, e);
        else active_box<KIND>(z[k], KIND >= 2 ? a[k] : 0.0, KIND >= 2 ? b[k] : 0.0, KIND == 3 ? c[k] : 0.0, st, m, e);
        if (state != nullptr) state[k] = st;
        if (mult != nullptr) mult[k] = m;
        if (k == 0 || e < best) { best = e; at = k; }
    }
    if (margin != nullptr) *margin = best;
    if (where != nullptr) *where = at;
    return 0;
}

} // namespace dqq
