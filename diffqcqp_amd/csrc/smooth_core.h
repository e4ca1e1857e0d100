// smooth_core.h -- the Newton family on the central path (dqq_polish_smooth_f64, dqq_newton_bwd_smooth_f64,
// dqq_newton_jvp_smooth_f64; dqq_newton_jac_smooth_f64: DESIGN 4.21, newton_jac_*_smooth.hip), host/device and
// without a lane notion, on top of polish_core.h and newton_core.h.
// The hard projection PI of F(x) = x - PI(x - (P x + q)) is replaced by the Chen-Harker-Kanzow-Smale smoothing PI_k with one
// scalar kappa >= 0 per call; D and E below are its derivatives, and everything else -- g, z, r, M = (I - D) + D P', the
// elimination, the status words, the damped step rule, both derivative modes -- is polish_core.h's and newton_core.h's with PI_k,
// D, E in place of the hard ones.  polish_diag_smooth.hip, polish_dense_smooth.hip, newton_diag_smooth.hip and
// newton_dense_smooth.hip run these functions with their own thread mappings; the *_problem functions below run them on one
// thread (tests/hostcore/smooth_core_check.cpp) and are what the kernels must reproduce bit for bit.  tests/smooth_reference.py
// is the same definition in numpy.  No fused multiply-add is formed but the squared norm of a contact's z.
//
//   s(t)  = sqrt(t t + 4 (kappa kappa))
//   p(t)  = (s + t) / 2               for t >= 0,   (2 (kappa kappa)) / (s - t)         otherwise      -- smooth max(t, 0)
//   p'(t) = (1 + t / s) / 2           for t >= 0,   (2 (kappa kappa)) / (s (s - t))     otherwise      -- in (0, 1)
// every product, sum, quotient and root rounded on its own, in the order written (the products by 2 and 4 are exact).
//
// Box-like coordinate on [lo, hi] (polish_bounds; the signed box on sbox_bounds.h's effective bounds):
//   PI_k = (lo + p(z - lo)) - p(z - hi),   D = p'(z - lo) - p'(z - hi),   E_lo = 1 - p'(z - lo),   E_hi = p'(z - hi)
//   QP ([0, +inf): the lower term alone): PI_k = p(z), D = p'(z), no E.  Signed box: E_lo / E_hi reach l_min / l_max only where
//   keep_lo / keep_hi hold, as in the hard case; v takes nothing.
//   M_ij = ((i == j) - (i == j ? D_i : 0)) + D_i P'_ij        (smooth_box_entry; DQQ_P_DIAG: the 1 x 1 block)
//   JVP:  rhs_i = (E_lo dlo_i + E_hi dhi_i) - D_i t_i;   backward:  v_i = D_i w_i, grad_lo_i = E_lo w_i, grad_hi_i = E_hi w_i
// QCQP contact, rad = l_n mu, n2 = fma(z_b, z_b, z_a z_a), t = sqrt(n2).  rad > 0: u = t - rad, m = rad + p(u), sc = rad / m,
//   PI_k = z sc,   c = (rad p'(u)) / ((m m) t) (0 at t == 0),   D = [[sc - (c z_a) z_a, 0 - (c z_a) z_b], [., sc - (c z_b) z_b]],
//   e = (p(u) + rad p'(u)) / (m m),   E_rad = z e,   d rad = mu dl_n + l_n dmu.   Otherwise PI_k = 0, D = 0, E = 0.
//   M rows, the right-hand side, v and the radius' gradients: polish_contact_entry, newton_contact_rhs (u := E_rad, on := rad > 0),
//   newton_contact_v, newton_contact_t.
// The smoothed polish: polish_problem_ls with F_k = x - PI_k(z), r_k = max |F_k| and the smoothed M; a trial point stays
// PI(x + t_k d) with the HARD projection, so every x_out is a projected point; acceptance is r_k lower than before.
// kappa == 0 is looked at at run time and takes polish_core.h's / newton_core.h's functions: the parents' bits (the formulas above
// at kappa = 0 are not the hard ones bit for bit; the branch is).  kappa so small that kappa kappa underflows is not meant.
// One-sided boxes are not admitted: an infinite bound is status 2 (DQQ_F_INFINITE_BOUNDS is an unknown bit to these entries).
// A diagonal P given as (n,n): M_ij = D_i 0 (a contact row: D_r0 0 + D_r1 0) is an exact zero wherever P_ij is, so
// polish_solve's zero-skip rule solves block by block and the bits are DQQ_P_DIAG's, although no row of M is a unit row now.
#pragma once

#include "newton_core.h"

namespace dqq {

DQQ_HD double smooth_s(double t, double kappa)
{
#pragma clang fp contract(off)
    const double tt = t * t;
    const double k4 = 4.0 * (kappa * kappa);
    return sqrt(tt + k4);
}
DQQ_HD double smooth_p(double t, double kappa)
{
#pragma clang fp contract(off)
    const double s = smooth_s(t, kappa);
    if (t >= 0.0) return (s + t) / 2.0;
    return (2.0 * (kappa * kappa)) / (s - t);
}
DQQ_HD double smooth_dp(double t, double kappa)
{
#pragma clang fp contract(off)
    const double s = smooth_s(t, kappa);
    if (t >= 0.0) return (1.0 + t / s) / 2.0;
    return (2.0 * (kappa * kappa)) / (s * (s - t));
}

// a box-like coordinate at z: PI_k, D, and E towards the interval's two ends (zeros for the QP)
struct SmoothBox {
    double pi, D, elo, ehi;
};
template <int KIND>
DQQ_HD SmoothBox smooth_box(double z, double lo, double hi, double kappa)
{
#pragma clang fp contract(off)
    SmoothBox b;
    if (KIND == 0) {
        b.pi = smooth_p(z, kappa);
        b.D = smooth_dp(z, kappa);
        b.elo = b.ehi = 0.0;
        return b;
    }
    const double tl = z - lo, th = z - hi;
    const double dl = smooth_dp(tl, kappa), dh = smooth_dp(th, kappa);
    b.pi = (lo + smooth_p(tl, kappa)) - smooth_p(th, kappa);
    b.D = dl - dh;
    b.elo = 1.0 - dl;
    b.ehi = dh;
    return b;
}
// ... from the kind's extras: the interval, and E masked to the caller's own bounds (keep_lo / keep_hi)
template <int KIND>
DQQ_HD SmoothBox smooth_box_at(double z, double a, double b, double c, double kappa)
{
    double lo, hi;
    bool keep_lo = KIND == 2, keep_hi = KIND == 2;
    if (KIND == 3) {
        const SBoxBounds e = sbox_bounds(a, b, c);
        lo = e.lo; hi = e.hi; keep_lo = e.keep_lo; keep_hi = e.keep_hi;
    } else {
        polish_bounds<KIND>(a, b, c, lo, hi);
    }
    SmoothBox s = smooth_box<KIND>(z, lo, hi, kappa);
    if (!keep_lo) s.elo = 0.0;
    if (!keep_hi) s.ehi = 0.0;
    return s;
}
DQQ_HD double smooth_box_entry(bool on_diag, double D, double p)
{
#pragma clang fp contract(off)
    return ((on_diag ? 1.0 : 0.0) - (on_diag ? D : 0.0)) + D * p;
}
DQQ_HD double smooth_box_rhs(double D, double t, double elo, double dlo, double ehi, double dhi)
{
#pragma clang fp contract(off)
    return (elo * dlo + ehi * dhi) - D * t;
}
DQQ_HD double smooth_F(double x, double pi)
{
#pragma clang fp contract(off)
    return x - pi;
}

// a contact at z: PI_k (pa, pb), D as (d00, d01, d11), E_rad (ea, eb); on: rad > 0
struct SmoothDisc {
    double pa, pb, D[3], ea, eb;
    bool on;
};
DQQ_HD SmoothDisc smooth_disc(double za, double zb, double rad, double kappa)
{
#pragma clang fp contract(off)
    SmoothDisc d;
    d.on = rad > 0.0;
    if (!d.on) {
        d.pa = d.pb = d.D[0] = d.D[1] = d.D[2] = d.ea = d.eb = 0.0;
        return d;
    }
    const double n2 = __builtin_fma(zb, zb, za * za);
    const double t = sqrt(n2), u = t - rad;
    const double pu = smooth_p(u, kappa), dpu = smooth_dp(u, kappa);
    const double m = rad + pu, sc = rad / m, mm = m * m;
    d.pa = za * sc;
    d.pb = zb * sc;
    const double c = t == 0.0 ? 0.0 : (rad * dpu) / (mm * t);
    const double ca = c * za, cb = c * zb;
    d.D[0] = sc - ca * za;
    d.D[1] = 0.0 - ca * zb;
    d.D[2] = sc - cb * zb;
    const double e = (pu + rad * dpu) / mm;
    d.ea = za * e;
    d.eb = zb * e;
    return d;
}

// ---- one problem on one thread -----------------------------------------------------------------------------------------
// z, F_k, the Jacobian dj (box-like: D_i, n of them; QCQP: 3 per contact) and r_k at xv.  diag: P is the n diagonal entries.
template <int KIND>
DQQ_HD double smooth_eval(const double* P, bool diag, const double* q, const double* a, const double* b, const double* c,
                          const double* xv, int n, double kappa, double* z, double* F, double* dj)
{
    for (int i = 0; i < n; ++i) {
        double s = 0.0;
        if (diag) s = polish_acc(s, P[i], xv[i]);
        else for (int j = 0; j < n; ++j) s = polish_acc(s, P[(long)i * n + j], xv[j]);
        z[i] = polish_z(xv[i], s, q[i]);
    }
    if (KIND == 1) {
        for (int k = 0; k < n / 2; ++k) {
            const SmoothDisc d = smooth_disc(z[2 * k], z[2 * k + 1], a[k] * b[k], kappa);
            F[2 * k] = smooth_F(xv[2 * k], d.pa);
            F[2 * k + 1] = smooth_F(xv[2 * k + 1], d.pb);
            dj[3 * k] = d.D[0]; dj[3 * k + 1] = d.D[1]; dj[3 * k + 2] = d.D[2];
        }
    } else {
        for (int i = 0; i < n; ++i) {
            const SmoothBox s = smooth_box_at<KIND>(z[i], KIND >= 2 ? a[i] : 0.0, KIND >= 2 ? b[i] : 0.0, KIND == 3 ? c[i] : 0.0, kappa);
            F[i] = smooth_F(xv[i], s.pi);
            dj[i] = s.D;
        }
    }
    double r = 0.0;
    for (int i = 0; i < n; ++i) r = nmax(r, F[i]);
    return r;
}

// M (transposed: M') into the n x n buffer from P and the Jacobian dj of smooth_eval
template <int KIND>
DQQ_HD void smooth_matrix(const double* P, const double* dj, int n, bool transposed, double* M, double reg)
{
    if (KIND == 1) { newton_matrix<1>(P, dj, n, transposed, M, reg); return; }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const double pij = P[(long)i * n + j];
            M[transposed ? (long)j * n + i : (long)i * n + j] = smooth_box_entry(i == j, dj[i], i == j ? polish_reg(pij, reg) : pij);
        }
}

// The smoothed damped polish of one problem (dqq_polish_smooth_f64): polish_problem_ls's arguments and kappa.  -> status
template <int KIND>
DQQ_HD int polish_problem_smooth(const double* P, bool diag, const double* q, const double* a, const double* b, const double* c,
                                 const double* x, double* x_out, int n, int max_steps, int max_halvings, double* resid,
                                 int* steps_out, int* halvings_out, double* work, double reg, double kappa)
{
#pragma clang fp contract(off)
    if (kappa == 0.0)
        return polish_problem_ls<KIND>(P, diag, q, a, b, c, x, x_out, n, max_steps, max_halvings, resid, steps_out, halvings_out, work,
                                       false, reg);
    double* M = work;
    double* xc = M + (long)n * n;
    double* xn = xc + n;
    double* F = xn + n;
    double* z = F + n;
    double* d = z + n;
    double* dj = d + n;
    const bool bad = polish_inputs_bad<KIND>(P, diag, q, a, b, c, x, n, false);
    for (int i = 0; i < n; ++i) xc[i] = x[i];
    const double r0 = smooth_eval<KIND>(P, diag, q, a, b, c, xc, n, kappa, z, F, dj);
    double r = r0;
    int steps = 0, halvings = 0;
    const bool run = !bad && __builtin_isfinite(r0);
    while (run && steps < max_steps && r != 0.0) {
        bool ok = true;
        if (diag) {
            if (KIND == 1) {
                for (int k = 0; k < n / 2 && ok; ++k) {
                    double m[4];
                    newton_contact_block(dj + 3 * k, polish_reg(P[2 * k], reg), polish_reg(P[2 * k + 1], reg), m);
                    d[2 * k] = -F[2 * k];
                    d[2 * k + 1] = -F[2 * k + 1];
                    ok = polish_solve2(m[0], m[1], m[2], m[3], d[2 * k], d[2 * k + 1]);
                }
            } else {
                for (int i = 0; i < n && ok; ++i) {
                    d[i] = -F[i];
                    ok = polish_solve1(smooth_box_entry(true, dj[i], polish_reg(P[i], reg)), d[i]);
                }
            }
        } else {
            for (int i = 0; i < n; ++i) d[i] = -F[i];
            smooth_matrix<KIND>(P, dj, n, false, M, reg);
            ok = polish_solve(M, n, d, n);
        }
        if (!ok) break;
        double t = 1.0, rn = r;
        int k = 0;
        bool accepted = false;
        for (; k <= max_halvings && !accepted; ++k, t = polish_half(t)) {
            if (KIND == 1) {
                for (int c2 = 0; c2 < n / 2; ++c2) {
                    double ta = polish_trial(xc[2 * c2], t, d[2 * c2]), tb = polish_trial(xc[2 * c2 + 1], t, d[2 * c2 + 1]);
                    check_proj_circle(ta, tb, a[c2] * b[c2]);
                    xn[2 * c2] = ta;
                    xn[2 * c2 + 1] = tb;
                }
            } else {
                for (int i = 0; i < n; ++i) {
                    double lo, hi;
                    polish_bounds<KIND>(KIND >= 2 ? a[i] : 0.0, KIND >= 2 ? b[i] : 0.0, KIND == 3 ? c[i] : 0.0, lo, hi);
                    xn[i] = polish_proj<KIND>(polish_trial(xc[i], t, d[i]), lo, hi);
                }
            }
            rn = smooth_eval<KIND>(P, diag, q, a, b, c, xn, n, kappa, z, F, dj);
            accepted = rn < r;
        }
        if (!accepted) break;
        for (int i = 0; i < n; ++i) xc[i] = xn[i];
        r = rn;
        ++steps;
        halvings += k - 1;
    }
    for (int i = 0; i < n; ++i) x_out[i] = xc[i];
    if (resid != nullptr) { resid[0] = r0; resid[1] = r; }
    if (steps_out != nullptr) *steps_out = steps;
    if (halvings_out != nullptr) *halvings_out = halvings;
    return polish_status(bad, r0, steps);
}

// The smoothed forward-mode derivative of one problem (dqq_newton_jvp_smooth_f64): newton_jvp_problem's arguments and kappa
template <int KIND>
DQQ_HD int newton_jvp_problem_smooth(const double* P, bool diag, const double* q, const double* a, const double* b, const double* c,
                                     const double* x, const double* dP, const double* dq, const double* da, const double* db,
                                     double* dx, int n, double* work, double reg, double kappa)
{
#pragma clang fp contract(off)
    if (kappa == 0.0) return newton_jvp_problem<KIND>(P, diag, q, a, b, c, x, dP, dq, da, db, dx, n, work, false, reg);
    double* M = work;
    double* z = M + (long)n * n;
    double* F = z + n;
    double* dj = F + n;
    double* d = dj + 2 * n;
    const int ne = KIND == 0 ? 0 : (KIND == 1 ? n / 2 : n);
    bool bad = polish_inputs_bad<KIND>(P, diag, q, a, b, c, x, n, false);
    bad |= newton_vec_bad(dP, diag ? n : (long)n * n) || newton_vec_bad(dq, n) || newton_vec_bad(da, ne) || newton_vec_bad(db, ne);
    bool ok = !bad;
    if (ok) {
        smooth_eval<KIND>(P, diag, q, a, b, c, x, n, kappa, z, F, dj);
        for (int i = 0; i < n; ++i) {   // t into F
            double s = 0.0;
            if (dP != nullptr) {
                if (diag) s = polish_acc(s, dP[i], x[i]);
                else for (int j = 0; j < n; ++j) s = polish_acc(s, dP[(long)i * n + j], x[j]);
            }
            F[i] = newton_t(s, dq != nullptr ? dq[i] : 0.0);
        }
        if (KIND == 1) {
            for (int k = 0; k < n / 2; ++k) {
                const SmoothDisc s = smooth_disc(z[2 * k], z[2 * k + 1], a[k] * b[k], kappa);
                const double drad = newton_drad(a[k], b[k], da != nullptr ? da[k] : 0.0, db != nullptr ? db[k] : 0.0);
                d[2 * k] = newton_contact_rhs(s.D[0], s.D[1], F[2 * k], F[2 * k + 1], s.on, s.ea, drad);
                d[2 * k + 1] = newton_contact_rhs(s.D[1], s.D[2], F[2 * k], F[2 * k + 1], s.on, s.eb, drad);
            }
        } else {
            for (int i = 0; i < n; ++i) {
                const SmoothBox s = smooth_box_at<KIND>(z[i], KIND >= 2 ? a[i] : 0.0, KIND >= 2 ? b[i] : 0.0, KIND == 3 ? c[i] : 0.0, kappa);
                d[i] = smooth_box_rhs(s.D, F[i], s.elo, KIND >= 2 && da != nullptr ? da[i] : 0.0, s.ehi,
                                      KIND >= 2 && db != nullptr ? db[i] : 0.0);
            }
        }
        if (diag) {
            if (KIND == 1) {
                for (int k = 0; k < n / 2; ++k) {
                    double m[4];
                    newton_contact_block(dj + 3 * k, polish_reg(P[2 * k], reg), polish_reg(P[2 * k + 1], reg), m);
                    ok = polish_solve2(m[0], m[1], m[2], m[3], d[2 * k], d[2 * k + 1]) && ok;
                }
            } else {
                for (int i = 0; i < n; ++i) ok = polish_solve1(smooth_box_entry(true, dj[i], polish_reg(P[i], reg)), d[i]) && ok;
            }
        } else {
            smooth_matrix<KIND>(P, dj, n, false, M, reg);
            ok = polish_solve(M, n, d, n);
        }
    }
    for (int i = 0; i < n; ++i) dx[i] = ok ? d[i] : newton_nan();
    return bad ? 2 : (ok ? 0 : 1);
}

// ---- the smoothed Jacobians (dqq_newton_jac_smooth_f64) ------------------------------------------------------------------
// Column j of Jq / Ja / Jb is newton_jvp_problem_smooth's dx for dq / da / db = e_j and every other tangent NULL: the right-hand
// side by the same element functions on unit tangents formed as newton_core.h's hard Jacobian forms them, all columns through
// one elimination (polish_solve_multi) of the smoothed M, whose row operations depend on M only -- each column has the bits of
// its own newton_jvp_problem_smooth call.  dx/dP is not an output: d x_i / d P_jk = Jq_ij x_k still holds, the JVP's right-hand
// side being -D (dP x + dq).  which: 0 q, 1 a, 2 b.  hit: this row's own entry of the unit tangent is the 1.
DQQ_HD double smooth_jac_box_rhs(const SmoothBox& s, int which, bool hit)
{
    const double t = newton_t(0.0, which == 0 && hit ? 1.0 : 0.0);
    return smooth_box_rhs(s.D, t, s.elo, which == 1 && hit ? 1.0 : 0.0, s.ehi, which == 2 && hit ? 1.0 : 0.0);
}
// row r1 (0 / 1) of contact k from its SmoothDisc; hit_a, hit_b as newton_jac_contact_rhs has them
DQQ_HD double smooth_jac_contact_rhs(const SmoothDisc& s, int r1, double ln, double mu, int which, bool hit_a, bool hit_b)
{
    return newton_jac_contact_rhs(r1 ? s.D[1] : s.D[0], r1 ? s.D[2] : s.D[1], s.on, r1 ? s.eb : s.ea, ln, mu, which, hit_a, hit_b);
}
// entry (row i, column j of input `which`) of the right-hand-side block, from z and the extras: D and E are taken again from z
// (smooth_box_at / smooth_disc are functions of z, the extras and kappa alone, so the bits are smooth_eval's)
template <int KIND>
DQQ_HD double smooth_jac_rhs(const double* z, const double* a, const double* b, const double* c, int i, int which, int j, double kappa)
{
    if (KIND == 1) {
        const int k = i / 2;
        const SmoothDisc s = smooth_disc(z[2 * k], z[2 * k + 1], a[k] * b[k], kappa);
        const bool ha = which == 0 ? j == 2 * k : j == k, hb = which == 0 && j == 2 * k + 1;
        return smooth_jac_contact_rhs(s, i & 1, a[k], b[k], which, ha, hb);
    }
    const SmoothBox s = smooth_box_at<KIND>(z[i], KIND >= 2 ? a[i] : 0.0, KIND >= 2 ? b[i] : 0.0, KIND == 3 ? c[i] : 0.0, kappa);
    return smooth_jac_box_rhs(s, which, i == j);
}

// The smoothed Jacobians of one problem: newton_jac_problem's arguments, layouts, status and NaN fill, and kappa.
// work: newton_jac_work_doubles.
template <int KIND>
DQQ_HD int newton_jac_problem_smooth(const double* P, bool diag, const double* q, const double* a, const double* b, const double* c,
                                     const double* x, double* Jq, double* Ja, double* Jb, int n, double* work, double reg, double kappa)
{
#pragma clang fp contract(off)
    if (kappa == 0.0) return newton_jac_problem<KIND>(P, diag, q, a, b, c, x, Jq, Ja, Jb, n, work, false, reg);
    double* M = work;
    double* z = M + (long)n * n;
    double* F = z + n;
    double* dj = F + n;
    double* R = z + newton_vec_doubles(n);
    const int ne = newton_jac_extra_cols(KIND, n);
    double* const out[3] = {Jq, KIND == 0 ? nullptr : Ja, KIND == 0 ? nullptr : Jb};
    const bool bad = polish_inputs_bad<KIND>(P, diag, q, a, b, c, x, n, false);
    bool ok = !bad;
    if (ok) {
        smooth_eval<KIND>(P, diag, q, a, b, c, x, n, kappa, z, F, dj);
        if (diag) {
            for (int k = 0; k < n / 2 && KIND == 1; ++k) {
                double m[4];
                newton_contact_block(dj + 3 * k, polish_reg(P[2 * k], reg), polish_reg(P[2 * k + 1], reg), m);
                for (int col = 0; col < 4; ++col) {   // q_2k, q_2k+1, l_n_k, mu_k
                    const int which = col < 2 ? 0 : col - 1, j = col < 2 ? 2 * k + col : k;
                    double d0 = smooth_jac_rhs<KIND>(z, a, b, c, 2 * k, which, j, kappa);
                    double d1 = smooth_jac_rhs<KIND>(z, a, b, c, 2 * k + 1, which, j, kappa);
                    ok = polish_solve2(m[0], m[1], m[2], m[3], d0, d1) && ok;
                    if (col < 2 && Jq != nullptr) { Jq[2 * (2 * k) + col] = d0; Jq[2 * (2 * k + 1) + col] = d1; }
                    if (col >= 2 && out[which] != nullptr) { out[which][2 * k] = d0; out[which][2 * k + 1] = d1; }
                }
            }
            for (int i = 0; i < n && KIND != 1; ++i)
                for (int which = 0; which < (KIND == 0 ? 1 : 3); ++which) {
                    double d = smooth_jac_rhs<KIND>(z, a, b, c, i, which, i, kappa);
                    ok = polish_solve1(smooth_box_entry(true, dj[i], polish_reg(P[i], reg)), d) && ok;
                    if (out[which] != nullptr) out[which][i] = d;
                }
        } else {
            int ncol = 0, off[3];
            for (int which = 0; which < 3; ++which) {
                off[which] = ncol;
                if (out[which] != nullptr) ncol += which == 0 ? n : ne;
            }
            for (int i = 0; i < n; ++i)
                for (int which = 0; which < 3; ++which)
                    if (out[which] != nullptr)
                        for (int j = 0; j < (which == 0 ? n : ne); ++j)
                            R[(long)i * ncol + off[which] + j] = smooth_jac_rhs<KIND>(z, a, b, c, i, which, j, kappa);
            smooth_matrix<KIND>(P, dj, n, false, M, reg);
            ok = polish_solve_multi(M, n, R, ncol, n, ncol);
            for (int i = 0; i < n && ok; ++i)
                for (int which = 0; which < 3; ++which)
                    if (out[which] != nullptr) {
                        const int w = which == 0 ? n : ne;
                        for (int j = 0; j < w; ++j) out[which][(long)i * w + j] = R[(long)i * ncol + off[which] + j];
                    }
        }
    }
    if (!ok) {
        const double nan = newton_nan();
        for (int which = 0; which < 3; ++which)
            if (out[which] != nullptr) {
                const long cnt = diag ? (KIND == 1 && which == 0 ? 2L * n : n) : (long)n * (which == 0 ? n : ne);
                for (long i = 0; i < cnt; ++i) out[which][i] = nan;
            }
    }
    return bad ? 2 : (ok ? 0 : 1);
}

// The smoothed reverse-mode derivative of one problem (dqq_newton_bwd_smooth_f64): newton_bwd_problem's arguments and kappa
template <int KIND>
DQQ_HD int newton_bwd_problem_smooth(const double* P, bool diag, const double* q, const double* a, const double* b, const double* c,
                                     const double* x, const double* gx, double* gP, double* gq, double* ga, double* gb, int n,
                                     double* work, double reg, double kappa)
{
#pragma clang fp contract(off)
    if (kappa == 0.0) return newton_bwd_problem<KIND>(P, diag, q, a, b, c, x, gx, gP, gq, ga, gb, n, work, false, reg);
    double* M = work;
    double* z = M + (long)n * n;
    double* F = z + n;
    double* dj = F + n;
    double* w = dj + 2 * n;
    double* v = w + n;
    const int ne = KIND == 0 ? 0 : (KIND == 1 ? n / 2 : n);
    const bool bad = polish_inputs_bad<KIND>(P, diag, q, a, b, c, x, n, false) || newton_vec_bad(gx, n);
    bool ok = !bad;
    if (ok) {
        smooth_eval<KIND>(P, diag, q, a, b, c, x, n, kappa, z, F, dj);
        for (int i = 0; i < n; ++i) w[i] = gx[i];
        if (diag) {
            if (KIND == 1) {
                for (int k = 0; k < n / 2; ++k) {
                    double m[4];
                    newton_contact_block(dj + 3 * k, polish_reg(P[2 * k], reg), polish_reg(P[2 * k + 1], reg), m);
                    ok = polish_solve2(m[0], m[2], m[1], m[3], w[2 * k], w[2 * k + 1]) && ok;
                }
            } else {
                for (int i = 0; i < n; ++i) ok = polish_solve1(smooth_box_entry(true, dj[i], polish_reg(P[i], reg)), w[i]) && ok;
            }
        } else {
            smooth_matrix<KIND>(P, dj, n, true, M, reg);
            ok = polish_solve(M, n, w, n);
        }
    }
    if (!ok) {
        const double nan = newton_nan();
        if (gP != nullptr) for (long i = 0; i < (diag ? n : (long)n * n); ++i) gP[i] = nan;
        if (gq != nullptr) for (int i = 0; i < n; ++i) gq[i] = nan;
        if (ga != nullptr) for (int i = 0; i < ne; ++i) ga[i] = nan;
        if (gb != nullptr) for (int i = 0; i < ne; ++i) gb[i] = nan;
        return bad ? 2 : 1;
    }
    if (KIND == 1) {
        for (int k = 0; k < n / 2; ++k) {
            const SmoothDisc s = smooth_disc(z[2 * k], z[2 * k + 1], a[k] * b[k], kappa);
            v[2 * k] = newton_contact_v(s.D[0], s.D[1], w[2 * k], w[2 * k + 1]);
            v[2 * k + 1] = newton_contact_v(s.D[1], s.D[2], w[2 * k], w[2 * k + 1]);
            const double t = newton_contact_t(s.ea, s.eb, w[2 * k], w[2 * k + 1]);
            if (ga != nullptr) ga[k] = s.on ? newton_mul(b[k], t) : 0.0;
            if (gb != nullptr) gb[k] = s.on ? newton_mul(a[k], t) : 0.0;
        }
    } else {
        for (int i = 0; i < n; ++i) {
            const SmoothBox s = smooth_box_at<KIND>(z[i], KIND >= 2 ? a[i] : 0.0, KIND >= 2 ? b[i] : 0.0, KIND == 3 ? c[i] : 0.0, kappa);
            v[i] = newton_mul(s.D, w[i]);
            if (KIND >= 2 && ga != nullptr) ga[i] = newton_mul(s.elo, w[i]);
            if (KIND >= 2 && gb != nullptr) gb[i] = newton_mul(s.ehi, w[i]);
        }
    }
    if (gq != nullptr) for (int i = 0; i < n; ++i) gq[i] = -v[i];
    if (gP != nullptr) {
        if (diag) for (int i = 0; i < n; ++i) gP[i] = newton_gP(v[i], x[i]);
        else for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) gP[(long)i * n + j] = newton_gP(v[i], x[j]);
    }
    return 0;
}

} // namespace dqq
