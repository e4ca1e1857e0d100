// polish_core.h -- the arithmetic of the polish (dqq_polish_f64), host/device and without a lane notion: a semismooth Newton
// iteration on the natural residual that keeps a step only if it lowers the residual.  polish_diag.hip and polish_dense.hip
// run these functions with their own thread mappings; polish_problem below runs them on one thread
// (tests/hostcore/polish_core_check.cpp) and is what the kernels must reproduce bit for bit.  tests/polish_reference.py is
// the same definition in numpy.  No fused multiply-add is formed but the one check_proj_circle writes out.
//
// Per problem, float64.  PI: the kind's projection (check_core.h; kind 3 on the effective bounds of sbox_bounds.h, the QP on
// [0, +inf)).  With P the (n,n) matrix (DQQ_P_DIAG: its diagonal):
//   g_i   = (0 + P_i0 x_0 + P_i1 x_1 + ...) + q_i        products and sums rounded one by one, in index order
//           (DQQ_P_DIAG: (0 + p_i x_i) + q_i -- what the full sum leaves when the other entries are zeros)
//   z     = x - g,   F = x - PI(z),   r = max |F_i| by nmax in index order (a NaN survives)
//   D     = the generalised Jacobian of PI at z:  box-like kinds D_ii = 1 if lo_i < z_i < hi_i else 0;  QCQP contact with
//           rad = l_n mu, n2 = fma(z_b, z_b, z_a z_a): not (n2 > rad |rad|): I_2;  else rad > 0: with nrm = sqrt(n2),
//           sc = rad / nrm, u = z / nrm:  [[sc (1 - u_a u_a), sc (0 - u_a u_b)], [., sc (1 - u_b u_b)]];  else 0
//   M     = (I - D) + D P:  box-like kinds: row i of P where D_ii = 1, the unit row otherwise;  QCQP rows of contact c:
//           M_rj = (delta_rj - D_rj) + (D_r,2c P_2c,j + D_r,2c+1 P_2c+1,j)
//   M d = -F by Gaussian elimination with partial pivoting (polish_solve), no refinement;  x+ = PI(x + d);  accepted iff
//           r+ < r;  stop at r == 0, at a failed or rejected step, or after max_steps accepted steps.
// Elimination order (polish_solve): column k = 0 .. n-1: the pivot is the first largest |M_ik|, i >= k (a NaN below row k is
// passed over); zero or not finite: the step fails.  Rows k and the pivot's swap (columns >= k, and the right-hand side).
// f_i = M_ik / M_kk; where f_i is not a zero: rhs_i = rhs_i - f_i rhs_k, M_ij = M_ij - f_i M_kj (j > k).  Back substitution by
// columns, k = n-1 .. 0: d_k = rhs_k / M_kk; where M_ik is not a zero (i < k): rhs_i = rhs_i - M_ik d_k.  An exact zero never
// enters the arithmetic, so a block-diagonal M is solved block by block with the same bits (polish_solve1 / polish_solve2:
// DQQ_P_DIAG) and unit rows cost nothing.
// Status: 2 if an entry of P, q, the kind's extras or x, or the first r, is not finite (x_out = x); else 0 if a step was
// accepted, 1 if x was kept.  resid_out = (first r, last accepted r); steps_out = accepted steps.
//
// One-sided boxes (DQQ_F_INFINITE_BOUNDS, inf_ok below; box and signed box only).  The input rule of the two bounds alone
// changes (polish_lo_bad / polish_hi_bad): l_min may be -inf, l_max may be +inf; l_min = +inf, l_max = -inf and a NaN stay
// status 2, and so does every other entry that is not finite (P, q, x, v, the first r; newton_core.h: grad_x and the tangents).
// Nothing else is written for the flag: PI, D and the Newton cores' E are the comparisons above (check_proj, polish_free,
// newton_box_state), sbox_bounds.h selects, and no expression takes a bound as an operand of arithmetic -- no width, no
// midpoint, no product.  A finite z is never at or beyond an infinite side, so that side is never sat on: the results are, bit
// for bit and signed zeros included, those of the unflagged call with the infinite bounds replaced by any finite bound no
// iterate reaches.  QCQP radii stay finite-only.
//
// The proximal weight (dqq_polish_reg_f64 and the *_reg_f64 entries of newton_core.h; reg >= 0, finite).  reg enters only where
// M is formed: P is replaced by P' with P'_ii = P_ii + reg, one rounded add (polish_reg), and P'_ij = P_ij off the diagonal, so
// M_reg = (I - D) + D P'.  Box-like kinds: the diagonal entry of a free row; a unit row has none.  QCQP: pa of
// polish_contact_entry in column 2c, pb in column 2c+1 -- the contact's own two diagonal entries of P, in both of its rows.
// DQQ_P_DIAG: the p of the 1 x 1 and 2 x 2 blocks.  g, z, F, r, D, E, the right-hand sides, the acceptance test and grad_P use
// the caller's P.  reg == 0 does not add (a -0.0 stays -0.0): every output is the unregularised one bit for bit.  For P
// positive semidefinite and reg > 0, M_reg is nonsingular (DESIGN 4.11's argument on P + reg I).
//
// The damped polish (dqq_polish_ls_f64, polish_problem_ls).  Everything above but the step: with d from M d = -F (a
// failed elimination ends the loop as above), trial points x_k = PI(x + t_k d), t_k = 2^-k, k = 0 .. max_halvings (polish_trial:
// the product t_k d, exact but for underflow, and the sum rounded one by one), r_k = r(x_k); the first k with r_k < r is accepted
// (a NaN r_k is not); if none is, the loop ends and x is kept.  An accepted k counts one step and k halvings: `halvings` is the
// number of rejected trial points that came before the accepted ones (the trial points of a last step that accepts none are not
// counted).  d is solved for once per step.  max_halvings = 0 is the polish above bit for bit (1 d is d), and so is any
// max_halvings on a problem whose full steps are all accepted; r after <= r before always.
#pragma once

#include "check_core.h"
#include "sbox_bounds.h"

namespace dqq {

// the doubles polish_problem / a kernel's team needs besides the matrix: x, x+, F, z, d and the Jacobian (2n)
DQQ_HD long polish_vec_doubles(int n) { return 7L * n; }

DQQ_HD bool polish_zero(double v) { return v == 0.0; }

// P'_ii of the proximal weight: the kernels' REG = true instantiations add; the one-thread cores add unless reg is a zero
DQQ_HD double polish_reg_add(double p, double reg)
{
#pragma clang fp contract(off)
    return p + reg;
}
DQQ_HD double polish_reg(double p, double reg) { return reg != 0.0 ? polish_reg_add(p, reg) : p; }

// the effective interval of a coordinate of the box-like kinds
template <int KIND>
DQQ_HD void polish_bounds(double a, double b, double c, double& lo, double& hi)
{
    if (KIND == 0) { lo = 0.0; hi = __builtin_inf(); }
    else if (KIND == 3) { const SBoxBounds e = sbox_bounds(a, b, c); lo = e.lo; hi = e.hi; }
    else { lo = a; hi = b; }
}

template <int KIND>
DQQ_HD double polish_proj(double t, double lo, double hi)
{
    return KIND == 0 ? check_proj<0>(t, 0.0, 0.0, 0.0) : check_proj<2>(t, lo, hi, 0.0);
}

// one term of a row sum, and the row sum's end
DQQ_HD double polish_acc(double s, double p, double x)
{
#pragma clang fp contract(off)
    return s + p * x;
}
DQQ_HD double polish_z(double x, double s, double q)
{
#pragma clang fp contract(off)
    return x - (s + q);
}

// a trial point's coordinate before PI: x + t d, the product and the sum rounded one by one (t = 1: x + d, the full step's bits)
DQQ_HD double polish_trial(double x, double t, double d)
{
#pragma clang fp contract(off)
    const double s = t * d;
    return x + s;
}
// the next step length: t is a power of two from 1 down to 2^-60, so the product is exact
DQQ_HD double polish_half(double t) { return 0.5 * t; }

// box-like kinds: F_i, and whether the coordinate is free (D_ii = 1)
template <int KIND>
DQQ_HD double polish_F(double x, double z, double lo, double hi)
{
#pragma clang fp contract(off)
    return x - polish_proj<KIND>(z, lo, hi);
}
DQQ_HD bool polish_free(double z, double lo, double hi) { return lo < z && z < hi; }

// the input rule of a box kind's bounds: finite; with inf_ok (DQQ_F_INFINITE_BOUNDS) the lower bound may also be -inf, the
// upper bound +inf (a NaN fails both comparisons)
DQQ_HD bool polish_lo_bad(double lo, bool inf_ok) { return inf_ok ? !(lo < __builtin_inf()) : !__builtin_isfinite(lo); }
DQQ_HD bool polish_hi_bad(double hi, bool inf_ok) { return inf_ok ? !(hi > -__builtin_inf()) : !__builtin_isfinite(hi); }

// QCQP: F of a contact, and D_c as (d00, d01, d11)
DQQ_HD void polish_F_contact(double xa, double xb, double za, double zb, double rad, double& Fa, double& Fb)
{
#pragma clang fp contract(off)
    double pa = za, pb = zb;
    check_proj_circle(pa, pb, rad);
    Fa = xa - pa;
    Fb = xb - pb;
}
DQQ_HD void polish_disc_jacobian(double za, double zb, double rad, double (&D)[3])
{
#pragma clang fp contract(off)
    const double n2 = __builtin_fma(zb, zb, za * za);
    if (!(n2 > rad * fabs(rad))) { D[0] = 1.0; D[1] = 0.0; D[2] = 1.0; return; }
    if (!(rad > 0.0)) { D[0] = D[1] = D[2] = 0.0; return; }
    const double nrm = sqrt(n2), sc = rad / nrm, ua = za / nrm, ub = zb / nrm;
    D[0] = sc * (1.0 - ua * ua);
    D[1] = sc * (0.0 - ua * ub);
    D[2] = sc * (1.0 - ub * ub);
}
// M_rj of a contact's row r: (dr0, dr1) that row of D_c, djr its entry in column j (0 outside the contact), pa / pb the
// entries of P's rows 2c / 2c+1 in column j
DQQ_HD double polish_contact_entry(bool on_diag, double djr, double dr0, double dr1, double pa, double pb)
{
#pragma clang fp contract(off)
    return ((on_diag ? 1.0 : 0.0) - djr) + (dr0 * pa + dr1 * pb);
}

// the pivot test of a column's largest |entry|
DQQ_HD bool polish_pivot_ok(double best) { return best > 0.0 && __builtin_isfinite(best); }

// M d = rhs, in place (M: n x n, row stride ld; d: rhs in, solution out).  false: a pivot was zero or not finite.
DQQ_HD bool polish_solve(double* M, long ld, double* d, int n)
{
#pragma clang fp contract(off)
    for (int k = 0; k < n; ++k) {
        double best = fabs(M[k * ld + k]);
        int piv = k;
        for (int i = k + 1; i < n; ++i) {
            const double v = fabs(M[i * ld + k]);
            if (v > best) { best = v; piv = i; }
        }
        if (!polish_pivot_ok(best)) return false;
        if (piv != k) {
            for (int j = k; j < n; ++j) { const double t = M[k * ld + j]; M[k * ld + j] = M[piv * ld + j]; M[piv * ld + j] = t; }
            const double t = d[k]; d[k] = d[piv]; d[piv] = t;
        }
        const double pv = M[k * ld + k];
        for (int i = k + 1; i < n; ++i) {
            const double f = M[i * ld + k] / pv;
            if (polish_zero(f)) continue;
            d[i] = d[i] - f * d[k];
            for (int j = k + 1; j < n; ++j) M[i * ld + j] = M[i * ld + j] - f * M[k * ld + j];
        }
    }
    for (int k = n - 1; k >= 0; --k) {
        d[k] = d[k] / M[k * ld + k];
        for (int i = 0; i < k; ++i)
            if (!polish_zero(M[i * ld + k])) d[i] = d[i] - M[i * ld + k] * d[k];
    }
    return true;
}

// polish_solve with nrhs right-hand sides (R: n x nrhs, row stride ldr; column c in, the solution of column c out): the pivot
// search, the swap, the zero-skip on multipliers and matrix entries and the back substitution by columns are polish_solve's and
// depend on M only, so every column comes out with the bits polish_solve gives it alone.
DQQ_HD bool polish_solve_multi(double* M, long ld, double* R, long ldr, int n, int nrhs)
{
#pragma clang fp contract(off)
    for (int k = 0; k < n; ++k) {
        double best = fabs(M[k * ld + k]);
        int piv = k;
        for (int i = k + 1; i < n; ++i) {
            const double v = fabs(M[i * ld + k]);
            if (v > best) { best = v; piv = i; }
        }
        if (!polish_pivot_ok(best)) return false;
        if (piv != k) {
            for (int j = k; j < n; ++j) { const double t = M[k * ld + j]; M[k * ld + j] = M[piv * ld + j]; M[piv * ld + j] = t; }
            for (int c = 0; c < nrhs; ++c) { const double t = R[k * ldr + c]; R[k * ldr + c] = R[piv * ldr + c]; R[piv * ldr + c] = t; }
        }
        const double pv = M[k * ld + k];
        for (int i = k + 1; i < n; ++i) {
            const double f = M[i * ld + k] / pv;
            if (polish_zero(f)) continue;
            for (int c = 0; c < nrhs; ++c) R[i * ldr + c] = R[i * ldr + c] - f * R[k * ldr + c];
            for (int j = k + 1; j < n; ++j) M[i * ld + j] = M[i * ld + j] - f * M[k * ld + j];
        }
    }
    for (int k = n - 1; k >= 0; --k) {
        for (int c = 0; c < nrhs; ++c) R[k * ldr + c] = R[k * ldr + c] / M[k * ld + k];
        for (int i = 0; i < k; ++i)
            if (!polish_zero(M[i * ld + k]))
                for (int c = 0; c < nrhs; ++c) R[i * ldr + c] = R[i * ldr + c] - M[i * ld + k] * R[k * ldr + c];
    }
    return true;
}

// polish_solve on a 1 x 1 and on a 2 x 2 block, written out (registers only)
DQQ_HD bool polish_solve1(double m, double& d)
{
#pragma clang fp contract(off)
    if (!polish_pivot_ok(fabs(m))) return false;
    d = d / m;
    return true;
}
DQQ_HD bool polish_solve2(double m00, double m01, double m10, double m11, double& d0, double& d1)
{
#pragma clang fp contract(off)
    const double best = fabs(m10) > fabs(m00) ? fabs(m10) : fabs(m00);
    if (!polish_pivot_ok(best)) return false;
    if (fabs(m10) > fabs(m00)) {
        double t = m00; m00 = m10; m10 = t;
        t = m01; m01 = m11; m11 = t;
        t = d0; d0 = d1; d1 = t;
    }
    const double f = m10 / m00;
    if (!polish_zero(f)) {
        d1 = d1 - f * d0;
        m11 = m11 - f * m01;
    }
    if (!polish_pivot_ok(fabs(m11))) return false;
    d1 = d1 / m11;
    if (!polish_zero(m01)) d0 = d0 - m01 * d1;
    d0 = d0 / m00;
    return true;
}

// what a problem leaves behind
DQQ_HD int polish_status(bool bad_input, double r0, int steps)
{
    if (bad_input || !__builtin_isfinite(r0)) return 2;
    return steps > 0 ? 0 : 1;
}

// ---- one problem on one thread -----------------------------------------------------------------------------------------
// z, F, the Jacobian dj (box-like: n flags; QCQP: 3 per contact) and r at xv.  diag: P is the n diagonal entries.
template <int KIND>
DQQ_HD double polish_eval(const double* P, bool diag, const double* q, const double* a, const double* b, const double* c,
                          const double* xv, int n, double* z, double* F, double* dj)
{
    for (int i = 0; i < n; ++i) {
        double s = 0.0;
        if (diag) s = polish_acc(s, P[i], xv[i]);
        else for (int j = 0; j < n; ++j) s = polish_acc(s, P[(long)i * n + j], xv[j]);
        z[i] = polish_z(xv[i], s, q[i]);
    }
    if (KIND == 1) {
        for (int k = 0; k < n / 2; ++k) {
            const double rad = a[k] * b[k];
            polish_F_contact(xv[2 * k], xv[2 * k + 1], z[2 * k], z[2 * k + 1], rad, F[2 * k], F[2 * k + 1]);
            double D[3];
            polish_disc_jacobian(z[2 * k], z[2 * k + 1], rad, D);
            dj[3 * k] = D[0]; dj[3 * k + 1] = D[1]; dj[3 * k + 2] = D[2];
        }
    } else {
        for (int i = 0; i < n; ++i) {
            double lo, hi;
            polish_bounds<KIND>(KIND >= 2 ? a[i] : 0.0, KIND >= 2 ? b[i] : 0.0, KIND == 3 ? c[i] : 0.0, lo, hi);
            F[i] = polish_F<KIND>(xv[i], z[i], lo, hi);
            dj[i] = polish_free(z[i], lo, hi) ? 1.0 : 0.0;
        }
    }
    double r = 0.0;
    for (int i = 0; i < n; ++i) r = nmax(r, F[i]);
    return r;
}

template <int KIND>
DQQ_HD bool polish_inputs_bad(const double* P, bool diag, const double* q, const double* a, const double* b, const double* c,
                              const double* x, int n, bool inf_ok = false)
{
    bool bad = false;
    const long np = diag ? n : (long)n * n;
    for (long i = 0; i < np; ++i) bad |= !__builtin_isfinite(P[i]);
    for (int i = 0; i < n; ++i) bad |= !__builtin_isfinite(q[i]) || !__builtin_isfinite(x[i]);
    const int ne = KIND == 0 ? 0 : (KIND == 1 ? n / 2 : n);
    if (KIND >= 2) for (int i = 0; i < ne; ++i) bad |= polish_lo_bad(a[i], inf_ok) || polish_hi_bad(b[i], inf_ok);
    else for (int i = 0; i < ne; ++i) bad |= !__builtin_isfinite(a[i]) || !__builtin_isfinite(b[i]);
    if (KIND == 3) for (int i = 0; i < n; ++i) bad |= !__builtin_isfinite(c[i]);
    return bad;
}

// The whole damped polish of one problem (dqq_polish_ls_f64; max_halvings = 0: dqq_polish_reg_f64).  work: n*n +
// polish_vec_doubles(n) doubles.  x_out may be x.  inf_ok: the flag.  reg: the proximal weight of the step's matrix (acceptance
// stays r_k < r on the true residual).  halvings_out (optional): the rejected trial points before the accepted ones.  -> status
template <int KIND>
DQQ_HD int polish_problem_ls(const double* P, bool diag, const double* q, const double* a, const double* b, const double* c,
                             const double* x, double* x_out, int n, int max_steps, int max_halvings, double* resid, int* steps_out,
                             int* halvings_out, double* work, bool inf_ok = false, double reg = 0.0)
{
#pragma clang fp contract(off)
    double* M = work;
    double* xc = M + (long)n * n;
    double* xn = xc + n;
    double* F = xn + n;
    double* z = F + n;
    double* d = z + n;
    double* dj = d + n;
    const bool bad = polish_inputs_bad<KIND>(P, diag, q, a, b, c, x, n, inf_ok);
    for (int i = 0; i < n; ++i) xc[i] = x[i];
    const double r0 = polish_eval<KIND>(P, diag, q, a, b, c, xc, n, z, F, dj);
    double r = r0;
    int steps = 0, halvings = 0;
    const bool run = !bad && __builtin_isfinite(r0);
    while (run && steps < max_steps && r != 0.0) {
        bool ok = true;
        if (diag) {
            if (KIND == 1) {
                for (int k = 0; k < n / 2 && ok; ++k) {
                    const double* D = dj + 3 * k;
                    const double pa = polish_reg(P[2 * k], reg), pb = polish_reg(P[2 * k + 1], reg);
                    const double m00 = polish_contact_entry(true, D[0], D[0], D[1], pa, 0.0);
                    const double m01 = polish_contact_entry(false, D[1], D[0], D[1], 0.0, pb);
                    const double m10 = polish_contact_entry(false, D[1], D[1], D[2], pa, 0.0);
                    const double m11 = polish_contact_entry(true, D[2], D[1], D[2], 0.0, pb);
                    d[2 * k] = -F[2 * k];
                    d[2 * k + 1] = -F[2 * k + 1];
                    ok = polish_solve2(m00, m01, m10, m11, d[2 * k], d[2 * k + 1]);
                }
            } else {
                for (int i = 0; i < n && ok; ++i) {
                    d[i] = -F[i];
                    ok = polish_solve1(dj[i] != 0.0 ? polish_reg(P[i], reg) : 1.0, d[i]);
                }
            }
        } else {
            for (int i = 0; i < n; ++i) {
                d[i] = -F[i];
                for (int j = 0; j < n; ++j) {
                    if (KIND == 1) {
                        const int k = i / 2, r1 = i & 1;
                        const double* D = dj + 3 * k;
                        const double dr0 = r1 ? D[1] : D[0], dr1 = r1 ? D[2] : D[1];
                        const double djr = j == 2 * k ? dr0 : (j == 2 * k + 1 ? dr1 : 0.0);
                        const double pa = P[(long)(2 * k) * n + j], pb = P[(long)(2 * k + 1) * n + j];
                        M[(long)i * n + j] = polish_contact_entry(i == j, djr, dr0, dr1, j == 2 * k ? polish_reg(pa, reg) : pa,
                                                                  j == 2 * k + 1 ? polish_reg(pb, reg) : pb);
                    } else {
                        const double pij = P[(long)i * n + j];
                        M[(long)i * n + j] = dj[i] != 0.0 ? (i == j ? polish_reg(pij, reg) : pij) : (i == j ? 1.0 : 0.0);
                    }
                }
            }
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
            rn = polish_eval<KIND>(P, diag, q, a, b, c, xn, n, z, F, dj);
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

// The polish that takes full steps only (dqq_polish_f64, dqq_polish_reg_f64): the damped one with no halving allowed.
template <int KIND>
DQQ_HD int polish_problem(const double* P, bool diag, const double* q, const double* a, const double* b, const double* c,
                          const double* x, double* x_out, int n, int max_steps, double* resid, int* steps_out, double* work,
                          bool inf_ok = false, double reg = 0.0)
{
    return polish_problem_ls<KIND>(P, diag, q, a, b, c, x, x_out, n, max_steps, 0, resid, steps_out, nullptr, work, inf_ok, reg);
}

} // namespace dqq
