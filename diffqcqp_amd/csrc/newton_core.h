// newton_core.h -- the arithmetic of the Newton derivatives (dqq_newton_bwd_f64, dqq_newton_jvp_f64), host/device and without
// a lane notion: both modes of the implicit derivative of F(x) = x - PI(x - (P x + q)) = 0 from the polish's Jacobian
// M = (I - D) + D P.  No regularisation, no epsilon, no refinement: one elimination per problem, and the two modes are each
// other's transpose to rounding.  newton_diag.hip and newton_dense.hip run these functions with their own thread mappings;
// newton_jvp_problem / newton_bwd_problem below run them on one thread (tests/hostcore/newton_core_check.cpp) and are what the
// kernels must reproduce bit for bit.  tests/newton_reference.py is the same definition in numpy.  No fused multiply-add is
// formed but the one polish_disc_jacobian writes out.
//
// Per problem, float64, at the x given (meant to be a polished point; it does not have to be).  z, D and M: polish_core.h's, at
// x (box-like kinds on polish_bounds' interval, the signed box on sbox_bounds.h's effective bounds).
//   E     = dPI/dtheta at z.  Box-like coordinate that is not free (polish_free false): z_i <= lo_i: E_lo,i = 1; else
//           z_i >= hi_i: E_hi,i = 1; else none.  The QP has no extras.  Signed box: the entry belongs to l_min / l_max only where
//           lo' == l_min / hi' == l_max (keep_lo / keep_hi, ties included); elsewhere it is the constant 0's.  v takes nothing.
//           QCQP contact, rad = l_n mu: outside the disc (polish_disc_jacobian's n2 > rad |rad|) with rad > 0: E_rad = u = z / nrm,
//           the u of D, and d rad = mu dl_n + l_n dmu; otherwise 0 (at rad <= 0 a subgradient choice, the one D makes).
//   M dx  = -D (dP x + dq) + E dtheta
// JVP:      s_i = (0 + dP_i0 x_0 + dP_i1 x_1 + ...) (DQQ_P_DIAG: 0 + dp_i x_i), t_i = s_i + dq_i;
//           box-like: rhs_i = -t_i where free, else the bound's tangent E selects, else 0;
//           contact row r: w = D_r0 t_a + D_r1 t_b, rhs_r = u_r drad - w where E is on, else -w;
//           dx = M^-1 rhs by polish_solve (DQQ_P_DIAG: polish_solve1 / polish_solve2).  A NULL tangent reads as 0.0.
// Backward: M' w = grad_x by the same elimination on the transposed matrix (the buffer holds M_ji; DQQ_P_DIAG: the contact
//           block's off-diagonals swapped);  v = D w (box-like: w_i where free, else +0.0; contact: D_r0 w_a + D_r1 w_b);
//           grad_q = -v;  grad_P_ij = -(v_i x_j) (DQQ_P_DIAG: -(v_i x_i));  grad_lo_i / grad_hi_i = w_i where E is 1, else +0.0;
//           contact: t = u_a w_a + u_b w_b, grad_l_n = mu t, grad_mu = l_n t where E is on, else +0.0.
// polish_solve's zero-skip rule holds, so a block-diagonal M or M' is solved block by block with the same bits: a diagonal P
// given as (n,n) gives DQQ_P_DIAG's bits.
// Status: 2 if an entry of P, q, the kind's extras, x, grad_x or a given tangent is not finite (polish_inputs_bad's rule,
// infinite bounds included); else 1 if the elimination met a zero or non-finite pivot; else 0.  Status 1 and 2: every
// requested output of the problem is NaN.
// One-sided boxes (inf_ok: DQQ_F_INFINITE_BOUNDS, box and signed box): polish_core.h's rule -- polish_inputs_bad admits
// l_min = -inf and l_max = +inf, a tangent or cotangent stays finite-only.  newton_box_state's comparisons never put a finite z
// on an infinite side, so its E entry is 0: grad_l_min / grad_l_max there is the +0.0 of a never-active bound, its column of
// Ja / Jb the zeros the finite-bound path gives such a column, and its tangent da / db is not read into the right-hand side.
// The proximal weight reg (the *_reg_f64 entries): polish_core.h's rule -- M_reg = (I - D) + D (P + reg I) replaces M in the one
// elimination of each mode (backward: M_reg' w = grad_x; JVP and Jacobians: M_reg dx = rhs); z, D, E, the right-hand sides, v = D w
// and grad_P = -v x' are the caller's P's.  Both modes share M_reg and stay adjoint to rounding.  reg == 0: today's bits.
#pragma once

#include "polish_core.h"

namespace dqq {

// a box-like coordinate at z: 0 free (D_ii = 1); 1 on the lower bound, which is the caller's; 2 on the upper bound, the caller's;
// 3 fixed on a constant (the QP's 0, the sign constraint's 0) or on neither bound (z is a NaN)
constexpr int kNewtonFree = 0, kNewtonLo = 1, kNewtonHi = 2, kNewtonConst = 3;

template <int KIND>
DQQ_HD int newton_box_state(double z, double a, double b, double c)
{
    double lo, hi;
    bool keep_lo = KIND == 2, keep_hi = KIND == 2;
    if (KIND == 3) {
        const SBoxBounds e = sbox_bounds(a, b, c);
        lo = e.lo; hi = e.hi; keep_lo = e.keep_lo; keep_hi = e.keep_hi;
    } else {
        polish_bounds<KIND>(a, b, c, lo, hi);
    }
    if (polish_free(z, lo, hi)) return kNewtonFree;
    if (z <= lo) return keep_lo ? kNewtonLo : kNewtonConst;
    if (z >= hi) return keep_hi ? kNewtonHi : kNewtonConst;
    return kNewtonConst;
}

// E of a contact: whether it is on, and u (polish_disc_jacobian's n2, nrm and quotients)
DQQ_HD bool newton_disc_u(double za, double zb, double rad, double& ua, double& ub)
{
#pragma clang fp contract(off)
    const double n2 = __builtin_fma(zb, zb, za * za);
    ua = ub = 0.0;
    if (!(n2 > rad * fabs(rad)) || !(rad > 0.0)) return false;
    const double nrm = sqrt(n2);
    ua = za / nrm;
    ub = zb / nrm;
    return true;
}

DQQ_HD double newton_t(double s, double dq)
{
#pragma clang fp contract(off)
    return s + dq;
}
DQQ_HD double newton_box_rhs(int state, double t, double dlo, double dhi)
{
    return state == kNewtonFree ? -t : (state == kNewtonLo ? dlo : (state == kNewtonHi ? dhi : 0.0));
}
DQQ_HD double newton_drad(double ln, double mu, double dln, double dmu)
{
#pragma clang fp contract(off)
    return mu * dln + ln * dmu;
}
// row r of a contact: (dr0, dr1) that row of D_c, u its entry of u
DQQ_HD double newton_contact_rhs(double dr0, double dr1, double ta, double tb, bool on, double u, double drad)
{
#pragma clang fp contract(off)
    const double w = dr0 * ta + dr1 * tb;
    return on ? u * drad - w : -w;
}
DQQ_HD double newton_contact_v(double dr0, double dr1, double wa, double wb)
{
#pragma clang fp contract(off)
    return dr0 * wa + dr1 * wb;
}
DQQ_HD double newton_contact_t(double ua, double ub, double wa, double wb)
{
#pragma clang fp contract(off)
    return ua * wa + ub * wb;
}
DQQ_HD double newton_mul(double a, double b)
{
#pragma clang fp contract(off)
    return a * b;
}
DQQ_HD double newton_gP(double v, double x)
{
#pragma clang fp contract(off)
    return -(v * x);
}

DQQ_HD double newton_nan() { return __builtin_nan(""); }

DQQ_HD bool newton_vec_bad(const double* p, long n)
{
    bool bad = false;
    if (p != nullptr) for (long i = 0; i < n; ++i) bad |= !__builtin_isfinite(p[i]);
    return bad;
}

// the doubles a problem needs besides the matrix: z, F (polish_eval's, unused), the Jacobian (2n), the right-hand side /
// solution, v or s -- within polish_vec_doubles
DQQ_HD long newton_vec_doubles(int n) { return polish_vec_doubles(n); }

// ---- one problem on one thread -----------------------------------------------------------------------------------------
// M (transposed: M') into the n x n buffer from P and the Jacobian dj of polish_eval
template <int KIND>
DQQ_HD void newton_matrix(const double* P, const double* dj, int n, bool transposed, double* M, double reg = 0.0)
{
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            double m;
            if (KIND == 1) {
                const int k = i / 2, r1 = i & 1;
                const double* D = dj + 3 * k;
                const double dr0 = r1 ? D[1] : D[0], dr1 = r1 ? D[2] : D[1];
                const double djr = j == 2 * k ? dr0 : (j == 2 * k + 1 ? dr1 : 0.0);
                const double pa = P[(long)(2 * k) * n + j], pb = P[(long)(2 * k + 1) * n + j];
                m = polish_contact_entry(i == j, djr, dr0, dr1, j == 2 * k ? polish_reg(pa, reg) : pa,
                                         j == 2 * k + 1 ? polish_reg(pb, reg) : pb);
            } else {
                const double pij = P[(long)i * n + j];
                m = dj[i] != 0.0 ? (i == j ? polish_reg(pij, reg) : pij) : (i == j ? 1.0 : 0.0);
            }
            M[transposed ? (long)j * n + i : (long)i * n + j] = m;
        }
}

// the 2 x 2 block of contact k on the compact diagonal: (m00, m01, m10, m11); pa, pb: P's (P''s) two diagonal entries
DQQ_HD void newton_contact_block(const double* D, double pa, double pb, double (&m)[4])
{
    m[0] = polish_contact_entry(true, D[0], D[0], D[1], pa, 0.0);
    m[1] = polish_contact_entry(false, D[1], D[0], D[1], 0.0, pb);
    m[2] = polish_contact_entry(false, D[1], D[1], D[2], pa, 0.0);
    m[3] = polish_contact_entry(true, D[2], D[1], D[2], 0.0, pb);
}

// The forward-mode derivative of one problem.  dP, dq, da, db: NULL = zero.  work: n*n + newton_vec_doubles(n).  -> status
template <int KIND>
DQQ_HD int newton_jvp_problem(const double* P, bool diag, const double* q, const double* a, const double* b, const double* c,
                              const double* x, const double* dP, const double* dq, const double* da, const double* db, double* dx,
                              int n, double* work, bool inf_ok = false, double reg = 0.0)
{
#pragma clang fp contract(off)
    double* M = work;
    double* z = M + (long)n * n;
    double* F = z + n;
    double* dj = F + n;
    double* d = dj + 2 * n;
    const int ne = KIND == 0 ? 0 : (KIND == 1 ? n / 2 : n);
    bool bad = polish_inputs_bad<KIND>(P, diag, q, a, b, c, x, n, inf_ok);
    bad |= newton_vec_bad(dP, diag ? n : (long)n * n) || newton_vec_bad(dq, n) || newton_vec_bad(da, ne) || newton_vec_bad(db, ne);
    bool ok = !bad;
    if (ok) {
        polish_eval<KIND>(P, diag, q, a, b, c, x, n, z, F, dj);
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
                const double* D = dj + 3 * k;
                double ua, ub;
                const bool on = newton_disc_u(z[2 * k], z[2 * k + 1], a[k] * b[k], ua, ub);
                const double drad = newton_drad(a[k], b[k], da != nullptr ? da[k] : 0.0, db != nullptr ? db[k] : 0.0);
                d[2 * k] = newton_contact_rhs(D[0], D[1], F[2 * k], F[2 * k + 1], on, ua, drad);
                d[2 * k + 1] = newton_contact_rhs(D[1], D[2], F[2 * k], F[2 * k + 1], on, ub, drad);
            }
        } else {
            for (int i = 0; i < n; ++i) {
                const int st = newton_box_state<KIND>(z[i], KIND >= 2 ? a[i] : 0.0, KIND >= 2 ? b[i] : 0.0, KIND == 3 ? c[i] : 0.0);
                d[i] = newton_box_rhs(st, F[i], da != nullptr ? da[i] : 0.0, db != nullptr ? db[i] : 0.0);
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
                for (int i = 0; i < n; ++i) ok = polish_solve1(dj[i] != 0.0 ? polish_reg(P[i], reg) : 1.0, d[i]) && ok;
            }
        } else {
            newton_matrix<KIND>(P, dj, n, false, M, reg);
            ok = polish_solve(M, n, d, n);
        }
    }
    for (int i = 0; i < n; ++i) dx[i] = ok ? d[i] : newton_nan();
    return bad ? 2 : (ok ? 0 : 1);
}

// ---- the Jacobians (dqq_newton_jac_f64) ----------------------------------------------------------------------------------
// Column j of Jq / Ja / Jb is newton_jvp_problem's dx for dq / da / db = e_j and every other tangent NULL: the right-hand side
// by the same element functions, all columns through one elimination (polish_solve_multi), whose row operations depend on M
// only -- each column has the bits of its own newton_jvp_problem call.  dx/dP is not an output: d x_i / d P_jk = Jq_ij x_k.
// which: 0 q, 1 a, 2 b.  hit: this row's own entry of the unit tangent is the 1.
DQQ_HD double newton_jac_box_rhs(int state, int which, bool hit)
{
    const double t = newton_t(0.0, which == 0 && hit ? 1.0 : 0.0);
    return newton_box_rhs(state, t, which == 1 && hit ? 1.0 : 0.0, which == 2 && hit ? 1.0 : 0.0);
}
// row r of contact k: (dr0, dr1) that row of D_c, u its entry of u.  which 0: hit_a / hit_b: j is 2k / 2k+1; which 1, 2: hit_a: j
// is k
DQQ_HD double newton_jac_contact_rhs(double dr0, double dr1, bool on, double u, double ln, double mu, int which, bool hit_a,
                                     bool hit_b)
{
    const double ta = newton_t(0.0, which == 0 && hit_a ? 1.0 : 0.0), tb = newton_t(0.0, which == 0 && hit_b ? 1.0 : 0.0);
    const double drad = newton_drad(ln, mu, which == 1 && hit_a ? 1.0 : 0.0, which == 2 && hit_a ? 1.0 : 0.0);
    return newton_contact_rhs(dr0, dr1, ta, tb, on, u, drad);
}
// entry (row i, column j of input `which`) of the right-hand-side block, from z, the Jacobian dj of polish_eval and the extras
template <int KIND>
DQQ_HD double newton_jac_rhs(const double* z, const double* dj, const double* a, const double* b, const double* c, int i, int which,
                             int j)
{
    if (KIND == 1) {
        const int k = i / 2;
        const double* D = dj + 3 * k;
        double ua, ub;
        const bool on = newton_disc_u(z[2 * k], z[2 * k + 1], a[k] * b[k], ua, ub);
        const bool ha = which == 0 ? j == 2 * k : j == k, hb = which == 0 && j == 2 * k + 1;
        return (i & 1) ? newton_jac_contact_rhs(D[1], D[2], on, ub, a[k], b[k], which, ha, hb)
                       : newton_jac_contact_rhs(D[0], D[1], on, ua, a[k], b[k], which, ha, hb);
    }
    const int st = newton_box_state<KIND>(z[i], KIND >= 2 ? a[i] : 0.0, KIND >= 2 ? b[i] : 0.0, KIND == 3 ? c[i] : 0.0);
    return newton_jac_box_rhs(st, which, i == j);
}

// columns of an extra's Jacobian on a general P
DQQ_HD int newton_jac_extra_cols(int kind, int n) { return kind == 0 ? 0 : (kind == 1 ? n / 2 : n); }
// the doubles newton_jac_problem needs: the matrix, the vectors and the block of every column the kind has
DQQ_HD long newton_jac_work_doubles(int kind, int n)
{
    return (long)n * n + newton_vec_doubles(n) + (long)n * (n + 2 * newton_jac_extra_cols(kind, n));
}

// The Jacobians of one problem; each of Jq, Ja, Jb: NULL = not requested.  General P: Jq (n,n) row-major, Jq[i*n+j] = dx_i/dq_j;
// Ja, Jb (n,ne).  diag (the Jacobians are block-diagonal, the outputs compact): box-like kinds Jq, Ja, Jb (n): dx_i/dq_i,
// dx_i/da_i, dx_i/db_i; QCQP Jq (n,2): row i holds dx_i/dq_2k, dx_i/dq_2k+1 (k = i/2), Ja, Jb (n): dx_i/dl_n_k, dx_i/dmu_k.
// work: newton_jac_work_doubles.  -> status (of M and the inputs alone: the same whatever is requested)
template <int KIND>
DQQ_HD int newton_jac_problem(const double* P, bool diag, const double* q, const double* a, const double* b, const double* c,
                              const double* x, double* Jq, double* Ja, double* Jb, int n, double* work,
                              bool inf_ok = false, double reg = 0.0)
{
#pragma clang fp contract(off)
    double* M = work;
    double* z = M + (long)n * n;
    double* F = z + n;
    double* dj = F + n;
    double* R = z + newton_vec_doubles(n);
    const int ne = newton_jac_extra_cols(KIND, n);
    double* const out[3] = {Jq, KIND == 0 ? nullptr : Ja, KIND == 0 ? nullptr : Jb};
    const bool bad = polish_inputs_bad<KIND>(P, diag, q, a, b, c, x, n, inf_ok);
    bool ok = !bad;
    if (ok) {
        polish_eval<KIND>(P, diag, q, a, b, c, x, n, z, F, dj);
        if (diag) {
            for (int k = 0; k < n / 2 && KIND == 1; ++k) {
                double m[4];
                newton_contact_block(dj + 3 * k, polish_reg(P[2 * k], reg), polish_reg(P[2 * k + 1], reg), m);
                for (int col = 0; col < 4; ++col) {   // q_2k, q_2k+1, l_n_k, mu_k
                    const int which = col < 2 ? 0 : col - 1, j = col < 2 ? 2 * k + col : k;
                    double d0 = newton_jac_rhs<KIND>(z, dj, a, b, c, 2 * k, which, j);
                    double d1 = newton_jac_rhs<KIND>(z, dj, a, b, c, 2 * k + 1, which, j);
                    ok = polish_solve2(m[0], m[1], m[2], m[3], d0, d1) && ok;
                    if (col < 2 && Jq != nullptr) { Jq[2 * (2 * k) + col] = d0; Jq[2 * (2 * k + 1) + col] = d1; }
                    if (col >= 2 && out[which] != nullptr) { out[which][2 * k] = d0; out[which][2 * k + 1] = d1; }
                }
            }
            for (int i = 0; i < n && KIND != 1; ++i)
                for (int which = 0; which < (KIND == 0 ? 1 : 3); ++which) {
                    double d = newton_jac_rhs<KIND>(z, dj, a, b, c, i, which, i);
                    ok = polish_solve1(dj[i] != 0.0 ? polish_reg(P[i], reg) : 1.0, d) && ok;
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
                            R[(long)i * ncol + off[which] + j] = newton_jac_rhs<KIND>(z, dj, a, b, c, i, which, j);
            newton_matrix<KIND>(P, dj, n, false, M, reg);
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

// The reverse-mode derivative of one problem.  gP ((n,n); diag: n), gq, ga, gb: NULL = not requested.  -> status
template <int KIND>
DQQ_HD int newton_bwd_problem(const double* P, bool diag, const double* q, const double* a, const double* b, const double* c,
                              const double* x, const double* gx, double* gP, double* gq, double* ga, double* gb, int n, double* work,
                              bool inf_ok = false, double reg = 0.0)
{
#pragma clang fp contract(off)
    double* M = work;
    double* z = M + (long)n * n;
    double* F = z + n;
    double* dj = F + n;
    double* w = dj + 2 * n;
    double* v = w + n;
    const int ne = KIND == 0 ? 0 : (KIND == 1 ? n / 2 : n);
    const bool bad = polish_inputs_bad<KIND>(P, diag, q, a, b, c, x, n, inf_ok) || newton_vec_bad(gx, n);
    bool ok = !bad;
    if (ok) {
        polish_eval<KIND>(P, diag, q, a, b, c, x, n, z, F, dj);
        for (int i = 0; i < n; ++i) w[i] = gx[i];
        if (diag) {
            if (KIND == 1) {
                for (int k = 0; k < n / 2; ++k) {
                    double m[4];
                    newton_contact_block(dj + 3 * k, polish_reg(P[2 * k], reg), polish_reg(P[2 * k + 1], reg), m);
                    ok = polish_solve2(m[0], m[2], m[1], m[3], w[2 * k], w[2 * k + 1]) && ok;
                }
            } else {
                for (int i = 0; i < n; ++i) ok = polish_solve1(dj[i] != 0.0 ? polish_reg(P[i], reg) : 1.0, w[i]) && ok;
            }
        } else {
            newton_matrix<KIND>(P, dj, n, true, M, reg);
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
            const double* D = dj + 3 * k;
            v[2 * k] = newton_contact_v(D[0], D[1], w[2 * k], w[2 * k + 1]);
            v[2 * k + 1] = newton_contact_v(D[1], D[2], w[2 * k], w[2 * k + 1]);
            double ua, ub;
            const bool on = newton_disc_u(z[2 * k], z[2 * k + 1], a[k] * b[k], ua, ub);
            const double t = newton_contact_t(ua, ub, w[2 * k], w[2 * k + 1]);
            if (ga != nullptr) ga[k] = on ? newton_mul(b[k], t) : 0.0;
            if (gb != nullptr) gb[k] = on ? newton_mul(a[k], t) : 0.0;
        }
    } else {
        for (int i = 0; i < n; ++i) {
            const int st = newton_box_state<KIND>(z[i], KIND >= 2 ? a[i] : 0.0, KIND >= 2 ? b[i] : 0.0, KIND == 3 ? c[i] : 0.0);
            v[i] = st == kNewtonFree ? w[i] : 0.0;
            if (KIND >= 2 && ga != nullptr) ga[i] = st == kNewtonLo ? w[i] : 0.0;
            if (KIND >= 2 && gb != nullptr) gb[i] = st == kNewtonHi ? w[i] : 0.0;
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
