// bwd_systems.h -- how every implicit-function backward STARTS, stated once: the duals recovered from the primal
// solution, the active sets, and the entries of the matrix and right-hand side handed to iterative_refinement.
//
//   QP     pybindings.cpp:24-30 -> Solver::dualFromPrimalQP (Solver.cpp:125-134): gamma = -(P l + q), zeroed where
//          l_i > epsilon; solveDerivativesQP (:136-196): active where gamma < -1e-10 (:139-147),
//          A = [[diag(l_A), 0],[0, P_II]] in the order (active..., inactive...) (:148-174), b = [0; grad_I] (:175-184).
//   QCQP   pybindings.cpp:62-71 -> dualFromPrimalQCQP (:584-617): r = l_n mu (pybindings.cpp:65), slack (:594-597), the
//          test (:598-604), gamma = -(A~^T A~)^-1 A~^T (P l + q) by llt().solve (:605-615); solveDerivativesQCQP
//          (:619-681): S = -r^2 + |l_c|^2 (:622-629), active where S > -1e-10 and r > 1e-10 (:637-641),
//          A = [[diag(S_act), (diag(gamma) C^T)_act],[C_act, P + blkdiag(2 gamma I2)]] (:643-657), b = [0; grad_l] (:659-667)
//   box    pybindings.cpp:39-45 -> dualFromPrimalBoxQP (:263-308): not_null lists (:268-283; lower before upper,
//          coordinate by coordinate), gamma_not_null = iterative_refinement(Id2, -P l - q) (:291-304);
//          solveDerivativesBoxQP (:310-371): A = [[0, B],[Id2, P]], B.row(j) = gamma_j Id2.col(j)^T (:341-350),
//          b = [0; grad_l] (:352-360).  The signed box QP is the box QP on the bounds of sbox_bounds.h.
// iterative_refinement receives A^T (transposeInPlace, :174 / :657 / :351): *_At return entry (rr, cc) of it, A[cc][rr].
// Host/device, no memory access other than through the arguments, no lane or thread notion: the kernels keep their own
// data flow (ballots, LDS staging, tiles) around these calls, and tests/hostcore/bwd_systems_check.cpp runs the same text
// on one CPU thread against the oracle.  FP contraction is off in every function: the operation order is the reference's.
#pragma once

#include "common.h"

namespace dqq {

// unknowns of the largest derivative system of a kind: N (QP), N + N/2 (QCQP), 3N (box kinds)
DQQ_HD constexpr int bwd_system_rows(int kind, int n) { return kind == 0 ? n : (kind >= 2 ? 3 * n : n + n / 2); }

// ------------------------------------------------------------------ QP
// plq_i = (P l + q)_i
DQQ_HD double qp_dual(double plq_i, double x_i, double eps)
{
#pragma clang fp contract(off)
    double gamma = -plq_i;
    if (x_i > eps) gamma = 0;
    return gamma;
}
DQQ_HD bool qp_active(double gamma)
{
#pragma clang fp contract(off)
    return gamma < -kActiveEps;
}
// perm: position -> coordinate, the na active ones first; xv = l; Pl = P with row stride ld
DQQ_HD double qp_system_At(int rr, int cc, int na, const int* perm, const double* xv, const double* Pl, int ld)
{
#pragma clang fp contract(off)
    if (cc < na || rr < na) return (cc == rr) ? xv[perm[cc]] : 0.0;
    return Pl[perm[cc] * ld + perm[rr]];
}
DQQ_HD double qp_system_rhs(int p, int na, const int* perm, const double* g)
{
#pragma clang fp contract(off)
    return (p < na) ? 0.0 : g[perm[p]];
}

// ------------------------------------------------------------------ QCQP
// gamma: dual of the contact (0 when the dual recovery finds it inactive); S: its diagonal entry of A; act: in the
// DERIVATIVE system's active set -- not the dual recovery's test
struct QcqpDual { double gamma, S; bool act; };
// the derivative system's active test on a contact's S and r = l_n mu
DQQ_HD bool qcqp_active(double S, double r)
{
#pragma clang fp contract(off)
    return S > -kActiveEps && r > kActiveEps;
}
// one contact: (xa, xb) = l_2c, l_2c+1, (pla, plb) = (P l + q) at the same coordinates
DQQ_HD QcqpDual qcqp_contact(double xa, double xb, double pla, double plb, double l_n, double mu, double eps)
{
#pragma clang fp contract(off)
    QcqpDual d;
    const double r = l_n * mu;
    const double slack = r + -sqrt(xa * xa + xb * xb);
    d.gamma = 0.0;
    if (!(slack > eps || r < eps)) {
        const double ca = 2 * xa, cb = 2 * xb;         // A~(2i,i), A~(2i+1,i)
        const double G = ca * ca + cb * cb;            // A~^T A~ (diagonal)
        const double rhs = ca * pla + cb * plb;        // A~^T (P l + q)
        const double L = sqrt(G);                      // llt().solve
        d.gamma = -((rhs / L) / L);
    }
    d.S = -(r * r);
    d.S = d.S + (xa * xa + xb * xb);
    d.act = qcqp_active(d.S, r);
    return d;
}

// perm: active slot -> contact (na of them); S, gam per contact; xv = l
DQQ_HD double qcqp_system_At(int rr, int cc, int na, const int* perm, const double* S, const double* gam,
                             const double* xv, const double* Pl, int ld)
{
#pragma clang fp contract(off)
    const int row = cc, col = rr;
    if (row < na) {
        const int cid = perm[row];
        if (col < na) return (col == row) ? S[cid] : 0.0;
        const int i = col - na;
        return (i / 2 == cid) ? gam[cid] * (2 * xv[i]) : 0.0;
    }
    const int i = row - na;
    if (col < na) return (i / 2 == perm[col]) ? 2 * xv[i] : 0.0;
    const int jj = col - na;
    const double d = (i == jj) ? 2 * gam[i / 2] : 0.0;
    return d + Pl[i * ld + jj];
}
// b = [0; grad_l] of the QCQP and box systems: nm multiplier rows in front of the n coordinate rows
DQQ_HD double system_rhs(int p, int nm, const double* g)
{
#pragma clang fp contract(off)
    return (p < nm) ? 0.0 : g[p - nm];
}

// ------------------------------------------------------------------ box QP
struct BoxNotNull { bool aL, aU; };   // the lower / upper multiplier of the coordinate exists
DQQ_HD BoxNotNull box_not_null(double x, double lo, double hi, double eps)
{
#pragma clang fp contract(off)
    return {!(x - lo > eps), !(x - hi < -eps)};
}
// Id2(i, .) in the column of multiplier id (id < n: lower bound of coordinate id, else upper bound of id - n)
DQQ_HD double box_id2(int id, int i, int n)
{
#pragma clang fp contract(off)
    return (id < n) ? ((id == i) ? -1.0 : 0.0) : ((id - n == i) ? 1.0 : 0.0);
}
// the dual recovery's n x nn system: At[i][p] = Id2(i, p); nnl: not_null position -> multiplier id
DQQ_HD double box_dual_At(int i, int p, const int* nnl, int n)
{
#pragma clang fp contract(off)
    return box_id2(nnl[p], i, n);
}
// its right-hand side (-P l - q)_i; Prow = row i of P
DQQ_HD double box_dual_rhs(const double* Prow, const double* xv, int n, double q_i)
{
#pragma clang fp contract(off)
    double rhs = 0.0;
    for (int j = 0; j < n; ++j) rhs += (-Prow[j]) * xv[j];
    return rhs - q_i;
}

// gam: 2n multipliers, scattered by id
DQQ_HD double box_system_At(int rr, int cc, int nn, const int* nnl, const double* gam, const double* Pl, int ld, int n)
{
#pragma clang fp contract(off)
    const int row = cc, col = rr;
    if (row < nn) {
        if (col < nn) return 0.0;
        const int id = nnl[row];
        return gam[id] * box_id2(id, col - nn, n);
    }
    const int i = row - nn;
    if (col < nn) return box_id2(nnl[col], i, n);
    return Pl[i * ld + (col - nn)];   // right-hand side: system_rhs
}

// ------------------------------------------------------------------ forward mode (dqq_jvp_f64)
// The backward is g -> R(b), b = iterative_refinement(At, rhs(g)), with R the gradient assembly of the kernels: grad_q = -dl,
// grad_P = -dl x^T, QCQP grad_l_n = E2 dgamma, grad_mu = E1 dgamma, box grad_l_min = -dgamma_lo gamma_lo, grad_l_max =
// dgamma_hi gamma_hi.  The JVP is its transpose: s = R^T(tangents), w = iterative_refinement(At^T, s), dx = rhs^T(w).
// *_system_A: entry (rr, cc) of the matrix the refinement receives then, At^T; *_jvp_*: the entries of s; jvp_dx_*: rhs^T.
DQQ_HD double qp_system_A(int rr, int cc, int na, const int* perm, const double* xv, const double* Pl, int ld)
{
    return qp_system_At(cc, rr, na, perm, xv, Pl, ld);
}
DQQ_HD double qcqp_system_A(int rr, int cc, int na, const int* perm, const double* S, const double* gam, const double* xv,
                            const double* Pl, int ld)
{
    return qcqp_system_At(cc, rr, na, perm, S, gam, xv, Pl, ld);
}
DQQ_HD double box_system_A(int rr, int cc, int nn, const int* nnl, const double* gam, const double* Pl, int ld, int n)
{
    return box_system_At(cc, rr, nn, nnl, gam, Pl, ld, n);
}
// a coordinate row of s, from grad_q = -dl and grad_P = -dl x^T: dPx_i = (dP x)_i, dP full, summed in index order
DQQ_HD double jvp_coord(double dPx_i, double dq_i)
{
#pragma clang fp contract(off)
    return -(dPx_i + dq_i);
}
// QP: s in the order (active..., inactive...), t[i] = jvp_coord of coordinate i; dx_perm[p] = jvp_dx_qp(p, na, w_p)
DQQ_HD double qp_jvp_s(int p, int na, const int* perm, const double* t)
{
#pragma clang fp contract(off)
    return (p < na) ? 0.0 : t[perm[p]];
}
DQQ_HD double jvp_dx_qp(int p, int na, double w_p)
{
#pragma clang fp contract(off)
    return (p < na) ? 0.0 : w_p;
}
// QCQP: the row of an active contact, e2 / e1 = getE12QCQP of the contact (kkt_core.h: QcqpContact::e2, e1)
DQQ_HD double qcqp_jvp_mult(double e2, double dl_n, double e1, double dmu)
{
#pragma clang fp contract(off)
    return e2 * dl_n + e1 * dmu;
}
// box kinds: the row of multiplier id; gam scattered by id; dlo, dhi: the bound tangents of the multiplier's coordinate (the
// signed box QP passes 0.0 where sbox_bounds.h does not keep the bound)
DQQ_HD double box_jvp_mult(int id, int n, const double* gam, double dlo, double dhi)
{
#pragma clang fp contract(off)
    return (id < n) ? -(dlo * gam[id]) : dhi * gam[id];
}
// QCQP and box kinds: s = [multiplier rows (nm); coordinate rows], dx_i = w[nm + i]
DQQ_HD double system_jvp_s(int p, int nm, const double* sm, const double* t)
{
#pragma clang fp contract(off)
    return (p < nm) ? sm[p] : t[p - nm];
}

} // namespace dqq
