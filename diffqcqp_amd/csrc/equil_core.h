// equil_core.h -- the arithmetic of the power-of-two equilibration (dqq_equilibrate_f64 / dqq_unscale_f64, equil.hip),
// host/device: the exponent of a coordinate from its diagonal entry of P, and what every array of the problem is multiplied by.
// Integer exponent arithmetic only -- frexp, compares, ldexp; no log2, no rounding of a mantissa -- so the host
// (tests/hostcore/equil_core_check.cpp), the device and the numpy restatement (tests/equil_ref.py: np.frexp, np.ldexp) give the
// same bits, and the scaled problem is the caller's problem in other units, not an approximation of it.
//
// The scaling.  D = diag(2^e_i), x = D y:   P~ = D P D,  q~ = D q,  bounds l~ = D^-1 l,  start y0 = D^-1 x0;  back: x = D y.
//
// The exponent of coordinate i:  e_i = -round_half_even(log2(P_ii) / 2), so that P~_ii = P_ii 2^(2 e_i) lies in [1/2, 2].
// The rule, exactly.  Let P_ii = m 2^k with m in [1/2, 1) (frexp) and n = round_half_even(log2(P_ii) / 2); log2(P_ii) lies in
// [k - 1, k).  n is the integer nearest to log2(P_ii) / 2, i.e. the one with |log2(P_ii) - 2 n| <= 1:
//     k odd,  k = 2 h + 1:   log2 in [2 h, 2 h + 1)      n = h
//     k even, k = 2 h:       log2 in [2 h - 1, 2 h)      n = h, but at log2 = 2 h - 1 exactly (m == 1/2: P_ii = 2^(2 h - 1), an
//                            odd power of two) h - 1 and h are equally near: the even one of the two
// so n = floor(k / 2), one less where m == 1/2, k is even and floor(k / 2) is odd; e_i = -n.  The only mantissa that is looked
// at is 1/2: the half-way points of log2(P_ii) / 2 are the odd powers of two and nothing else (a mantissa of sqrt(1/2) is the
// half-way point of log2(P_ii) itself, not of its half, and rounds like its neighbours: 2^(k - 1/2) has n = floor(k / 2)).
//     P_ii     1   2   1/2   4   8    1/8   3    2^40   2^-40
//     e_i      0   0   0    -1  -2    2    -1   -20     20
//     P~_ii    1   2   1/2   1   1/2  2    3/4   1      1
// e_i = 0 where P_ii is <= 0 (either zero included), a NaN or infinite: such a problem reaches the solver as it is.
// Clamp: |e_i| <= kEquilMaxExp = 255 (reached from 2^510 up and 2^-510 down, subnormals included), so e_i + e_j stays within
// +-510 and a positive semidefinite P, |P_ij| <= sqrt(P_ii P_jj), cannot overflow: |P~_ij| <= sqrt(P~_ii P~_jj), which is at
// most 2 where neither exponent was clamped, and P~_ii <= max(2, P_ii) always (a clamped negative exponent still shrinks).
//
// Per kind.  QP, box QP, signed box QP: a coordinate's exponent is its own.  QCQP: the two coordinates of a contact share one
// exponent, that of the larger of their two diagonal entries (pb > pa ? pb : pa -- a NaN in pb, or in both, leaves pa), so that
// the contact's disc stays a disc: |x_c| <= l_n mu  <=>  |y_c| <= (2^-e_c l_n) mu.
//     P~_ij = ldexp(P_ij, e_i + e_j)    DQQ_P_DIAG:  p~_i = ldexp(p_i, 2 e_i)
//     q~_i  = ldexp(q_i, e_i)
//     box kinds:  l~_min,i = ldexp(l_min,i, -e_i),  l~_max,i = ldexp(l_max,i, -e_i)   (+-inf stays +-inf);  v is passed through:
//                 sign(v_i) y_i <= 0  <=>  sign(v_i) x_i <= 0
//     QCQP:       l~_n,c = ldexp(l_n,c, -e_c),  mu unchanged
//     start:      y0_i = ldexp(x0_i, -e_i)
//     solution:   x_i = ldexp(y_i, e_i)
// Every ldexp is exact unless its result is subnormal or overflows (then it is the correctly rounded one, on host and device).
#pragma once

#include "common.h"

namespace dqq {

constexpr int kEquilMaxExp = 255;

DQQ_HD double equil_ldexp(double v, int e) { return __builtin_ldexp(v, e); }

// e_i from P_ii (the rule above)
DQQ_HD int equil_exp(double p)
{
    if (!(p > 0.0) || !(p <= 1.7976931348623157e308)) return 0;   // <= 0, NaN, +inf
    int k;
    const double m = __builtin_frexp(p, &k);   // p = m 2^k, m in [1/2, 1); subnormals included
    int n = k >> 1;                            // floor(k / 2)
    if (m == 0.5 && (k & 1) == 0 && (n & 1) != 0) n -= 1;
    const int e = -n;
    return e > kEquilMaxExp ? kEquilMaxExp : (e < -kEquilMaxExp ? -kEquilMaxExp : e);
}

// a QCQP contact (a, b): one exponent, from the larger diagonal entry
DQQ_HD int equil_exp_pair(double pa, double pb) { return equil_exp(pb > pa ? pb : pa); }

// the exponent of coordinate i of a problem whose diagonal is d(0 .. N-1)
template <int KIND, typename Diag>
DQQ_HD int equil_coord_exp(const Diag& d, int i)
{
    if constexpr (KIND == 1) return equil_exp_pair(d(i & ~1), d(i | 1));
    else return equil_exp(d(i));
}

DQQ_HD double equil_scale_p(double p, int ei, int ej) { return equil_ldexp(p, ei + ej); }   // P_ij; the compact p_i: ei = ej
DQQ_HD double equil_scale_q(double q, int e) { return equil_ldexp(q, e); }
DQQ_HD double equil_scale_bound(double l, int e) { return equil_ldexp(l, -e); }              // l_min, l_max, l_n and x0
DQQ_HD double equil_unscale(double y, int e) { return equil_ldexp(y, e); }

} // namespace dqq
