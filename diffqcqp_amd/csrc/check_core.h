// check_core.h -- the arithmetic of the solution check (dqq_check_f64, check.hip), host/device: what a lane adds up for its
// columns of a row of P, what a coordinate (a contact, for the QCQP) contributes to the four residual scalars, how the lanes of
// a problem merge, and the status word.  check.hip runs it on L = 1 .. 64 lanes per problem with DPP between them;
// tests/hostcore/check_core_check.cpp runs the same functions over an array of L "lanes" on the CPU, which must give the
// same bits (every fused multiply-add is written out and no other may be formed, as in admm_diag_body.inc).
//
// Per problem, float64 (include/diffqcqp_hip.h has the definitions):  g = P x + q,  PI = projection onto the kind's set,
//   resid[0] = max |x - PI(x - g)|   resid[1] = max |x - PI(x)|   resid[2] = 1/2 x'Px + q'x   resid[3] = max(max |P||x|, max |q|)
//
// Order of evaluation (a function of N and the layout alone).  W = 2 columns per lane for even N, 1 for odd N;
// L = min(64, 2^ceil(log2(N / W))) lanes per problem; lane j owns the columns c with (c mod L W) / W = j.
//   row sums      s_i = sum_c P_ic x_c and a_i = sum_c |P_ic| |x_c|: each lane over its columns in increasing order (fma chain
//                 from 0), then the tree v_j + v_(j xor 1), (j xor 2), ... over the L lanes (every lane ends with the same bits);
//   coordinates   the lane that owns column i evaluates row i's terms (check_coord / check_contact) into its own CheckAcc, rows
//                 in increasing order;
//   merge         the maxima by the same tree with nmax, the objective by the same tree with +.
// DQQ_P_DIAG: s_i = fma(p_i, x_i, 0), a_i = fma(|p_i|, |x_i|, 0), no row tree; the rest alike.
#pragma once

#include "common.h"
#include "route.h"   // check_lanes, check_cols_per_lane

namespace dqq {

struct CheckAcc {
    double nat, inf, obj, scl, xmx;   // resid[0..3] and max |x| (for the status only)
    DQQ_HD void init() { nat = inf = obj = scl = xmx = 0.0; }
};

// max(m, |v|) that keeps a NaN from either side (fmax and v_max_f64 drop it): a NaN anywhere must reach the status
DQQ_HD double nmax(double m, double v)
{
    v = fabs(v);
    return (v > m || v != v) ? v : m;
}

// a lane's W adjacent columns of one row: s += p x, a += |p| |x|, in column order
template <int W>
DQQ_HD void check_row_terms(const double (&p)[W], const double (&x)[W], double& s, double& ab)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int w = 0; w < W; ++w) {
        s = __builtin_fma(p[w], x[w], s);
        ab = __builtin_fma(fabs(p[w]), fabs(x[w]), ab);
    }
}

// The projections.  Written with selects that pass a NaN argument through (fmax would return the bound).
// KIND 0: max(t, 0);  2: clamp to [lo, hi];  3: the clamp, then sg min(sg t, 0) (admm_diag_body.inc, KIND 3)
template <int KIND>
DQQ_HD double check_proj(double t, double lo, double hi, double sg)
{
#pragma clang fp contract(off)
    if (KIND == 0) return t < 0.0 ? 0.0 : t;
    t = t < lo ? lo : t;
    t = hi < t ? hi : t;
    if (KIND == 3) {
        double m = sg * t;
        m = 0.0 < m ? 0.0 : m;
        t = sg * m;
    }
    return t;
}

// KIND 1: a contact (a, b) onto the disc of radius rad = l_n mu, tested on the squares as prox_circle is
DQQ_HD void check_proj_circle(double& a, double& b, double rad)
{
#pragma clang fp contract(off)
    const double n2 = __builtin_fma(b, b, a * a);
    if (n2 > rad * fabs(rad)) {
        const double sc = rad / sqrt(n2);
        a = a * sc;
        b = b * sc;
    }
}

// what coordinate i adds besides the projections: x_i (s_i / 2 + q_i), max(a_i, |q_i|), |x_i|
DQQ_HD void check_common(CheckAcc& c, double x, double s, double ab, double q)
{
#pragma clang fp contract(off)
    c.obj = __builtin_fma(x, __builtin_fma(0.5, s, q), c.obj);
    c.scl = nmax(nmax(c.scl, ab), q);
    c.xmx = nmax(c.xmx, x);
}

template <int KIND>
DQQ_HD void check_coord(CheckAcc& c, double x, double s, double ab, double q, double lo, double hi, double sg)
{
#pragma clang fp contract(off)
    const double g = s + q;
    c.nat = nmax(c.nat, x - check_proj<KIND>(x - g, lo, hi, sg));
    c.inf = nmax(c.inf, x - check_proj<KIND>(x, lo, hi, sg));
    check_common(c, x, s, ab, q);
}

DQQ_HD void check_contact(CheckAcc& c, const double (&x)[2], const double (&s)[2], const double (&ab)[2],
                          const double (&q)[2], double rad)
{
#pragma clang fp contract(off)
    double ta = x[0] - (s[0] + q[0]), tb = x[1] - (s[1] + q[1]);
    check_proj_circle(ta, tb, rad);
    c.nat = nmax(nmax(c.nat, x[0] - ta), x[1] - tb);
    double pa = x[0], pb = x[1];
    check_proj_circle(pa, pb, rad);
    c.inf = nmax(nmax(c.inf, x[0] - pa), x[1] - pb);
    check_common(c, x[0], s[0], ab[0], q[0]);
    check_common(c, x[1], s[1], ab[1], q[1]);
}

// one level of the merge: this lane's sums with its partner's (the partner does the same with the roles swapped)
DQQ_HD void check_merge(CheckAcc& c, const CheckAcc& o)
{
#pragma clang fp contract(off)
    c.nat = nmax(c.nat, o.nat);
    c.inf = nmax(c.inf, o.inf);
    c.scl = nmax(c.scl, o.scl);
    c.xmx = nmax(c.xmx, o.xmx);
    c.obj = c.obj + o.obj;
}

// 2: an entry of x or of resid is not finite;  1: the solve stopped at max_iter (iters given);  0 otherwise
DQQ_HD int check_status(const CheckAcc& c, bool has_iters, int iters, int max_iter)
{
    const bool finite = __builtin_isfinite(c.nat) && __builtin_isfinite(c.inf) && __builtin_isfinite(c.obj) &&
                        __builtin_isfinite(c.scl) && __builtin_isfinite(c.xmx);
    if (!finite) return 2;
    return (has_iters && iters >= max_iter) ? 1 : 0;
}

DQQ_HD double check_sign(double v) { return (double)((v > 0) - (v < 0)); }

} // namespace dqq
