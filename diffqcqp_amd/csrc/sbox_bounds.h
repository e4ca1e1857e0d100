// sbox_bounds.h -- the signed box QP as a box QP on other bounds: the one place the table is written down.
//
// Per coordinate, with s = sign(v), the signed forward's projection (Solver.cpp:395-398) is
//   t -> s * min(s * clamp(t, lo, hi), 0)
// and for lo <= hi that is clamp(t, lo', hi') with
//   s > 0:  hi' = min(hi, 0),  lo' = min(lo, hi')
//   s < 0:  lo' = max(lo, 0),  hi' = max(hi, lo')
//   s = 0:  lo' = hi' = 0                                (v = +0.0, v = -0.0; a NaN v has no sign either)
// The second min / max covers the combinations the sign constraint makes infeasible (lo > 0 with s > 0, hi < 0 with
// s < 0), where the forward returns 0.  min and max select one of their arguments: nothing is rounded.
//
// The signed box backward IS the box backward at (lo', hi') -- same active-set tests, same refinement loops, same
// exits.  What differs is where the bound gradients go: grad_l_min receives the lower multiplier's term only where the
// effective lower bound is still l_min (keep_lo: lo' == lo as VALUES, so -0.0 == +0.0), grad_l_max alike (keep_hi);
// elsewhere the bound the solution sits on is the sign constraint's 0, a constant, and the gradient is +0.0.  A tie
// (l_min == 0 with s < 0, l_max == 0 with s > 0, either bound == 0 with s = 0) passes the gradient to the bound: a
// subgradient choice.  No gradient flows to v: x is piecewise constant in it.
//
// Selects only, no arithmetic; contraction is switched off anyway so that host and device builds cannot differ.
#pragma once

#include "common.h"

namespace dqq {

struct SBoxBounds {
    double lo, hi;          // the effective bounds lo', hi'
    bool keep_lo, keep_hi;  // lo' == l_min / hi' == l_max: the bound gradient belongs to the caller's bound
};

DQQ_HD SBoxBounds sbox_bounds(double lo, double hi, double v)
{
#pragma clang fp contract(off)
    const bool pos = v > 0, neg = v < 0;
    const double hi_p = hi < 0 ? hi : 0.0;          // s > 0: min(hi, 0)
    const double lo_p = lo < hi_p ? lo : hi_p;      //        min(lo, hi')
    const double lo_n = lo > 0 ? lo : 0.0;          // s < 0: max(lo, 0)
    const double hi_n = hi > lo_n ? hi : lo_n;      //        max(hi, lo')
    SBoxBounds b;
    b.lo = pos ? lo_p : (neg ? lo_n : 0.0);
    b.hi = pos ? hi_p : (neg ? hi_n : 0.0);
    b.keep_lo = b.lo == lo;
    b.keep_hi = b.hi == hi;
    return b;
}

} // namespace dqq
