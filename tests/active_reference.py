"""The active-set report (dqq_newton_active_f64) restated in numpy: the definition of diffqcqp_amd/csrc/active_core.h a second
time, operation by operation, on top of tests/polish_reference.py (z is the polish's evaluate) and tests/newton_reference.py (the
box-like state is box_state), so that the host core (tests/hostcore/active_core_check.cpp) and through it the kernels can be held
to its bits.  Not a test file.

Per problem, float64, P always the full (n,n) matrix here (a diagonal P is a matrix with zeros).  An element is a coordinate, or
a contact of the QCQP:
  state   box-like: 0 free, 1 on the caller's lower bound, 2 on the caller's upper bound, 3 on a constant;
          contact: 0 inside the disc, 1 outside with rad > 0, 3 outside with rad <= 0
  mult    box-like: +0.0 free, lo - z where z <= lo (first), z - hi where z >= hi;  contact: +0.0 inside, else nrm - rad if
          rad > 0, else nrm
  margin  the first smallest in index order of  min(|z - lo|, |z - hi|)  /  |nrm - rad| if rad > 0 else nrm;  where: its index
  status  2 if an input (the flag's rule for infinite bounds: inf_bounds_reference.inputs_bad) or a z_i is not finite, else 0;
          with 2: state, where = -1, mult, margin = NaN
numpy's elementwise float64 arithmetic rounds every operation; the one fused multiply-add (the squared norm of a contact's z) is
taken exactly with fractions, as polish_reference does."""
import numpy as np

import inf_bounds_reference as IR
import newton_reference as NR
import polish_reference as R

NAN = float("nan")


def elements(kind, n):
    return n // 2 if kind == "qcqp" else n


def contact(za, zb, rad):
    """-> (state, mult, e) of a contact."""
    n2 = R.fma(zb, zb, za * za)
    nrm = float(np.sqrt(n2))
    outside, pos = n2 > rad * abs(rad), rad > 0.0
    state = 0 if not outside else (1 if pos else 3)
    mult = 0.0 if not outside else (nrm - rad if pos else nrm)
    return state, mult, (abs(nrm - rad) if pos else nrm)


def active(kind, P, q, ex, x, flag=False):
    """One problem.  P (n,n), q (n), ex the kind's extras, x (n) -> (state (ne) int32, mult (ne), margin, where, status)."""
    with np.errstate(all="ignore"):
        n = x.shape[0]
        ne = elements(kind, n)
        ex = tuple(np.asarray(e, dtype=np.float64).reshape(-1) for e in ex)
        bad = IR.inputs_bad(kind, P, q, ex, x, flag=flag)
        z = R.evaluate(kind, P, q, ex, x)[0] if not bad else None
        if bad or not np.isfinite(z).all():
            return np.full(ne, -1, dtype=np.int32), np.full(ne, NAN), NAN, -1, 2
        if kind == "qcqp":
            rows = [contact(float(z[2 * k]), float(z[2 * k + 1]), float(ex[0][k]) * float(ex[1][k])) for k in range(ne)]
            state = np.array([r[0] for r in rows], dtype=np.int32)
            mult, e = np.array([r[1] for r in rows]), np.array([r[2] for r in rows])
        else:
            lo, hi = R.effective_bounds(kind, ex, n)
            state = NR.box_state(kind, z, ex, n).astype(np.int32)
            free = (lo < z) & (z < hi)
            at_lo = ~free & (z <= lo)
            at_hi = ~free & ~at_lo & (z >= hi)
            mult = np.where(at_lo, lo - z, np.where(at_hi, z - hi, 0.0))
            t_lo, t_hi = np.abs(z - lo), np.abs(z - hi)
            e = np.where(t_hi < t_lo, t_hi, t_lo)
        where, margin = 0, float(e[0])
        for k in range(1, ne):
            if e[k] < margin:
                where, margin = k, float(e[k])
        return state, mult, margin, where, 0


def active_batch(kind, P, q, ex, x, flag=False):
    """P (B,n,n), q, x (B,n), ex each (B,.) -> state (B,ne) int32, mult (B,ne), margin (B), where (B) int32, status (B) int32"""
    B, n = x.shape
    ne = elements(kind, n)
    state, mult = np.empty((B, ne), dtype=np.int32), np.empty((B, ne))
    margin, where, status = np.empty(B), np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32)
    for b in range(B):
        state[b], mult[b], margin[b], where[b], status[b] = active(kind, P[b], q[b], tuple(e[b] for e in ex), x[b], flag)
    return state, mult, margin, where, status
