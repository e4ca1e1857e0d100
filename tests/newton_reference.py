"""The Newton derivatives (dqq_newton_bwd_f64, dqq_newton_jvp_f64) restated in numpy: the definition of
diffqcqp_amd/csrc/newton_core.h a second time, operation by operation, on top of tests/polish_reference.py (z, D, M and the
elimination are the polish's), so that the host core (tests/hostcore/newton_core_check.cpp) and through it the kernels can be
held to its bits.  Not a test file.

Per problem, float64, P always the full (n,n) matrix here (a diagonal P is a matrix with zeros), at the x given:
  M dx = -D (dP x + dq) + E dtheta                                                  (JVP;  a tangent None is a zero tangent)
  M' w = grad_x, v = D w, grad_q = -v, grad_P = -v x', grad_theta = E' w            (backward)
numpy's elementwise float64 arithmetic rounds every operation; the one fused multiply-add (the squared norm of a contact's z) is
taken exactly with fractions, as polish_reference does."""
import numpy as np

import polish_reference as R

NAN = float("nan")


def _finite(*arrays):
    return all(a is None or np.isfinite(a).all() for a in arrays)


def box_state(kind, z, ex, n):
    """Per coordinate: 0 free, 1 on the caller's lower bound, 2 on the caller's upper bound, 3 fixed on a constant."""
    lo, hi = R.effective_bounds(kind, ex, n)
    keep_lo = keep_hi = np.full(n, kind == "box")
    if kind == "sbox":
        keep_lo, keep_hi = lo == ex[0], hi == ex[1]
    free = (lo < z) & (z < hi)
    at_lo = ~free & (z <= lo)
    at_hi = ~free & ~at_lo & (z >= hi)
    return np.where(free, 0, np.where(at_lo & keep_lo, 1, np.where(at_hi & keep_hi, 2, 3)))


def disc_u(za, zb, rad):
    """-> (on, ua, ub) of a contact."""
    n2 = R.fma(zb, zb, za * za)
    if not n2 > rad * abs(rad) or not rad > 0.0:
        return False, 0.0, 0.0
    nrm = np.sqrt(n2)
    return True, za / nrm, zb / nrm


def _setup(kind, P, q, ex, x):
    n = x.shape[0]
    z, _, _ = R.evaluate(kind, P, q, ex, x)
    D = R.jacobian(kind, z, ex, n)
    return n, z, D, R.newton_matrix(kind, P, D)


def jvp(kind, P, q, ex, x, dP=None, dq=None, da=None, db=None):
    """One problem.  P (n,n), q (n), ex the kind's extras, x (n); tangents of their input's shape or None -> (dx (n), status)."""
    with np.errstate(all="ignore"):
        ex = tuple(np.asarray(e, dtype=np.float64).reshape(-1) for e in ex)
        n = x.shape[0]
        if not _finite(P, q, x, dP, dq, da, db, *ex):
            return np.full(n, NAN), 2
        n, z, D, M = _setup(kind, P, q, ex, x)
        s = np.zeros(n)
        if dP is not None:
            for j in range(n):
                s = s + dP[:, j] * x[j]
        t = s + (dq if dq is not None else 0.0)
        rhs = np.empty(n)
        if kind == "qcqp":
            for k in range(n // 2):
                ln, mu = float(ex[0][k]), float(ex[1][k])
                on, ua, ub = disc_u(float(z[2 * k]), float(z[2 * k + 1]), ln * mu)
                drad = mu * (float(da[k]) if da is not None else 0.0) + ln * (float(db[k]) if db is not None else 0.0)
                for r, u in ((2 * k, ua), (2 * k + 1, ub)):
                    w = D[r, 2 * k] * t[2 * k] + D[r, 2 * k + 1] * t[2 * k + 1]
                    rhs[r] = u * drad - w if on else -w
        else:
            st = box_state(kind, z, ex, n)
            dlo = da if da is not None and kind != "qp" else np.zeros(n)
            dhi = db if db is not None and kind != "qp" else np.zeros(n)
            rhs = np.where(st == 0, -t, np.where(st == 1, dlo, np.where(st == 2, dhi, 0.0)))
        dx = R.solve(M, rhs)
        return (np.full(n, NAN), 1) if dx is None else (dx, 0)


def backward(kind, P, q, ex, x, gx):
    """One problem -> (grad_P (n,n), grad_q (n), grad_a, grad_b (None for the QP), status)."""
    with np.errstate(all="ignore"):
        ex = tuple(np.asarray(e, dtype=np.float64).reshape(-1) for e in ex)
        n = x.shape[0]
        ne = 0 if kind == "qp" else (n // 2 if kind == "qcqp" else n)
        status = 0
        w = None
        if not _finite(P, q, x, gx, *ex):
            status = 2
        else:
            n, z, D, M = _setup(kind, P, q, ex, x)
            w = R.solve(np.ascontiguousarray(M.T), gx)
            if w is None:
                status = 1
        if status:
            g = (np.full((n, n), NAN), np.full(n, NAN))
            return g + ((None, None) if kind == "qp" else (np.full(ne, NAN), np.full(ne, NAN))) + (status,)
        ga = gb = None
        if kind == "qcqp":
            v, ga, gb = np.empty(n), np.zeros(ne), np.zeros(ne)
            for k in range(n // 2):
                ln, mu = float(ex[0][k]), float(ex[1][k])
                wa, wb = w[2 * k], w[2 * k + 1]
                v[2 * k] = D[2 * k, 2 * k] * wa + D[2 * k, 2 * k + 1] * wb
                v[2 * k + 1] = D[2 * k + 1, 2 * k] * wa + D[2 * k + 1, 2 * k + 1] * wb
                on, ua, ub = disc_u(float(z[2 * k]), float(z[2 * k + 1]), ln * mu)
                if on:
                    t = ua * wa + ub * wb
                    ga[k], gb[k] = mu * t, ln * t
        else:
            st = box_state(kind, z, ex, n)
            v = np.where(st == 0, w, 0.0)
            if kind != "qp":
                ga, gb = np.where(st == 1, w, 0.0), np.where(st == 2, w, 0.0)
        return -(v[:, None] * x[None, :]), -v, ga, gb, 0


def jvp_batch(kind, P, q, ex, x, dP=None, dq=None, da=None, db=None):
    """P (B,n,n), q, x (B,n), ex each (B,.), tangents batched or None -> dx (B,n), status (B) int32"""
    B, n = x.shape
    dx, st = np.empty((B, n)), np.empty(B, dtype=np.int32)
    pick = lambda a, b: None if a is None else a[b]
    for b in range(B):
        dx[b], st[b] = jvp(kind, P[b], q[b], tuple(e[b] for e in ex), x[b], pick(dP, b), pick(dq, b), pick(da, b), pick(db, b))
    return dx, st


def backward_batch(kind, P, q, ex, x, gx):
    """-> grad_P (B,n,n), grad_q (B,n), grad_a, grad_b (B,.) or None, status (B) int32"""
    B, n = x.shape
    ne = 0 if kind == "qp" else (n // 2 if kind == "qcqp" else n)
    gP, gq, st = np.empty((B, n, n)), np.empty((B, n)), np.empty(B, dtype=np.int32)
    ga, gb = (None, None) if kind == "qp" else (np.empty((B, ne)), np.empty((B, ne)))
    for b in range(B):
        r = backward(kind, P[b], q[b], tuple(e[b] for e in ex), x[b], gx[b])
        gP[b], gq[b], st[b] = r[0], r[1], r[4]
        if ga is not None:
            ga[b], gb[b] = r[2], r[3]
    return gP, gq, ga, gb, st
