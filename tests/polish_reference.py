"""The polish (dqq_polish_f64) restated in numpy: the definition of diffqcqp_amd/csrc/polish_core.h a second time, operation
by operation, so that the host core (tests/hostcore/polish_core_check.cpp) and through it the kernels can be held to its bits.
Not a test file.

Per problem, float64, P always the full (n,n) matrix here (a diagonal P is a matrix with zeros):
  g = P x + q (row sums from 0 in index order, every product and sum rounded),  z = x - g,  F = x - PI(z),  r = max |F|
  D = generalised Jacobian of PI at z,  M = (I - D) + D P,  M d = -F by Gaussian elimination with partial pivoting (first
  largest |entry|; rows whose multiplier is an exact zero are left alone, back substitution by columns),  x+ = PI(x + d),
  accepted iff r+ < r; stop at r == 0, at a failed or rejected step, or after max_steps accepted steps.
numpy's elementwise float64 arithmetic rounds every operation; the one fused multiply-add of the definition (the squared norm
of check_proj_circle) is taken exactly with fractions."""
from fractions import Fraction

import numpy as np

KIND = {"qp": 0, "qcqp": 1, "box": 2, "sbox": 3}
INF = float("inf")


def fma(a, b, c):
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def effective_bounds(kind, ex, n):
    """-> (lo, hi) of the box-like kinds (csrc/sbox_bounds.h for the signed box)."""
    if kind == "qp":
        return np.zeros(n), np.full(n, INF)
    lo, hi = np.asarray(ex[0], dtype=np.float64).reshape(n), np.asarray(ex[1], dtype=np.float64).reshape(n)
    if kind == "box":
        return lo, hi
    v = np.asarray(ex[2], dtype=np.float64).reshape(n)
    hi_p = np.where(hi < 0, hi, 0.0)
    lo_p = np.where(lo < hi_p, lo, hi_p)
    lo_n = np.where(lo > 0, lo, 0.0)
    hi_n = np.where(hi > lo_n, hi, lo_n)
    return (np.where(v > 0, lo_p, np.where(v < 0, lo_n, 0.0)), np.where(v > 0, hi_p, np.where(v < 0, hi_n, 0.0)))


def proj_box(kind, t, lo, hi):
    if kind == "qp":
        return np.where(t < 0.0, 0.0, t)
    t = np.where(t < lo, lo, t)
    return np.where(hi < t, hi, t)


def proj_circle(a, b, rad):
    n2 = fma(b, b, a * a)
    if n2 > rad * abs(rad):
        sc = rad / np.sqrt(n2)
        return a * sc, b * sc
    return a, b


def project(kind, t, ex, n):
    if kind != "qcqp":
        lo, hi = effective_bounds(kind, ex, n)
        return proj_box(kind, t, lo, hi)
    out = np.empty(n)
    for k in range(n // 2):
        out[2 * k], out[2 * k + 1] = proj_circle(t[2 * k], t[2 * k + 1], float(ex[0].reshape(-1)[k]) * float(ex[1].reshape(-1)[k]))
    return out


def nmax_abs(F):
    r = 0.0
    for v in np.abs(F):
        if v > r or v != v:
            r = float(v)
    return r


def evaluate(kind, P, q, ex, x):
    """-> (z, F, r)"""
    n = x.shape[0]
    s = np.zeros(n)
    for j in range(n):
        s = s + P[:, j] * x[j]
    z = x - (s + q)
    F = x - project(kind, z, ex, n)
    return z, F, nmax_abs(F)


def jacobian(kind, z, ex, n):
    """D as a full (n,n) matrix."""
    D = np.zeros((n, n))
    if kind != "qcqp":
        lo, hi = effective_bounds(kind, ex, n)
        D[np.arange(n), np.arange(n)] = np.where((lo < z) & (z < hi), 1.0, 0.0)
        return D
    for k in range(n // 2):
        za, zb = float(z[2 * k]), float(z[2 * k + 1])
        rad = float(ex[0].reshape(-1)[k]) * float(ex[1].reshape(-1)[k])
        n2 = fma(zb, zb, za * za)
        if not n2 > rad * abs(rad):
            blk = (1.0, 0.0, 1.0)
        elif not rad > 0.0:
            blk = (0.0, 0.0, 0.0)
        else:
            nrm = np.sqrt(n2)
            sc, ua, ub = rad / nrm, za / nrm, zb / nrm
            blk = (sc * (1.0 - ua * ua), sc * (0.0 - ua * ub), sc * (1.0 - ub * ub))
        D[2 * k, 2 * k], D[2 * k, 2 * k + 1], D[2 * k + 1, 2 * k], D[2 * k + 1, 2 * k + 1] = blk[0], blk[1], blk[1], blk[2]
    return D


def newton_matrix(kind, P, D):
    n = P.shape[0]
    eye = np.eye(n)
    if kind != "qcqp":
        return np.where(np.diag(D)[:, None] != 0.0, P, eye)
    M = np.empty((n, n))
    for k in range(n // 2):
        for r in (2 * k, 2 * k + 1):
            M[r] = (eye[r] - D[r]) + (D[r, 2 * k] * P[2 * k] + D[r, 2 * k + 1] * P[2 * k + 1])
    return M


def solve(M, rhs):
    """Gaussian elimination with partial pivoting as polish_core.h orders it.  -> d, or None if a pivot is zero / not finite."""
    M, d = M.copy(), rhs.copy()
    n = d.shape[0]
    for k in range(n):
        best, piv = abs(M[k, k]), k
        for i in range(k + 1, n):
            if abs(M[i, k]) > best:
                best, piv = abs(M[i, k]), i
        if not (best > 0.0 and np.isfinite(best)):
            return None
        if piv != k:
            M[[k, piv], k:] = M[[piv, k], k:]
            d[[k, piv]] = d[[piv, k]]
        f = M[k + 1:, k] / M[k, k]
        rows = np.nonzero(f != 0.0)[0] + k + 1
        if rows.size:
            fr = f[rows - k - 1]
            d[rows] = d[rows] - fr * d[k]
            M[rows, k + 1:] = M[rows, k + 1:] - fr[:, None] * M[k, k + 1:][None, :]
    for k in range(n - 1, -1, -1):
        d[k] = d[k] / M[k, k]
        rows = np.nonzero(M[:k, k] != 0.0)[0]
        if rows.size:
            d[rows] = d[rows] - M[rows, k] * d[k]
    return d


def polish(kind, P, q, ex, x, max_steps=8):
    """One problem.  P (n,n), q (n), ex the kind's extras, x (n) -> (x_out, (r_before, r_after), steps, status)."""
    with np.errstate(all="ignore"):
        n = x.shape[0]
        ex = tuple(np.asarray(e, dtype=np.float64).reshape(-1) for e in ex)
        bad = not (np.isfinite(P).all() and np.isfinite(q).all() and np.isfinite(x).all() and all(np.isfinite(e).all() for e in ex))
        xc = x.copy()
        z, F, r0 = evaluate(kind, P, q, ex, xc)
        r, steps = r0, 0
        if bad or not np.isfinite(r0):
            return xc, (r0, r0), 0, 2
        while steps < max_steps and r != 0.0:
            d = solve(newton_matrix(kind, P, jacobian(kind, z, ex, n)), -F)
            if d is None:
                break
            xn = project(kind, xc + d, ex, n)
            zn, Fn, rn = evaluate(kind, P, q, ex, xn)
            if not rn < r:
                break
            xc, z, F, r = xn, zn, Fn, rn
            steps += 1
        return xc, (r0, r), steps, 0 if steps > 0 else 1


def polish_batch(kind, P, q, ex, x, max_steps=8):
    """P (B,n,n), q (B,n), ex each (B,.), x (B,n) -> x_out (B,n), resid (B,2), steps (B) int32, status (B) int32"""
    B, n = x.shape
    xo, rs, st, ss = np.empty((B, n)), np.empty((B, 2)), np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32)
    for b in range(B):
        xo[b], rs[b], st[b], ss[b] = polish(kind, P[b], q[b], tuple(e[b] for e in ex), x[b], max_steps)
    return xo, rs, st, ss


def scale(P, q, x):
    """resid[3] of dqq_check_f64 per problem: max(max_i sum_j |P_ij| |x_j|, max |q|)."""
    s = np.zeros(x.shape)
    for j in range(x.shape[1]):          # in index order, elementwise: the same bits on every host (a matrix product is not)
        s = s + np.abs(P[:, :, j]) * np.abs(x[:, j:j + 1])
    return np.maximum(s.max(axis=1), np.abs(q).max(axis=1))
