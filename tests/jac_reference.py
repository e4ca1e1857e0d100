"""The Newton Jacobians (dqq_newton_jac_f64) restated in numpy: newton_core.h's newton_jac_problem a second time, operation by
operation, on top of tests/polish_reference.py and tests/newton_reference.py.  Not a test file.

Per problem, float64, P always the full (n,n) matrix here, at the x given: column j of Jq (Ja, Jb) is newton_reference.jvp's dx
for dq (da, db) = e_j and every other tangent None -- the same right-hand side, entry by entry -- and all columns go through ONE
elimination (solve_multi: polish_reference.solve's row operations, which depend on M only, applied to every column)."""
import numpy as np

import newton_reference as NR
import polish_reference as R

NAN = float("nan")


def extra_cols(kind, n):
    return 0 if kind == "qp" else (n // 2 if kind == "qcqp" else n)


def solve_multi(M, Rhs):
    """polish_core.h's polish_solve_multi: M (n,n), Rhs (n,C) -> the solutions (n,C), or None if a pivot is zero / not finite."""
    M, d = M.copy(), Rhs.copy()
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
            d[rows] = d[rows] - fr[:, None] * d[k][None, :]
            M[rows, k + 1:] = M[rows, k + 1:] - fr[:, None] * M[k, k + 1:][None, :]
    for k in range(n - 1, -1, -1):
        d[k] = d[k] / M[k, k]
        rows = np.nonzero(M[:k, k] != 0.0)[0]
        if rows.size:
            d[rows] = d[rows] - M[rows, k][:, None] * d[k][None, :]
    return d


def rhs_block(kind, z, D, ex, n, which):
    """(n, columns of input `which`: 0 q, 1 a, 2 b): newton_reference.jvp's right-hand side for each unit tangent."""
    w = n if which == 0 else extra_cols(kind, n)
    out = np.empty((n, w))
    zero = np.zeros(n)
    for j in range(w):
        e = np.zeros(w)
        e[j] = 1.0
        t = zero + (e if which == 0 else 0.0)     # s + dq, s = 0.0
        if kind == "qcqp":
            for k in range(n // 2):
                ln, mu = float(ex[0][k]), float(ex[1][k])
                on, ua, ub = NR.disc_u(float(z[2 * k]), float(z[2 * k + 1]), ln * mu)
                drad = mu * (e[k] if which == 1 else 0.0) + ln * (e[k] if which == 2 else 0.0)
                for r, u in ((2 * k, ua), (2 * k + 1, ub)):
                    wv = D[r, 2 * k] * t[2 * k] + D[r, 2 * k + 1] * t[2 * k + 1]
                    out[r, j] = u * drad - wv if on else -wv
        else:
            st = NR.box_state(kind, z, ex, n)
            dlo = e if which == 1 else zero
            dhi = e if which == 2 else zero
            out[:, j] = np.where(st == 0, -t, np.where(st == 1, dlo, np.where(st == 2, dhi, 0.0)))
    return out


def setup(kind, P, q, ex, x):
    """-> (n, z, D, M) of a problem (newton_reference's)."""
    return NR._setup(kind, P, q, ex, x)


def jacobians(kind, P, q, ex, x, need=(True, True, True)):
    """One problem.  P (n,n), q (n), ex the kind's extras, x (n) -> (Jq (n,n), Ja, Jb (n,ne); None where not needed or the QP has
    none, status)."""
    with np.errstate(all="ignore"):
        ex = tuple(np.asarray(e, dtype=np.float64).reshape(-1) for e in ex)
        n = x.shape[0]
        ne = extra_cols(kind, n)
        need = tuple(bool(v) and (i == 0 or kind != "qp") for i, v in enumerate(tuple(need) + (True,) * (3 - len(need))))
        widths = [n if i == 0 else ne for i in range(3)]
        nan = lambda: tuple(np.full((n, widths[i]), NAN) if need[i] else None for i in range(3))
        if not NR._finite(P, q, x, *ex):
            return nan() + (2,)
        n, z, D, M = setup(kind, P, q, ex, x)
        blocks = [rhs_block(kind, z, D, ex, n, i) for i in range(3) if need[i]]
        sol = solve_multi(M, np.concatenate(blocks, axis=1))
        if sol is None:
            return nan() + (1,)
        out, off = [], 0
        for i in range(3):
            out.append(np.ascontiguousarray(sol[:, off:off + widths[i]]) if need[i] else None)
            off += widths[i] if need[i] else 0
        return tuple(out) + (0,)


def jacobians_batch(kind, P, q, ex, x, need=(True, True, True)):
    """P (B,n,n), q, x (B,n), ex each (B,.) -> Jq (B,n,n), Ja, Jb (B,n,ne) or None, status (B) int32"""
    B, n = x.shape
    ne = extra_cols(kind, n)
    need = tuple(bool(v) and (i == 0 or kind != "qp") for i, v in enumerate(need))
    out = [np.empty((B, n, n if i == 0 else ne)) if need[i] else None for i in range(3)]
    st = np.empty(B, dtype=np.int32)
    for b in range(B):
        r = jacobians(kind, P[b], q[b], tuple(e[b] for e in ex), x[b], need)
        st[b] = r[3]
        for i in range(3):
            if need[i]:
                out[i][b] = r[i]
    return out[0], out[1], out[2], st


def compact(kind, J, which):
    """The DQQ_P_DIAG form of a Jacobian (B,n,.) of a diagonal P: its diagonal blocks (header: dqq_newton_jac_f64)."""
    B, n = J.shape[:2]
    i = np.arange(n)
    if kind != "qcqp":
        return np.ascontiguousarray(J[:, i, i])
    if which == 0:
        return np.ascontiguousarray(np.stack([J[:, i, 2 * (i // 2)], J[:, i, 2 * (i // 2) + 1]], axis=2))
    return np.ascontiguousarray(J[:, i, i // 2])


def off_block_mask(kind, n, which):
    """(n, columns) bool: True off the diagonal blocks."""
    w = n if which == 0 else extra_cols(kind, n)
    i, j = np.arange(n)[:, None], np.arange(w)[None, :]
    if kind != "qcqp":
        return i != j
    return (i // 2 != j // 2) if which == 0 else (i // 2 != j)
