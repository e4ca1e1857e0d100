"""The smoothed Newton Jacobians (dqq_newton_jac_smooth_f64) restated in numpy: smooth_core.h's newton_jac_problem_smooth a second
time, operation by operation, on top of tests/smooth_reference.py (PI_k, D, E, the smoothed M) and tests/jac_reference.py (the
multi-column elimination, the compact form).  Not a test file.

Per problem, float64, P always the full (n,n) matrix here, at the x given: column j of Jq (Ja, Jb) is smooth_reference.jvp's dx for
dq (da, db) = e_j and every other tangent None -- the same right-hand side, entry by entry -- and all columns go through ONE
elimination of M = (I - D) + D (P + reg I).  kappa == 0 is a branch to jac_reference (with a proximal weight: to reg_reference),
not the formulas at 0."""
import numpy as np

import jac_reference as JR
import polish_ls_reference as L
import reg_reference as RG
import smooth_reference as S

NAN = float("nan")
extra_cols = JR.extra_cols
compact = JR.compact
off_block_mask = JR.off_block_mask


def rhs_block(kind, D, E, ex, n, which):
    """(n, columns of input `which`: 0 q, 1 a, 2 b): smooth_reference.jvp's right-hand side for each unit tangent."""
    w = n if which == 0 else extra_cols(kind, n)
    out = np.empty((n, w))
    zero = np.zeros(n)
    for j in range(w):
        e = np.zeros(w)
        e[j] = 1.0
        t = zero + (e if which == 0 else 0.0)     # s + dq, s = 0.0
        if kind == "qcqp":
            er, on = E
            for k in range(n // 2):
                ln, mu = float(ex[0][k]), float(ex[1][k])
                drad = mu * (e[k] if which == 1 else 0.0) + ln * (e[k] if which == 2 else 0.0)
                for r in (2 * k, 2 * k + 1):
                    wv = D[r, 2 * k] * t[2 * k] + D[r, 2 * k + 1] * t[2 * k + 1]
                    out[r, j] = er[r] * drad - wv if on[k] else -wv
        else:
            dlo = e if which == 1 else zero
            dhi = e if which == 2 else zero
            out[:, j] = (E[0] * dlo + E[1] * dhi) - np.diag(D) * t
    return out


def jacobians(kind, P, q, ex, x, need=(True, True, True), reg=0.0, kappa=0.0):
    """One problem.  P (n,n), q (n), ex the kind's extras, x (n) -> (Jq (n,n), Ja, Jb (n,ne); None where not needed or the QP has
    none, status)."""
    if kappa == 0.0:
        if reg == 0.0:
            return JR.jacobians(kind, P, q, ex, x, need)
        # the hard Jacobians with a proximal weight: tests/reg_reference.py's, column by column through its own JVP
        need = tuple(bool(v) and (i == 0 or kind != "qp") for i, v in enumerate(tuple(need) + (True,) * (3 - len(need))))
        r = RG.jacobian(kind, P, q, tuple(np.asarray(e, dtype=np.float64).reshape(-1) for e in ex), x, reg)
        return tuple(r[i] if need[i] else None for i in range(3)) + (r[3],)
    with np.errstate(all="ignore"):
        ex = tuple(np.asarray(e, dtype=np.float64).reshape(-1) for e in ex)
        n = x.shape[0]
        ne = extra_cols(kind, n)
        need = tuple(bool(v) and (i == 0 or kind != "qp") for i, v in enumerate(tuple(need) + (True,) * (3 - len(need))))
        widths = [n if i == 0 else ne for i in range(3)]
        nan = lambda: tuple(np.full((n, widths[i]), NAN) if need[i] else None for i in range(3))     # noqa: E731
        if not S._finite(P, q, x, *ex):
            return nan() + (2,)
        _, _, _, D, E = S.evaluate(kind, P, q, ex, x, kappa)
        M = S.matrix(kind, L._with_reg(P, reg), D)
        blocks = [rhs_block(kind, D, E, ex, n, i) for i in range(3) if need[i]]
        sol = JR.solve_multi(M, np.concatenate(blocks, axis=1))
        if sol is None:
            return nan() + (1,)
        out, off = [], 0
        for i in range(3):
            out.append(np.ascontiguousarray(sol[:, off:off + widths[i]]) if need[i] else None)
            off += widths[i] if need[i] else 0
        return tuple(out) + (0,)


def jacobians_batch(kind, P, q, ex, x, need=(True, True, True), reg=0.0, kappa=0.0):
    """P (B,n,n), q, x (B,n), ex each (B,.) -> Jq (B,n,n), Ja, Jb (B,n,ne) or None, status (B) int32"""
    B, n = x.shape
    ne = extra_cols(kind, n)
    need = tuple(bool(v) and (i == 0 or kind != "qp") for i, v in enumerate(tuple(need) + (True,) * (3 - len(need))))
    out = [np.empty((B, n, n if i == 0 else ne)) if need[i] else None for i in range(3)]
    st = np.empty(B, dtype=np.int32)
    for b in range(B):
        r = jacobians(kind, P[b], q[b], tuple(e[b] for e in ex), x[b], need, reg, kappa)
        st[b] = r[3]
        for i in range(3):
            if need[i]:
                out[i][b] = r[i]
    return out[0], out[1], out[2], st
