"""The Newton family with DQQ_F_INFINITE_BOUNDS restated in numpy: tests/polish_reference.py, newton_reference.py and
jac_reference.py with the input rule of the box kinds' bounds replaced -- and nothing else.  Not a test file.

The rule (csrc/polish_core.h: polish_lo_bad / polish_hi_bad): with the flag a lower bound may be finite or -inf, an upper bound
finite or +inf; l_min = +inf, l_max = -inf and a NaN are status 2, as is any other entry that is not finite (P, q, x, v, the
cotangent, a given tangent, the polish's first r).  Everything behind the rule is the unflagged restatements' own functions
(evaluate, jacobian, newton_matrix, solve, box_state, rhs_block, solve_multi): they compare a bound and select it, and never
take it as an operand of arithmetic, so they are called as they are."""
import numpy as np

import jac_reference as JR
import newton_reference as NR
import polish_reference as R

NAN = float("nan")
INF = float("inf")
BOX_KINDS = ("box", "sbox")


def inputs_bad(kind, P, q, ex, x, more=(), flag=True):
    """polish_inputs_bad with inf_ok = flag, plus `more` (cotangent, tangents; None = not given): finite-only."""
    bad = not NR._finite(P, q, x, *more)
    for i, e in enumerate(ex):
        e = np.asarray(e, dtype=np.float64)
        if flag and kind in BOX_KINDS and i == 0:
            bad = bad or not bool((e < INF).all())        # finite or -inf; a NaN fails the comparison
        elif flag and kind in BOX_KINDS and i == 1:
            bad = bad or not bool((e > -INF).all())       # finite or +inf
        else:
            bad = bad or not bool(np.isfinite(e).all())
    return bad


def polish(kind, P, q, ex, x, max_steps=8, flag=True):
    """polish_reference.polish with the flagged input rule -> (x_out, (r_before, r_after), steps, status, reach): reach is the
    largest |x + d| of any step that was tried (0.0 if none was)."""
    with np.errstate(all="ignore"):
        n = x.shape[0]
        ex = tuple(np.asarray(e, dtype=np.float64).reshape(-1) for e in ex)
        bad = inputs_bad(kind, P, q, ex, x, flag=flag)
        xc = x.copy()
        z, F, r0 = R.evaluate(kind, P, q, ex, xc)
        r, steps, reach = r0, 0, 0.0
        if bad or not np.isfinite(r0):
            return xc, (r0, r0), 0, 2, reach
        while steps < max_steps and r != 0.0:
            d = R.solve(R.newton_matrix(kind, P, R.jacobian(kind, z, ex, n)), -F)
            if d is None:
                break
            reach = max(reach, float(np.abs(xc + d).max()))
            xn = R.project(kind, xc + d, ex, n)
            zn, Fn, rn = R.evaluate(kind, P, q, ex, xn)
            if not rn < r:
                break
            xc, z, F, r = xn, zn, Fn, rn
            steps += 1
        return xc, (r0, r), steps, 0 if steps > 0 else 1, reach


def jvp(kind, P, q, ex, x, dP=None, dq=None, da=None, db=None, flag=True):
    """newton_reference.jvp with the flagged input rule -> (dx, status)."""
    with np.errstate(all="ignore"):
        ex = tuple(np.asarray(e, dtype=np.float64).reshape(-1) for e in ex)
        n = x.shape[0]
        if inputs_bad(kind, P, q, ex, x, (dP, dq, da, db), flag):
            return np.full(n, NAN), 2
        assert kind != "qcqp"                      # (the flag changes nothing for the QCQP: newton_reference.jvp is its rule)
        n, z, D, M = NR._setup(kind, P, q, ex, x)
        s = np.zeros(n)
        if dP is not None:
            for j in range(n):
                s = s + dP[:, j] * x[j]
        t = s + (dq if dq is not None else 0.0)
        st = NR.box_state(kind, z, ex, n)
        dlo = da if da is not None and kind != "qp" else np.zeros(n)
        dhi = db if db is not None and kind != "qp" else np.zeros(n)
        rhs = np.where(st == 0, -t, np.where(st == 1, dlo, np.where(st == 2, dhi, 0.0)))
        dx = R.solve(M, rhs)
        return (np.full(n, NAN), 1) if dx is None else (dx, 0)


def backward(kind, P, q, ex, x, gx, flag=True):
    """newton_reference.backward with the flagged input rule -> (grad_P, grad_q, grad_a, grad_b, status)."""
    with np.errstate(all="ignore"):
        ex = tuple(np.asarray(e, dtype=np.float64).reshape(-1) for e in ex)
        n = x.shape[0]
        assert kind in BOX_KINDS
        w = None
        status = 2 if inputs_bad(kind, P, q, ex, x, (gx,), flag) else 0
        if not status:
            n, z, D, M = NR._setup(kind, P, q, ex, x)
            w = R.solve(np.ascontiguousarray(M.T), gx)
            status = 1 if w is None else 0
        if status:
            return np.full((n, n), NAN), np.full(n, NAN), np.full(n, NAN), np.full(n, NAN), status
        st = NR.box_state(kind, z, ex, n)
        v = np.where(st == 0, w, 0.0)
        return -(v[:, None] * x[None, :]), -v, np.where(st == 1, w, 0.0), np.where(st == 2, w, 0.0), 0


def jacobians(kind, P, q, ex, x, flag=True):
    """jac_reference.jacobians (every output) with the flagged input rule -> (Jq, Ja, Jb, status)."""
    with np.errstate(all="ignore"):
        ex = tuple(np.asarray(e, dtype=np.float64).reshape(-1) for e in ex)
        n = x.shape[0]
        assert kind in BOX_KINDS
        nan = lambda: tuple(np.full((n, n), NAN) for _ in range(3))      # noqa: E731
        if inputs_bad(kind, P, q, ex, x, flag=flag):
            return nan() + (2,)
        n, z, D, M = JR.setup(kind, P, q, ex, x)
        sol = JR.solve_multi(M, np.concatenate([JR.rhs_block(kind, z, D, ex, n, i) for i in range(3)], axis=1))
        if sol is None:
            return nan() + (1,)
        return tuple(np.ascontiguousarray(sol[:, i * n:(i + 1) * n]) for i in range(3)) + (0,)


def run_batch(kind, P, q, ex, x, gx, tangents=(None, None, None, None), max_steps=8, flag=True):
    """All four over a batch: P (B,n,n), q, x, gx (B,n), ex each (B,n), tangents batched or None.  -> a dict of arrays keyed as
    inf_bounds_cases.host_all's, plus "reach" (B)."""
    B, n = x.shape
    o = {k: np.empty((B, n)) for k in ("x_out", "dx", "gq", "ga", "gb")}
    o.update({k: np.empty((B, n, n)) for k in ("gP", "Jq", "Ja", "Jb")})
    o["resid"], o["reach"] = np.empty((B, 2)), np.empty(B)
    o.update({k: np.empty(B, dtype=np.int32) for k in ("steps", "st_polish", "st_jvp", "st_bwd", "st_jac")})
    pick = lambda a, b: None if a is None else a[b]      # noqa: E731
    for b in range(B):
        exb = tuple(e[b] for e in ex)
        o["x_out"][b], o["resid"][b], o["steps"][b], o["st_polish"][b], o["reach"][b] = polish(kind, P[b], q[b], exb, x[b],
                                                                                                max_steps, flag)
        o["dx"][b], o["st_jvp"][b] = jvp(kind, P[b], q[b], exb, x[b], *(pick(t, b) for t in tangents), flag=flag)
        o["gP"][b], o["gq"][b], o["ga"][b], o["gb"][b], o["st_bwd"][b] = backward(kind, P[b], q[b], exb, x[b], gx[b], flag)
        o["Jq"][b], o["Ja"][b], o["Jb"][b], o["st_jac"][b] = jacobians(kind, P[b], q[b], exb, x[b], flag)
    return o


def natural_residual(kind, P, q, ex, x):
    """max |x - PI(x - (P x + q))| per problem of a batch, polish_reference's evaluation (bounds may be infinite)."""
    with np.errstate(all="ignore"):
        return np.array([R.evaluate(kind, P[b], q[b], tuple(np.asarray(e[b], dtype=np.float64).reshape(-1) for e in ex), x[b])[2]
                         for b in range(x.shape[0])])
