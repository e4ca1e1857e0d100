"""The Newton family on the central path (dqq_polish_smooth_f64, dqq_newton_bwd_smooth_f64, dqq_newton_jvp_smooth_f64) restated
in numpy: the definition of diffqcqp_amd/csrc/smooth_core.h a second time, operation by operation, on top of
tests/polish_reference.py (g, z, r, the elimination, the hard PI of the trial point), tests/polish_ls_reference.py (the step rule)
and tests/newton_reference.py, so that the host core (tests/hostcore/smooth_core_check.cpp) and through it the kernels can be held
to its bits.  Not a test file.

Per call one scalar kappa >= 0; s(t) = sqrt(t t + 4 (kappa kappa)); p(t) = (s + t) / 2 for t >= 0, (2 (kappa kappa)) / (s - t)
otherwise; p'(t) = (1 + t / s) / 2 for t >= 0, (2 (kappa kappa)) / (s (s - t)) otherwise.  P is always the full (n,n) matrix here.
kappa == 0 is a branch to the parents' restatements, not the formulas at 0."""
import numpy as np

import newton_reference as NR
import polish_ls_reference as L
import polish_reference as R

NAN = float("nan")


def s_(t, kappa):
    return np.sqrt(t * t + 4.0 * (kappa * kappa))


def p(t, kappa):
    """Elementwise, both branches evaluated and selected (what is not selected may be inf or nan: ignored)."""
    t = np.asarray(t, dtype=np.float64)
    s = s_(t, kappa)
    return np.where(t >= 0.0, (s + t) / 2.0, (2.0 * (kappa * kappa)) / (s - t))


def dp(t, kappa):
    t = np.asarray(t, dtype=np.float64)
    s = s_(t, kappa)
    return np.where(t >= 0.0, (1.0 + t / s) / 2.0, (2.0 * (kappa * kappa)) / (s * (s - t)))


def box(kind, z, ex, n, kappa):
    """-> (PI_k, D, E_lo, E_hi) per coordinate, E masked to the caller's own bounds."""
    if kind == "qp":
        return p(z, kappa), dp(z, kappa), np.zeros(n), np.zeros(n)
    lo, hi = R.effective_bounds(kind, ex, n)
    keep_lo = keep_hi = np.full(n, True)
    if kind == "sbox":
        keep_lo, keep_hi = lo == ex[0], hi == ex[1]
    tl, th = z - lo, z - hi
    dl, dh = dp(tl, kappa), dp(th, kappa)
    pi = (lo + p(tl, kappa)) - p(th, kappa)
    return pi, dl - dh, np.where(keep_lo, 1.0 - dl, 0.0), np.where(keep_hi, dh, 0.0)


def disc(za, zb, rad, kappa):
    """-> (pa, pb, (d00, d01, d11), ea, eb, on) of a contact."""
    za, zb, rad = float(za), float(zb), float(rad)
    if not rad > 0.0:
        return 0.0, 0.0, (0.0, 0.0, 0.0), 0.0, 0.0, False
    n2 = R.fma(zb, zb, za * za)
    t = float(np.sqrt(n2))
    u = t - rad
    pu, dpu = float(p(u, kappa)), float(dp(u, kappa))
    m = rad + pu
    sc, mm = rad / m, m * m
    c = 0.0 if t == 0.0 else (rad * dpu) / (mm * t)
    ca, cb = c * za, c * zb
    e = (pu + rad * dpu) / mm
    return za * sc, zb * sc, (sc - ca * za, 0.0 - ca * zb, sc - cb * zb), za * e, zb * e, True


def evaluate(kind, P, q, ex, x, kappa):
    """-> (z, F_k, r_k, D as a full (n,n) matrix, E: box-like (E_lo, E_hi); QCQP (E_rad (n), on (n/2)))"""
    n = x.shape[0]
    s = np.zeros(n)
    for j in range(n):
        s = s + P[:, j] * x[j]
    z = x - (s + q)
    D = np.zeros((n, n))
    if kind != "qcqp":
        pi, d, elo, ehi = box(kind, z, ex, n, kappa)
        D[np.arange(n), np.arange(n)] = d
        E = (elo, ehi)
    else:
        pi, er, on = np.empty(n), np.empty(n), np.empty(n // 2, dtype=bool)
        for k in range(n // 2):
            a, b = 2 * k, 2 * k + 1
            pi[a], pi[b], blk, er[a], er[b], on[k] = disc(z[a], z[b], float(ex[0][k]) * float(ex[1][k]), kappa)
            D[a, a], D[a, b], D[b, a], D[b, b] = blk[0], blk[1], blk[1], blk[2]
        E = (er, on)
    F = x - pi
    return z, F, R.nmax_abs(F), D, E


def matrix(kind, P, D):
    """M = (I - D) + D P, entry by entry as smooth_box_entry / polish_contact_entry round it."""
    if kind == "qcqp":
        return R.newton_matrix(kind, P, D)
    n = P.shape[0]
    dcol = np.diag(D)[:, None]
    return (np.eye(n) - D) + dcol * P


def _finite(*arrays):
    return all(a is None or np.isfinite(a).all() for a in arrays)


def polish(kind, P, q, ex, x, max_steps=8, max_halvings=0, reg=0.0, kappa=0.0):
    """One problem.  -> (x_out, (r_before, r_after), steps, status, halvings)"""
    if kappa == 0.0:
        return L.polish_ls(kind, P, q, ex, x, max_steps, max_halvings, reg)
    with np.errstate(all="ignore"):
        n = x.shape[0]
        ex = tuple(np.asarray(e, dtype=np.float64).reshape(-1) for e in ex)
        bad = not _finite(P, q, x, *ex)
        xc = x.copy()
        z, F, r0, D, _ = evaluate(kind, P, q, ex, xc, kappa)
        r, steps, halvings = r0, 0, 0
        if bad or not np.isfinite(r0):
            return xc, (r0, r0), 0, 2, 0
        Pm = L._with_reg(P, reg)
        while steps < max_steps and r != 0.0:
            d = R.solve(matrix(kind, Pm, D), -F)
            if d is None:
                break
            t, found = 1.0, None
            for k in range(max_halvings + 1):
                sstep = t * d
                xn = R.project(kind, xc + sstep, ex, n)
                zn, Fn, rn, Dn, _ = evaluate(kind, P, q, ex, xn, kappa)
                if rn < r:
                    found = k
                    break
                t = 0.5 * t
            if found is None:
                break
            xc, z, F, r, D = xn, zn, Fn, rn, Dn
            steps += 1
            halvings += found
        return xc, (r0, r), steps, 0 if steps > 0 else 1, halvings


def jvp(kind, P, q, ex, x, dP=None, dq=None, da=None, db=None, reg=0.0, kappa=0.0):
    """One problem -> (dx (n), status)."""
    if kappa == 0.0:
        assert reg == 0.0, "the hard derivatives with a proximal weight: tests/reg_reference.py"
        return NR.jvp(kind, P, q, ex, x, dP, dq, da, db)
    with np.errstate(all="ignore"):
        ex = tuple(np.asarray(e, dtype=np.float64).reshape(-1) for e in ex)
        n = x.shape[0]
        if not _finite(P, q, x, dP, dq, da, db, *ex):
            return np.full(n, NAN), 2
        z, _, _, D, E = evaluate(kind, P, q, ex, x, kappa)
        M = matrix(kind, L._with_reg(P, reg), D)
        s = np.zeros(n)
        if dP is not None:
            for j in range(n):
                s = s + dP[:, j] * x[j]
        t = s + (dq if dq is not None else 0.0)
        if kind == "qcqp":
            rhs = np.empty(n)
            er, on = E
            for k in range(n // 2):
                ln, mu = float(ex[0][k]), float(ex[1][k])
                drad = mu * (float(da[k]) if da is not None else 0.0) + ln * (float(db[k]) if db is not None else 0.0)
                for r_ in (2 * k, 2 * k + 1):
                    w = D[r_, 2 * k] * t[2 * k] + D[r_, 2 * k + 1] * t[2 * k + 1]
                    rhs[r_] = er[r_] * drad - w if on[k] else -w
        else:
            dlo = da if da is not None and kind != "qp" else np.zeros(n)
            dhi = db if db is not None and kind != "qp" else np.zeros(n)
            rhs = (E[0] * dlo + E[1] * dhi) - np.diag(D) * t
        dx = R.solve(M, rhs)
        return (np.full(n, NAN), 1) if dx is None else (dx, 0)


def backward(kind, P, q, ex, x, gx, reg=0.0, kappa=0.0):
    """One problem -> (grad_P (n,n), grad_q (n), grad_a, grad_b (None for the QP), status)."""
    if kappa == 0.0:
        assert reg == 0.0, "the hard derivatives with a proximal weight: tests/reg_reference.py"
        return NR.backward(kind, P, q, ex, x, gx)
    with np.errstate(all="ignore"):
        ex = tuple(np.asarray(e, dtype=np.float64).reshape(-1) for e in ex)
        n = x.shape[0]
        ne = 0 if kind == "qp" else (n // 2 if kind == "qcqp" else n)
        status, w = 0, None
        if not _finite(P, q, x, gx, *ex):
            status = 2
        else:
            z, _, _, D, E = evaluate(kind, P, q, ex, x, kappa)
            w = R.solve(np.ascontiguousarray(matrix(kind, L._with_reg(P, reg), D).T), gx)
            if w is None:
                status = 1
        if status:
            g = (np.full((n, n), NAN), np.full(n, NAN))
            return g + ((None, None) if kind == "qp" else (np.full(ne, NAN), np.full(ne, NAN))) + (status,)
        ga = gb = None
        if kind == "qcqp":
            v, ga, gb = np.empty(n), np.zeros(ne), np.zeros(ne)
            er, on = E
            for k in range(n // 2):
                ln, mu = float(ex[0][k]), float(ex[1][k])
                a, b = 2 * k, 2 * k + 1
                v[a] = D[a, a] * w[a] + D[a, b] * w[b]
                v[b] = D[b, a] * w[a] + D[b, b] * w[b]
                if on[k]:
                    t = er[a] * w[a] + er[b] * w[b]
                    ga[k], gb[k] = mu * t, ln * t
        else:
            v = np.diag(D) * w
            if kind != "qp":
                ga, gb = E[0] * w, E[1] * w
        return -(v[:, None] * x[None, :]), -v, ga, gb, 0


def polish_batch(kind, P, q, ex, x, max_steps=8, max_halvings=0, reg=0.0, kappa=0.0):
    """P (B,n,n), q (B,n), ex each (B,.), x (B,n) -> x_out (B,n), resid (B,2), steps, status, halvings (B) int32"""
    B, n = x.shape
    xo, rs = np.empty((B, n)), np.empty((B, 2))
    st, ss, hs = np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32)
    for b in range(B):
        xo[b], rs[b], st[b], ss[b], hs[b] = polish(kind, P[b], q[b], tuple(e[b] for e in ex), x[b], max_steps, max_halvings, reg, kappa)
    return xo, rs, st, ss, hs


def jvp_batch(kind, P, q, ex, x, dP=None, dq=None, da=None, db=None, reg=0.0, kappa=0.0):
    """-> dx (B,n), status (B) int32"""
    B, n = x.shape
    dx, st = np.empty((B, n)), np.empty(B, dtype=np.int32)
    pick = lambda a, b: None if a is None else a[b]
    for b in range(B):
        dx[b], st[b] = jvp(kind, P[b], q[b], tuple(e[b] for e in ex), x[b], pick(dP, b), pick(dq, b), pick(da, b), pick(db, b), reg, kappa)
    return dx, st


def backward_batch(kind, P, q, ex, x, gx, reg=0.0, kappa=0.0):
    """-> grad_P (B,n,n), grad_q (B,n), grad_a, grad_b (B,.) or None, status (B) int32"""
    B, n = x.shape
    ne = 0 if kind == "qp" else (n // 2 if kind == "qcqp" else n)
    gP, gq, st = np.empty((B, n, n)), np.empty((B, n)), np.empty(B, dtype=np.int32)
    ga, gb = (None, None) if kind == "qp" else (np.empty((B, ne)), np.empty((B, ne)))
    for b in range(B):
        r = backward(kind, P[b], q[b], tuple(e[b] for e in ex), x[b], gx[b], reg, kappa)
        gP[b], gq[b], st[b] = r[0], r[1], r[4]
        if ga is not None:
            ga[b], gb[b] = r[2], r[3]
    return gP, gq, ga, gb, st
