"""A numpy restatement of the four ADMM forward loops (Solver::solveQP / solveQCQP / solveBoxQP / solveSignedBoxQP as
oracle/diffqcqp_oracle.c: admm_solve_ex restates them) WITH a start point.  Not a test file: the yardstick of
tests/test_gpu_warm.py, pinned to the oracle -- which knows no warm start -- by tests/test_warm_reference.py (x0 = None: the
oracle's iteration counts exactly, its x within 1e-12).

The loop is the oracle's, operation for operation and in its order of summation (every inner sum runs sequentially over the
index, vectorised over the batch only), so that nothing but the state at entry separates a warm solve from the pinned cold one:

    x0 = None     l_2 = l_2_pred = 0,  u = 0,            q_prox = q                 (the reference)
    x0 (B,N,1)    l_2 = l_2_pred = x0, u = -(P x0 + q),  q_prox = q - mu_prox x0    (include/diffqcqp_hip.h: dqq_fwd_warm_f64)

L, rho, tau_inc, tau_dec, rho_up and cpt are the cold start's in both.  x0 is taken as given (not projected); max_iter = 0
returns it; x0 = 0 is not the cold start (u = -q)."""
import math

import numpy as np

KINDS = {"qp": 0, "qcqp": 1, "box": 2, "sbox": 3}
MU_THRESH, ALPHA, EPS_REL = 10., 1.5, 1e-4


def _matvec(A, v):
    """(B,n,n) x (B,n) -> (B,n): s += A[i][j] * v[j], j ascending (oracle matvec)."""
    s = np.zeros_like(v)
    for j in range(A.shape[2]):
        s = s + A[:, :, j] * v[:, j:j + 1]
    return s


def _chol_inverse(A):
    """Lower Cholesky + the explicit inverse, column by column (oracle chol_inverse); only the lower triangle of A is read."""
    B, n, _ = A.shape
    if n > 16:   # python-level loops cost seconds here: LAPACK's Cholesky of the same (lower) matrix, ~1e-16 cond apart.  The
        # pin to the oracle (tests/test_warm_reference.py) is at N = 8, on the sequential code below
        low = np.tril(A)
        sym = low + np.transpose(np.tril(A, -1), (0, 2, 1))
        ok = np.isfinite(sym).all(axis=(1, 2))
        out = np.full_like(A, np.nan)
        if ok.any():
            try:
                Lc = np.linalg.cholesky(sym[ok])
                Li = np.linalg.solve(Lc, np.broadcast_to(np.eye(n), Lc.shape))
                out[ok] = np.transpose(Li, (0, 2, 1)) @ Li
            except np.linalg.LinAlgError:
                pass
        return out
    L = np.zeros_like(A)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(n):
            s = np.zeros(B)
            for j in range(k):
                s = s + L[:, k, j] * L[:, k, j]
            x = np.sqrt(A[:, k, k] - s)
            L[:, k, k] = x
            if k + 1 < n:
                t = np.zeros((B, n - k - 1))
                for j in range(k):
                    t = t + L[:, k + 1:, j] * L[:, k:k + 1, j]
                L[:, k + 1:, k] = (A[:, k + 1:, k] - t) / x[:, None]
        Ainv = np.zeros_like(A)   # [b, i, c]
        for i in range(n):
            t = np.zeros((B, n))
            t[:, i] = 1.0
            for j in range(i):
                t = t - L[:, i:i + 1, j] * Ainv[:, j, :]
            Ainv[:, i, :] = t / L[:, i:i + 1, i]
        for i in range(n - 1, -1, -1):
            t = Ainv[:, i, :].copy()
            for j in range(i + 1, n):
                t = t - L[:, j:j + 1, i] * Ainv[:, j, :]
            Ainv[:, i, :] = t / L[:, i:i + 1, i]
    return Ainv


def _power_iteration(P, steps):
    B, n, _ = P.shape
    v = np.full((B, n), 1 / math.sqrt(n))

    def normalize(v):
        s = np.zeros(B)
        for i in range(n):
            s = s + v[:, i] * v[:, i]
        nn = np.sqrt(s)
        return np.where((s > 0)[:, None], v / np.where(s > 0, nn, 1.0)[:, None], v)
    v = normalize(v)
    for _ in range(steps):
        v = normalize(_matvec(P, v))
    Av = _matvec(P, v)
    lmax = np.zeros(B)
    for i in range(n):
        lmax = lmax + v[:, i] * Av[:, i]
    return lmax


def _pow(a, e):
    return np.array([math.pow(x, e) if x == x and x >= 0 else float("nan") for x in a.tolist()])


def solve(kind, P, q, eps, max_iter, extras=(), x0=None, mu_prox=1e-7, adaptive=True):
    """kind: 'qp' | 'qcqp' | 'box' | 'sbox' or 0..3; P (B,n,n), q (B,n,1); extras: (), (l_n, mu), (l_min, l_max),
    (l_min, l_max, v) with the reference's shapes; x0: None or (B,n,1).  -> (x (B,n,1), iters (B) int32)."""
    kind = KINDS.get(kind, kind)
    qp_like = kind != 1
    P = np.ascontiguousarray(P, dtype=np.float64)
    B, n, _ = P.shape
    q = np.asarray(q, dtype=np.float64).reshape(B, n)
    ex = [np.asarray(e, dtype=np.float64).reshape(B, -1) for e in extras]
    if kind == 1:
        radius = ex[0] * ex[1]                                      # pybindings.cpp:57
    elif kind >= 2:
        lo, hi = ex[0], ex[1]
        sg = np.sign(ex[2]) if kind == 3 else None
    lmax = _power_iteration(P, 10 if qp_like else 100)
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = np.sqrt(mu_prox * lmax) * _pow(lmax / mu_prox, .4)
        tau_inc = _pow(lmax / mu_prox, .15)
    tau_dec = tau_inc.copy()
    if x0 is None:
        l_2 = np.zeros((B, n))
        u = np.zeros((B, n))
        q_prox = q.copy()
    else:
        l_2 = np.array(x0, dtype=np.float64).reshape(B, n)
        u = -(_matvec(P, l_2) + q)
        q_prox = q - mu_prox * l_2
    l_2_pred = l_2.copy()
    M = P.copy()
    idx = np.arange(n)
    M[:, idx, idx] += (rho + mu_prox)[:, None]
    Minv = _chol_inverse(M)
    rho_up = np.zeros(B, dtype=np.int64)
    cpt = np.zeros(B, dtype=np.int64)
    iters = np.zeros(B, dtype=np.int32)
    act = np.ones(B, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for it in range(max_iter):
            if not act.any():
                break
            iters[act] = it + 1
            l = _matvec(Minv, rho[:, None] * l_2 - u - q_prox)
            q_prox_n = q - mu_prox * l
            t = ALPHA * l + (1 - ALPHA) * l_2 + u / rho[:, None]
            if kind == 0:
                t = np.where(t < 0, 0.0, t)
            elif kind >= 2:
                t = np.where(t < lo, lo, t)
                t = np.where(hi < t, hi, t)
                if kind == 3:
                    m = sg * t
                    m = np.where(0 < m, 0.0, m)
                    t = sg * m
            else:
                a, b = t[:, 0::2], t[:, 1::2]
                nrm = np.sqrt(a * a + b * b)
                big = nrm > radius
                t = t.copy()
                t[:, 0::2] = np.where(big, a * radius / nrm, a)
                t[:, 1::2] = np.where(big, b * radius / nrm, b)
            l_2_n = t
            w = ALPHA * l + (1 - ALPHA) * l_2_pred
            u_n = u + rho[:, None] * (w - l_2_n)
            d = l_2_n - l_2_pred
            if qp_like:
                res_dual = np.fmax.reduce(np.abs(rho[:, None] * d), axis=1, initial=0.0)   # (the oracle's `>` skips a NaN)
            else:
                res_dual = rho * np.fmax.reduce(np.abs(d), axis=1, initial=0.0)
            res_prim = np.fmax.reduce(np.abs(l_2_n - w), axis=1, initial=0.0)
            # commit the iteration for the problems still running
            a_ = act[:, None]
            q_prox = np.where(a_, q_prox_n, q_prox)
            l_2 = np.where(a_, l_2_n, l_2)
            u = np.where(a_, u_n, u)
            l_2_pred = l_2.copy()
            stop = res_dual < eps
            if kind == 1:
                s = np.zeros(B)
                for i in range(n):
                    s = s + l[:, i] * l[:, i]
                stop = stop & (res_prim < eps + EPS_REL * np.sqrt(s))
            act = act & ~stop
            if not adaptive:
                continue
            inc = act & (res_prim > MU_THRESH * res_dual)
            dec = act & ~inc & (res_dual > MU_THRESH * res_prim)
            fire_i = inc & (cpt % 5 == 0)
            fire_d = dec & (cpt % 5 == 0)
            cpt = cpt + (inc | dec)
            if fire_i.any() or fire_d.any():
                damp_i, damp_d = fire_i & (rho_up == -1), fire_d & (rho_up == 1)
                ti, td = 1 + .8 * (tau_inc - 1), 1 + .8 * (tau_dec - 1)
                if qp_like:
                    both = damp_i | damp_d
                    tau_inc = np.where(both, ti, tau_inc)
                    tau_dec = np.where(both, td, tau_dec)
                else:
                    tau_inc = np.where(damp_i, ti, tau_inc)
                    tau_dec = np.where(damp_d, td, tau_dec)
                delta = np.where(fire_i, rho * (tau_inc - 1), np.where(fire_d, rho * (1. / tau_dec - 1), 0.0))
                rho = np.where(fire_i, rho * tau_inc, np.where(fire_d, rho / tau_dec, rho))
                rho_up = np.where(fire_i, 1, np.where(fire_d, -1, rho_up))
                fired = fire_i | fire_d
                M[fired[:, None, None] & np.eye(n, dtype=bool)[None]] += np.repeat(delta[fired], n)
                Minv[fired] = _chol_inverse(M[fired])
    return l_2.reshape(B, n, 1), iters


def perturbed_start(kind, P, q, extras, rel, seed, eps=1e-7, max_iter=1000):
    """The cold solution of the batch with q perturbed by `rel` (q (1 + rel N(0,1)) entry by entry): what the last step of a
    time-stepping loop would hand over."""
    rng = np.random.default_rng(seed)
    qn = np.asarray(q, dtype=np.float64)
    qp = qn * (1 + rel * rng.standard_normal(qn.shape))
    return solve(kind, P, qp, eps, max_iter, extras)[0]
