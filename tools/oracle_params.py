"""The oracle at any solver parameters, and backward inputs on which the dual-recovery threshold matters.

fwd() / bwd() reach mu_prox, adaptive_rho and epsilon through the oracle's single-problem functions (the reference's pybind11
signatures, oracle/oracle.py), assembling the gradients as its batch loops do, so that the fuzzers (tools/fuzz_small.py,
tools/fuzz_bwd.py) need nothing of the oracle beyond that long-standing API.  nudge(): the oracle's forward x with a share of
its constraints made barely inactive (tests/param_cases.py, tools/fuzz_bwd.py)."""
import numpy as np


def fwd(O, kind, d, eps, max_iter, mu_prox=1e-7, adaptive=True, nthreads=16):
    """-> x (B,N,1), iterations (B,) of the forward; d: dict of numpy arrays (make_problem's keys)."""
    if adaptive:
        if kind == "qp":
            return O.qp_fwd_batch(d["P"], d["q"], eps, max_iter, mu_prox=mu_prox, nthreads=nthreads)
        if kind == "qcqp":
            return O.qcqp_fwd_batch(d["P"], d["q"], d["l_n"], d["mu"], eps, max_iter, mu_prox=mu_prox, nthreads=nthreads)
        return O.boxqp_fwd_batch(d["P"], d["q"], d["l_min"], d["l_max"], eps, max_iter, v=d.get("v") if kind == "sbox" else None,
                                 mu_prox=mu_prox, nthreads=nthreads)
    B, N = d["q"].shape[0], d["q"].shape[1]
    x, it = np.empty((B, N, 1)), np.empty(B, dtype=np.int32)
    for b in range(B):
        args = (eps, mu_prox, max_iter, False)
        if kind == "qp":
            r = O.solveQP(d["P"][b], d["q"][b], None, *args, return_iters=True)
        elif kind == "qcqp":
            r = O.solveQCQP(d["P"][b], d["q"][b], d["l_n"][b], d["mu"][b], None, *args, return_iters=True)
        elif kind == "box":
            r = O.solveBoxQP(d["P"][b], d["q"][b], d["l_min"][b], d["l_max"][b], None, *args, return_iters=True)
        else:
            r = O.solveSignedBoxQP(d["P"][b], d["q"][b], d["l_min"][b], d["l_max"][b], d["v"][b], None, *args,
                                   return_iters=True)
        x[b, :, 0], it[b] = r
    return x, it


def bwd(O, kind, d, x, epsilon):
    """The batch backward's outputs at dual-recovery threshold epsilon: qp (grad_P, grad_q, steps), qcqp (grad_P, grad_q,
    grad_l_n, grad_mu, steps), box (grad_P, grad_q, grad_l_min, grad_l_max, gamma (B,2N), steps (B,2))."""
    B, N = d["q"].shape[0], d["q"].shape[1]
    nc = N // 2
    gP, gq = np.empty((B, N, N)), np.empty((B, N, 1))
    if kind == "qcqp":
        gl, gm, st = np.empty((B, nc, 1)), np.empty((B, nc, 1)), np.empty(B, dtype=np.int32)
    elif kind == "box":
        glo, ghi, gam, st = np.empty((B, N, 1)), np.empty((B, N, 1)), np.empty((B, 2 * N)), np.empty((B, 2), dtype=np.int32)
    else:
        st = np.empty(B, dtype=np.int32)
    for b in range(B):
        xb, gb = x[b, :, 0], d["grad_x"][b, :, 0]
        if kind == "qp":
            dl, st[b] = O.solveDerivativesQP(d["P"][b], d["q"][b], xb, gb, epsilon, return_steps=True)
        elif kind == "qcqp":
            E1, E2, blg, st[b], _ = O.solveDerivativesQCQP(d["P"][b], d["q"][b], d["l_n"][b], d["mu"][b], xb, gb, epsilon,
                                                           return_steps=True)
            dl = blg[nc:]
            gl[b, :, 0], gm[b, :, 0] = np.diag(E2) * blg[:nc], np.diag(E1) * blg[:nc]
        else:
            blg, g, st[b] = O.solveDerivativesBoxQP(d["P"][b], d["q"][b], d["l_min"][b], d["l_max"][b], xb, gb, epsilon,
                                                    return_steps=True)
            dl = blg[2 * N:]
            glo[b, :, 0], ghi[b, :, 0], gam[b] = -(blg[:N] * g[:N]), blg[N:2 * N] * g[N:], g
        gP[b] = -(dl[:, None] * xb[None, :])
        gq[b, :, 0] = -dl
    if kind == "qp":
        return gP, gq, st
    if kind == "qcqp":
        return gP, gq, gl, gm, st
    return gP, gq, glo, ghi, gam, st


def nudge(kind, d, x, seed):
    """x (B,N,1) of the oracle's forward on batch d, with, independently with probability 1/2 each, and delta =
    10^U(-9,-1.5):  QP: a coordinate with x = 0 set to delta;  QCQP: a contact on its cone boundary
    (| ||x_c|| - r_c | < 1e-6 max(1, r_c), r_c = l_n mu) scaled inward to radius max(r_c - delta, 0);  box: a coordinate
    on a bound moved inside by delta.  Every draw is made for every coordinate / contact, so the result is a function of
    (seed, shape) and the data alone."""
    rng = np.random.default_rng(seed)
    x = np.array(x, dtype=np.float64, copy=True)
    B, N = x.shape[0], x.shape[1]
    if kind == "qcqp":
        nc = N // 2
        pick = rng.random((B, nc)) < 0.5
        delta = 10.0 ** rng.uniform(-9, -1.5, (B, nc))
        r = (np.asarray(d["l_n"]) * np.asarray(d["mu"]))[:, :, 0]
        xc = x[:, :, 0].reshape(B, nc, 2)
        nrm = np.hypot(xc[:, :, 0], xc[:, :, 1])
        on = (nrm > 0) & (np.abs(nrm - r) < 1e-6 * np.maximum(1.0, r)) & pick
        scale = np.where(on, np.maximum(r - delta, 0.0) / np.where(nrm > 0, nrm, 1.0), 1.0)
        x[:, :, 0] = (xc * scale[:, :, None]).reshape(B, N)
        return x
    pick = rng.random((B, N)) < 0.5
    delta = 10.0 ** rng.uniform(-9, -1.5, (B, N))
    xv = x[:, :, 0]
    if kind == "qp":
        x[:, :, 0] = np.where(pick & (xv == 0), delta, xv)
        return x
    lo, hi = np.asarray(d["l_min"])[:, :, 0], np.asarray(d["l_max"])[:, :, 0]
    x[:, :, 0] = np.where(pick & (xv <= lo), lo + delta, np.where(pick & (xv >= hi), hi - delta, xv))
    return x
