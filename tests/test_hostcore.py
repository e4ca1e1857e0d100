"""CPU check of the per-problem math templates the HIP kernels instantiate
(diffqcqp_amd/csrc/admm_core.h, kkt_core.h), compiled for the host with one lane
per problem (tests/hostcore/host_core_check.cpp) and compared with the oracle.
The host build is a test artefact; the product never calls it."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import make_problem
from param_cases import nudge

HERE = os.path.dirname(os.path.abspath(__file__))
D = ctypes.POINTER(ctypes.c_double)


def _p(a):
    return a.ctypes.data_as(D)


@pytest.fixture(scope="module")
def hostcore():
    src = os.path.join(HERE, "hostcore", "host_core_check.cpp")
    so = os.path.join(HERE, "hostcore", "libhostcore.so")
    deps = [src] + [os.path.join(HERE, "..", "diffqcqp_amd", "csrc", f) for f in ("admm_core.h", "kkt_core.h", "bwd_systems.h",
                                                                                 "common.h", "admm_diag_prologue.inc",
                                                                                 "admm_diag_body.inc")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               "-fvisibility=hidden", "-o", so, src])
    return ctypes.CDLL(so)


# (eps, mu_prox, max_iter, adaptive): the defaults, and the solver parameters a caller can move off them
PARAMS = [(1e-7, 1e-7, 1000, 1), (1e-10, 1e-10, 1000, 0), (1e-10, 1e-5, 1000, 0), (1e-10, 1e-2, 1000, 0),
          (1e-7, 1e-10, 1000, 1), (1e-7, 1e-5, 1000, 1), (1e-5, 1e-2, 1000, 1)]


@pytest.mark.parametrize("kind,N,p_lo", [("qp", 8, 0.1), ("qp", 8, 0.0), ("qp", 16, 0.1), ("qp", 2, 0.1),
                                         ("qcqp", 8, 0.1), ("qcqp", 4, 0.1), ("qcqp", 16, 0.1)])
def test_forward_core_follows_oracle_trajectory(oracle, hostcore, kind, N, p_lo):
    B = 300
    d = make_problem(kind, B, N, 61 + N, p_lo=p_lo)
    P, q = d["P"].numpy(), d["q"].numpy()
    p = np.ascontiguousarray(np.diagonal(P, axis1=1, axis2=2))
    qq = np.ascontiguousarray(q[:, :, 0])
    rad = np.zeros((B, N // 2)) if kind == "qp" else np.ascontiguousarray((d["l_n"] * d["mu"]).numpy()[:, :, 0])
    for eps, mu_prox, max_iter, adaptive in PARAMS:
        if p_lo == 0.0 and mu_prox > 1e-7:
            continue   # P = diag(U(0, 1)): lambda_max >= 10 mu_prox is not certain beyond the default
        if kind == "qp":
            xo, ito = oracle.qp_fwd_batch(P, q, eps, max_iter, mu_prox=mu_prox, adaptive=adaptive)
        else:
            xo, ito = oracle.qcqp_fwd_batch(P, q, d["l_n"].numpy(), d["mu"].numpy(), eps, max_iter, mu_prox=mu_prox,
                                            adaptive=adaptive)
        xh, ith = np.zeros((B, N)), np.zeros(B, dtype=int)
        for b in range(B):
            ith[b] = hostcore.hostcore_fwd(0 if kind == "qp" else 1, N, _p(p[b]), _p(qq[b]), _p(rad[b]),
                                           ctypes.c_double(eps), ctypes.c_double(mu_prox), max_iter, adaptive, _p(xh[b]))
        assert np.array_equal(ith, ito), "rho schedule / stopping iteration must match the reference algorithm"
        assert (np.abs(xh - xo[:, :, 0]) / np.maximum(1.0, np.abs(xo[:, :, 0]))).max() < 1e-11


def test_backward_cores_are_bit_exact(oracle, hostcore):
    _backward_cores(oracle, hostcore, False, 1e-10)


@pytest.mark.parametrize("epsilon", [1e-10, 1e-6, 1e-4])
def test_backward_cores_are_bit_exact_on_nudged_x(oracle, hostcore, epsilon):
    """On nudged x (tests/param_cases.py), where the dual-recovery threshold epsilon decides the active set."""
    _backward_cores(oracle, hostcore, True, epsilon)


def _backward_cores(oracle, hostcore, nudged, epsilon):
    B, N = 400, 8
    d = make_problem("qcqp", B, N, 71)
    P, q, g = d["P"].numpy(), d["q"].numpy(), d["grad_x"].numpy()
    ln, mu = d["l_n"].numpy(), d["mu"].numpy()
    p = np.ascontiguousarray(np.diagonal(P, axis1=1, axis2=2))
    qq, gg = np.ascontiguousarray(q[:, :, 0]), np.ascontiguousarray(g[:, :, 0])
    dn = {k: v.numpy() for k, v in d.items()}
    # QP
    x, _ = oracle.qp_fwd_batch(P, q, 1e-7, 1000)
    if nudged:
        x = nudge("qp", dn, x, 72)
    gP, gq, st = oracle.qp_bwd_batch(P, q, x, g, epsilon=epsilon)
    xx = np.ascontiguousarray(x[:, :, 0])
    dl, sth = np.zeros((B, N)), np.zeros(B, dtype=int)
    for b in range(B):
        sth[b] = hostcore.hostcore_qp_bwd(N, _p(p[b]), _p(qq[b]), _p(xx[b]), _p(gg[b]), _p(dl[b]), ctypes.c_double(epsilon))
    assert np.array_equal(-dl, gq[:, :, 0]) and np.array_equal(sth, st)
    # QCQP (1-step and 3-step refinement exits both occur)
    x, _ = oracle.qcqp_fwd_batch(P, q, ln, mu, 1e-7, 1000)
    if nudged:
        x = nudge("qcqp", dn, x, 73)
    gP, gq, gl, gm, st = oracle.qcqp_bwd_batch(P, q, ln, mu, x, g, epsilon=epsilon)
    assert set(np.unique(st)) >= {1, 3}
    xx = np.ascontiguousarray(x[:, :, 0])
    l1, m1 = np.ascontiguousarray(ln[:, :, 0]), np.ascontiguousarray(mu[:, :, 0])
    gl2, gm2 = np.zeros((B, N // 2)), np.zeros((B, N // 2))
    for b in range(B):
        sth[b] = hostcore.hostcore_qcqp_bwd(N, _p(p[b]), _p(qq[b]), _p(l1[b]), _p(m1[b]), _p(xx[b]), _p(gg[b]),
                                            _p(dl[b]), _p(gl2[b]), _p(gm2[b]), ctypes.c_double(epsilon))
    assert np.array_equal(sth, st)
    assert np.array_equal(-dl, gq[:, :, 0])
    assert np.array_equal(gl2, gl[:, :, 0]) and np.array_equal(gm2, gm[:, :, 0])


@pytest.mark.parametrize("kind,N", [("box", 8), ("box", 2), ("box", 16), ("sbox", 8), ("sbox", 4)])
def test_box_forward_core_follows_oracle_trajectory(oracle, hostcore, kind, N):
    B = 300
    d = make_problem(kind, B, N, 161 + N)
    P, q = d["P"].numpy(), d["q"].numpy()
    lo, hi = d["l_min"].numpy(), d["l_max"].numpy()
    v = d["v"].numpy() if kind == "sbox" else None
    p = np.ascontiguousarray(np.diagonal(P, axis1=1, axis2=2))
    qq, l1, h1 = (np.ascontiguousarray(a[:, :, 0]) for a in (q, lo, hi))
    v1 = None if v is None else np.ascontiguousarray(v[:, :, 0])
    for eps, mu_prox, max_iter, adaptive in PARAMS:
        xo, ito = oracle.boxqp_fwd_batch(P, q, lo, hi, eps, max_iter, v=v, mu_prox=mu_prox, adaptive=adaptive)
        xh, ith = np.zeros((B, N)), np.zeros(B, dtype=int)
        for b in range(B):
            ith[b] = hostcore.hostcore_box_fwd(N, _p(p[b]), _p(qq[b]), _p(l1[b]), _p(h1[b]),
                                               None if v1 is None else _p(v1[b]), ctypes.c_double(eps),
                                               ctypes.c_double(mu_prox), max_iter, adaptive, _p(xh[b]))
        assert np.array_equal(ith, ito)
        assert (np.abs(xh - xo[:, :, 0]) / np.maximum(1.0, np.abs(xo[:, :, 0]))).max() < 1e-11


def test_box_backward_core_is_bit_exact(oracle, hostcore):
    """Per-coordinate blocks (1x1 / 2x2 dual, up to 3x3 derivative system, incl. pinned coordinates with both
    multipliers) against the oracle's dense (3N)^2 solve: identical bits, identical refinement exits."""
    _box_backward_core(oracle, hostcore, False, 1e-10)


@pytest.mark.parametrize("epsilon", [1e-10, 1e-6, 1e-4])
def test_box_backward_core_is_bit_exact_on_nudged_x(oracle, hostcore, epsilon):
    """The same on nudged x (tests/param_cases.py) at the dual-recovery thresholds epsilon a caller can pass."""
    _box_backward_core(oracle, hostcore, True, epsilon)


def _box_backward_core(oracle, hostcore, nudged, epsilon):
    B, N = 400, 8
    d = make_problem("box", B, N, 171)
    P, q, g = d["P"].numpy(), d["q"].numpy(), d["grad_x"].numpy()
    lo, hi = d["l_min"].numpy().copy(), d["l_max"].numpy().copy()
    x, _ = oracle.boxqp_fwd_batch(P, q, lo, hi, 1e-7, 1000)
    if nudged:
        x = nudge("box", {"l_min": lo, "l_max": hi}, x, 172)
    hi[::5, 2, 0] = lo[::5, 2, 0]          # pinned coordinates: both bounds active
    x[::5, 2, 0] = lo[::5, 2, 0]
    gP, gq, glo, ghi, gam, st = oracle.boxqp_bwd_batch(P, q, lo, hi, x, g, epsilon=epsilon)
    p = np.ascontiguousarray(np.diagonal(P, axis1=1, axis2=2))
    qq, gg, xx, l1, h1 = (np.ascontiguousarray(a[:, :, 0]) for a in (q, g, x, lo, hi))
    dl, gm, dg = np.zeros((B, N)), np.zeros((B, 2 * N)), np.zeros((B, 2 * N))
    sth = np.zeros((B, 2), dtype=np.int32)
    for b in range(B):
        hostcore.hostcore_box_bwd(N, _p(p[b]), _p(qq[b]), _p(l1[b]), _p(h1[b]), _p(xx[b]), _p(gg[b]), _p(dl[b]),
                                  _p(gm[b]), _p(dg[b]), sth[b].ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                  ctypes.c_double(epsilon))
    assert np.array_equal(sth, st)
    assert np.array_equal(-dl, gq[:, :, 0]) and np.array_equal(gm, gam)
    assert np.array_equal(-(dg[:, :N] * gm[:, :N]), glo[:, :, 0]) and np.array_equal(dg[:, N:] * gm[:, N:], ghi[:, :, 0])
