"""Inputs and host-side yardsticks of the forward-mode (JVP) tests -- tests/test_jvp_*.py on the CPU, tests/test_gpu_jvp.py on
the device.  Not a test file.  Problems: make_problem's families with every P re-conditioned by warm_cases.well_conditioned
(condition number <= 4), solved by the oracle at eps = 1e-10; the derivative threshold is epsilon = 1e-10.  The yardstick of
the kernels is the host core (tests/hostcore/jvp_check.cpp: the product's own bwd_systems.h helpers on one CPU thread), itself
held bit-equal to the numpy restatement tests/jvp_reference.py."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np

import jvp_reference as R
from conftest import make_problem
from warm_cases import well_conditioned

HERE = os.path.dirname(os.path.abspath(__file__))
D = ctypes.POINTER(ctypes.c_double)
I = ctypes.POINTER(ctypes.c_int)
EPS_FWD, MAX_ITER, EPSILON = 1e-10, 100000, 1e-10
EXTRAS = {"qp": (), "qcqp": ("l_n", "mu"), "box": ("l_min", "l_max"), "sbox": ("l_min", "l_max", "v")}


def _p(a):
    return None if a is None else a.ctypes.data_as(D)


@functools.lru_cache(maxsize=None)
def hostcore():
    src = os.path.join(HERE, "hostcore", "jvp_check.cpp")
    so = os.path.join(HERE, "hostcore", "libjvpcheck.so")
    deps = [src, os.path.join(HERE, "hostcore", "bwd_systems_check.cpp")]
    deps += [os.path.join(HERE, "..", "diffqcqp_amd", "csrc", f) for f in ("bwd_systems.h", "kkt_core.h", "sbox_bounds.h", "common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fvisibility=hidden",
                               "-o", so + ".tmp", src])
        os.replace(so + ".tmp", so)
    return ctypes.CDLL(so)


def seed_of(kind, N, structure):
    return 52000 + 1000 * R.KIND[kind] + 10 * N + (structure == "diag")


@functools.lru_cache(maxsize=None)
def problem(kind, N, B, structure="dense"):
    """-> (d: make_problem's dict as read-only numpy arrays, P well conditioned; x: the oracle's solution (B,N,1))."""
    from oracle import oracle as O
    O.build()
    t = make_problem(kind, B, N, seed_of(kind, N, structure), structure)
    t["P"] = well_conditioned(t["P"])
    d = {k: np.ascontiguousarray(v.numpy()) for k, v in t.items()}
    if kind == "qp":
        x, _ = O.qp_fwd_batch(d["P"], d["q"], EPS_FWD, MAX_ITER)
    elif kind == "qcqp":
        x, _ = O.qcqp_fwd_batch(d["P"], d["q"], d["l_n"], d["mu"], EPS_FWD, MAX_ITER)
    else:
        x, _ = O.boxqp_fwd_batch(d["P"], d["q"], d["l_min"], d["l_max"], EPS_FWD, MAX_ITER, v=d.get("v"))
    for a in list(d.values()) + [x]:
        a.setflags(write=False)
    return d, x


def host_jvp(kind, d, x, tangents, epsilon=EPSILON):
    """The host core over a batch.  tangents: (dP (B,N,N), dq (B,N)[, da, db]), None entries = NULL -> (dx (B,N), steps)."""
    lib = hostcore()
    P, q, ex = R.flat(d, kind)
    B, N = q.shape
    xx = np.ascontiguousarray(x.reshape(B, N))
    tangents = tuple(tangents) + (None,) * (4 - len(tangents))
    tangents = [None if t is None else np.ascontiguousarray(t, dtype=np.float64) for t in tangents]
    ex = [np.ascontiguousarray(e) for e in ex] + [None] * (3 - len(ex))
    dx = np.zeros((B, N))
    steps = np.zeros((B, 2 if kind in ("box", "sbox") else 1), dtype=np.int32)
    row = lambda a, b: None if a is None else _p(a[b])   # noqa: E731
    for b in range(B):
        lib.jvp_check(R.KIND[kind], N, _p(np.ascontiguousarray(P[b])), _p(q[b]), row(ex[0], b), row(ex[1], b), row(ex[2], b),
                      _p(xx[b]), row(tangents[0], b), row(tangents[1], b), row(tangents[2], b), row(tangents[3], b),
                      ctypes.c_double(epsilon), _p(dx[b]), steps[b].ctypes.data_as(I))
    return dx, steps


# ---- the adjoint identity <g, dx> = sum <grad, tangent> ----------------------------------------------------------------------
# Backward and JVP return Tikhonov iterates of A^T b = rhs and A w = s (mu_ir = 1e-7, 1 or 3 bodies): regularised by A A^T and
# by A^T A, truncated alike, so the identity holds to the refinement's accuracy only.  ADJOINT_GAP_CPU: the largest relative gap
# of the numpy restatement's two modes on ADJOINT_BATCHES, as measured, to two digits (tests/test_jvp_reference.py measures it
# again and holds the record to exactly those digits); the GPU tests allow 10 x the record.  The gap is normalised by the sum
# of the absolute terms, so it cannot exceed 1: at 10 x the QCQP's and the signed box QP's bars catch a wrong sign or a
# misplaced row, not a small error -- what pins the values is the bit-equality with the host core.  QP: the system is symmetric, the gap is rounding.  QCQP: the
# cone rows put singular values of 1e-3 .. 1e-2 into A, where one body of the refinement is off by percents -- in each mode.
ADJOINT_BATCHES = ((8, 37, "dense"), (8, 67, "diag"), (3, 37, "dense"), (4, 37, "dense"))
ADJOINT_GAP_CPU = {"qp": 3.9e-16, "qcqp": 0.054, "box": 2.6e-4, "sbox": 0.060}


def adjoint_inputs(kind, N, B, structure):
    """-> (tangents as jvp_reference.random_tangents, g (B,N)) of a batch: seeded, shared by the CPU and GPU tests."""
    seed = 99 + seed_of(kind, N, structure)
    return R.random_tangents(kind, B, N, seed, diag=structure == "diag"), np.random.default_rng(seed + 1).standard_normal((B, N))


def adjoint_gap(g, dx, grads, tangents):
    """Largest over the batch of |<g, dx> - sum <grad, tangent>| / sum |terms|; every array (B, ...); exactly rounded sums."""
    worst = 0.0
    for b in range(g.shape[0]):
        lhs = (g[b] * dx[b]).ravel()
        rhs = np.concatenate([(a[b] * t[b]).ravel() for a, t in zip(grads, tangents)])
        scale = math.fsum(np.abs(lhs)) + math.fsum(np.abs(rhs))
        if scale > 0:   # (a QP with every coordinate at its bound: both sides are exact zeros)
            worst = max(worst, abs(math.fsum(lhs) - math.fsum(rhs)) / scale)
    return worst


def adjoint_gap_cpu(kind, N, B, structure):
    if kind == "qcqp" and N % 2:
        N += 1
    d, x = problem(kind, N, B, structure)
    P, q, ex = R.flat(d, kind)
    tan, g = adjoint_inputs(kind, N, B, structure)
    dx, grads = [], []
    for b in range(B):
        exb = tuple(e[b] for e in ex)
        bw = R.derivative(kind, P[b], q[b], exb, x[b, :, 0], EPSILON, "bwd", g=g[b])
        dx.append(R.derivative(kind, P[b], q[b], exb, x[b, :, 0], EPSILON, "jvp", tangents=tuple(t[b] for t in tan))["dx"])
        grads.append([bw["grad_P"], bw["grad_q"]] + ([bw["g0"], bw["g1"]] if kind != "qp" else []))
    return adjoint_gap(g, np.stack(dx), [np.stack(c) for c in zip(*grads)], tan)
