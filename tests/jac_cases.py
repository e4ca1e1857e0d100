"""Inputs and host-side yardsticks of the Newton-Jacobian tests -- tests/test_jac_*.py on the CPU, tests/test_gpu_jac*.py on the
device.  Not a test file.  Problems: newton_cases' (polish_cases' frozen batches at a polished x, and the built agreement
batches).  The yardstick of the kernels is the host core (tests/hostcore/newton_jac_check.cpp: csrc/newton_core.h's
newton_jac_problem on one CPU thread, loaded through ctypes), itself held bit-equal to the numpy restatement
tests/jac_reference.py."""
import ctypes
import functools
import os
import subprocess

import numpy as np

import jac_reference as JR
import newton_cases as NC
import newton_reference as NR
import polish_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = NC.KINDS
BATCHES = NC.BATCHES
# (kind, N, B) of tests/test_gpu_jac.py; the sizes and ragged_b are polish_cases'
DIAG_ROWS = NC.DIAG_ROWS
TEAM_ROWS = [(k, N, B) for k in KINDS for N in (2, 8, 20, 64) for B in (1, 67)] + [(k, NC.PC.TEAM_N16, 67) for k in KINDS]
ANY_ROWS = [(k, 66, B) for k in KINDS for B in (1, 67)]
ENTRIES = ("jac",)
_D = ctypes.POINTER(ctypes.c_double)
_I = ctypes.POINTER(ctypes.c_int)

# Both records: the largest figure over BATCHES (newton_cases.B_CPU problems each) per kind, of the numpy restatement alone, as
# measured, to two digits; tests/test_jac_reference.py measures them again and allows 16 x the record (what DESIGN.md 4.10 found
# necessary between hosts: numpy's solve is LAPACK's, whose last bits are the host's).  Both are relative to the check's scale
# (polish_reference.scale: resid[3] of dqq_check_f64, O(1) on these batches), per problem.
# SOLVE_GAP_CPU: max |Jq - (-solve(M, D))| / scale, numpy.linalg.solve on the restatement's own M and D.
SOLVE_GAP_CPU = {"qp": 7.4e-16, "qcqp": 1.8e-15, "box": 7.6e-16, "sbox": 4.9e-16}
# JAC_ADJOINT_CPU: |g'(Jq t) - grad_q't| / scale, grad_q newton_reference.backward's for the cotangent g; t and g standard normal
# (newton_cases.inputs), the products summed in index order.  The device tests hold ops.newton_jacobian_vjp / _jvp against the
# single-vector entries to 16 x this record of the scale, elementwise.
JAC_ADJOINT_CPU = {"qp": 2.6e-15, "qcqp": 1.8e-15, "box": 3.9e-15, "sbox": 1.8e-15}
BAR = 16


def _p(a):
    return None if a is None else a.ctypes.data_as(_D)


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


_DEPS = ("newton_core.h", "polish_core.h", "check_core.h", "sbox_bounds.h", "common.h")


@functools.lru_cache(maxsize=None)
def hostcore():
    """The host core as a shared library, built on demand (plain: the yardstick of the device tests too)."""
    src = os.path.join(HERE, "hostcore", "newton_jac_check.cpp")
    so = os.path.join(HERE, "hostcore", "libnewtonjaccheck.so")
    deps = [src] + [os.path.join(HERE, "..", "diffqcqp_amd", "csrc", f) for f in _DEPS]
    if not os.path.exists(so) or any(os.path.getmtime(p) > os.path.getmtime(so) for p in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fvisibility=hidden",
                               "-Wno-unknown-pragmas", "-o", so + ".tmp", src])
        os.replace(so + ".tmp", so)
    return ctypes.CDLL(so)


def hostcore_program():
    """The same file as a stand-alone program with the address and undefined-behaviour sanitizers -- CPU tests only."""
    src = os.path.join(HERE, "hostcore", "newton_jac_check.cpp")
    exe = os.path.join(HERE, "hostcore", "newton_jac_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                           "-ffp-contract=off", "-Wno-unknown-pragmas", "-DNEWTON_JAC_CHECK_MAIN", "-o", exe, src])
    return exe


def extra_cols(kind, N):
    return JR.extra_cols(kind, N)


def out_shapes(kind, B, N, diag):
    """Shapes of (Jq, Ja, Jb) as include/diffqcqp_hip.h has them (Ja, Jb None for the QP)."""
    ne = extra_cols(kind, N)
    if diag:
        s = ((B, N, 2) if kind == "qcqp" else (B, N), (B, N), (B, N))
    else:
        s = ((B, N, N), (B, N, ne), (B, N, ne))
    return s if kind != "qp" else (s[0], None, None)


def host_jac(kind, P, q, ex, x, need=(True, True, True), diag=False, status=True):
    """P (B,N,N), or (B,N) with diag; q, x (B,N); ex each (B,.) -> (Jq, Ja, Jb: None where not needed or the QP has none,
    status (B) int32)."""
    B, N = x.shape
    P, q, x = _c(P), _c(q), _c(x)
    assert P.shape == ((B, N) if diag else (B, N, N))
    ex = [_c(e) for e in ex] + [None] * (3 - len(ex))
    shapes = out_shapes(kind, B, N, diag)
    J = [np.full(s, 7.0) if s is not None and nd else None for s, nd in zip(shapes, need)]
    st = np.full(B, -1, dtype=np.int32)
    rc = hostcore().newton_jac_batch(R.KIND[kind], B, N, int(diag), _p(P), _p(q), _p(ex[0]), _p(ex[1]), _p(ex[2]), _p(x), _p(J[0]),
                                     _p(J[1]), _p(J[2]), st.ctypes.data_as(_I) if status else None)
    assert rc == 0
    return J[0], J[1], J[2], st


def unit_tangents(kind, B, N, which, j):
    """newton_reference.jvp_batch's (dP, dq, da, db) for the unit tangent e_j of input `which` (0 q, 1 a, 2 b)."""
    w = N if which == 0 else extra_cols(kind, N)
    e = np.zeros((B, w))
    e[:, j] = 1.0
    t = [None, None, None, None]
    t[1 + which] = e
    return tuple(t)


def solve_gap(kind, N, structure):
    """max over the batch of max |Jq - (-solve(M, D))| / scale."""
    P, q, ex, x = NC.problem(kind, N, structure)
    Jq = JR.jacobians_batch(kind, P, q, ex, x, (True, False, False))[0]
    scale = R.scale(P, q, x)
    worst = 0.0
    for b in range(x.shape[0]):
        exb = tuple(np.asarray(e[b]).reshape(-1) for e in ex)
        n, z, D, M = JR.setup(kind, P[b], q[b], exb, x[b])
        worst = max(worst, float(np.abs(Jq[b] + np.linalg.solve(M, D)).max()) / float(scale[b]))
    return worst


def dot_in_order(a, b):
    s = 0.0
    for u, v in zip(a, b):
        s = s + float(u) * float(v)
    return s


def adjoint_gap(kind, N, structure):
    """max over the batch of |g'(Jq t) - grad_q't| / scale."""
    P, q, ex, x = NC.problem(kind, N, structure)
    B = x.shape[0]
    tan, g = NC.inputs(kind, N, B, structure)
    t = tan[1]
    Jq = JR.jacobians_batch(kind, P, q, ex, x, (True, False, False))[0]
    gq = NR.backward_batch(kind, P, q, ex, x, g)[1]
    scale = R.scale(P, q, x)
    worst = 0.0
    for b in range(B):
        Jt = [dot_in_order(Jq[b, i], t[b]) for i in range(N)]
        worst = max(worst, abs(dot_in_order(g[b], Jt) - dot_in_order(gq[b], t[b])) / float(scale[b]))
    return worst


def same_bits(a, b):
    return NC.same_bits(a, b)
