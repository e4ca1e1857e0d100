"""CPU check of the general-P backward's set-up (diffqcqp_amd/csrc/bwd_systems.h: dual recovery, active sets and the entries of
the systems handed to iterative_refinement), run on one thread by tests/hostcore/bwd_systems_check.cpp and held bit-equal to
the oracle: the text the dense, any-size, small, lane and wave kernels call, on a machine without a GPU.  The host build is a
test artefact; the product never calls it."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import make_problem
from param_cases import KIND, nudge
from sbox_cases import effective_bounds

HERE = os.path.dirname(os.path.abspath(__file__))
D = ctypes.POINTER(ctypes.c_double)
I = ctypes.POINTER(ctypes.c_int)
B = 64


def _p(a):
    return None if a is None else a.ctypes.data_as(D)


@pytest.fixture(scope="module")
def bwdsys():
    src = os.path.join(HERE, "hostcore", "bwd_systems_check.cpp")
    so = os.path.join(HERE, "hostcore", "libbwdsystems.so")
    deps = [src] + [os.path.join(HERE, "..", "diffqcqp_amd", "csrc", f) for f in ("bwd_systems.h", "kkt_core.h", "sbox_bounds.h",
                                                                                 "common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               "-fvisibility=hidden", "-o", so, src])
    return ctypes.CDLL(so)


CASES = [("qp", 5), ("qp", 8), ("qcqp", 4), ("qcqp", 6), ("box", 3), ("box", 4), ("sbox", 3), ("sbox", 4)]
# (nudged, epsilon): the oracle's own x at the default threshold, then nudged x at the thresholds a caller can pass
INPUTS = [(False, 1e-10), (True, 1e-10), (True, 1e-6), (True, 1e-4)]
# nudged box cases (kind, N, epsilon) whose batch holds a problem without any multiplier (nn = 0): found once, asserted from
# then on.  nudge() moves coordinates off a bound, so it never gives a coordinate both multipliers; the count is printed.
NN_ZERO = {("box", 3, 1e-10), ("box", 3, 1e-6), ("box", 3, 1e-4), ("box", 4, 1e-10), ("sbox", 3, 1e-10), ("sbox", 3, 1e-6)}


# a case whose first seed left a test of the header one-sided (checked with the oracle alone): another seed
SEED = {("qcqp", 4): 31100}


def _seed(kind, N):
    return SEED.get((kind, N), 31000 + 100 * KIND[kind] + N)


@pytest.fixture(scope="module")
def forward(oracle):
    """(kind, N) -> (problem as numpy arrays, the oracle's forward x): computed once, shared, never modified."""
    out = {}
    for kind, N in CASES:
        d = {k: v.numpy() for k, v in make_problem(kind, B, N, _seed(kind, N), "dense").items()}
        if kind == "qp":
            x, _ = oracle.qp_fwd_batch(d["P"], d["q"], 1e-7, 1000)
        elif kind == "qcqp":
            x, _ = oracle.qcqp_fwd_batch(d["P"], d["q"], d["l_n"], d["mu"], 1e-7, 1000)
        else:
            x, _ = oracle.boxqp_fwd_batch(d["P"], d["q"], d["l_min"], d["l_max"], 1e-7, 1000, v=d.get("v"))
        x.setflags(write=False)
        out[(kind, N)] = (d, x)
    return out


def _oracle_backward(oracle, kind, d, x, epsilon):
    """-> dict of the oracle's backward outputs, by the batch calls of tests/test_hostcore.py: _backward_cores."""
    if kind == "qp":
        gP, gq, st = oracle.qp_bwd_batch(d["P"], d["q"], x, d["grad_x"], epsilon=epsilon)
        return {"grad_P": gP, "grad_q": gq[:, :, 0], "steps": st[:, None]}
    if kind == "qcqp":
        gP, gq, gl, gm, st, gam, dg = oracle.qcqp_bwd_batch(d["P"], d["q"], d["l_n"], d["mu"], x, d["grad_x"], epsilon=epsilon,
                                                            duals=True)
        return {"grad_P": gP, "grad_q": gq[:, :, 0], "g0": gl[:, :, 0], "g1": gm[:, :, 0], "gamma": gam[:, :, 0],
                "dgamma": dg[:, :, 0], "steps": st[:, None]}
    lo, hi = d["l_min"], d["l_max"]
    keep_lo = keep_hi = None
    if kind == "sbox":   # the box QP on the effective bounds; bound gradients only where the bound is still the caller's
        lo, hi, keep_lo, keep_hi = (t.numpy() for t in effective_bounds(*(torch.from_numpy(a) for a in (lo, hi, d["v"]))))
    gP, gq, glo, ghi, gam, st, dg = oracle.boxqp_bwd_batch(d["P"], d["q"], lo, hi, x, d["grad_x"], epsilon=epsilon, duals=True)
    if kind == "sbox":
        glo, ghi = np.where(keep_lo, glo, 0.0), np.where(keep_hi, ghi, 0.0)
    return {"grad_P": gP, "grad_q": gq[:, :, 0], "g0": glo[:, :, 0], "g1": ghi[:, :, 0], "gamma": gam, "dgamma": dg, "steps": st}


def _host_backward(bwdsys, kind, N, d, x, epsilon):
    """-> (the host build's outputs under the keys of _oracle_backward, stats summed over the batch)."""
    nm = {"qp": 0, "qcqp": N // 2, "box": N, "sbox": N}[kind]          # bound / contact gradients per problem
    ng = {"qp": 0, "qcqp": N // 2, "box": 2 * N, "sbox": 2 * N}[kind]  # multipliers per problem
    ns = 2 if kind in ("box", "sbox") else 1
    got = {"grad_P": np.zeros((B, N, N)), "grad_q": np.zeros((B, N)), "g0": np.zeros((B, nm)), "g1": np.zeros((B, nm)),
           "gamma": np.zeros((B, ng)), "dgamma": np.zeros((B, ng)), "steps": np.zeros((B, ns), dtype=np.int32)}
    stats = np.zeros((B, 6), dtype=np.int32)
    c = lambda a: np.ascontiguousarray(a.reshape(B, -1))   # noqa: E731
    q, g, xx = c(d["q"]), c(d["grad_x"]), c(x)
    a0, a1 = (c(d["l_n"]), c(d["mu"])) if kind == "qcqp" else (c(d["l_min"]), c(d["l_max"])) if kind != "qp" else (None, None)
    v = c(d["v"]) if kind == "sbox" else None
    for b in range(B):
        bwdsys.bwd_systems_check(KIND[kind], N, _p(d["P"][b]), _p(q[b]), None if a0 is None else _p(a0[b]),
                                 None if a1 is None else _p(a1[b]), None if v is None else _p(v[b]), _p(xx[b]), _p(g[b]),
                                 ctypes.c_double(epsilon), _p(got["grad_P"][b]), _p(got["grad_q"][b]), _p(got["g0"][b]),
                                 _p(got["g1"][b]), _p(got["gamma"][b]), _p(got["dgamma"][b]),
                                 got["steps"][b].ctypes.data_as(I), stats[b].ctypes.data_as(I))
    return got, stats.sum(axis=0)


@pytest.mark.parametrize("nudged,epsilon", INPUTS)
@pytest.mark.parametrize("kind,N", CASES)
def test_general_p_setup_is_bit_exact(oracle, bwdsys, forward, kind, N, nudged, epsilon):
    d, x = forward[(kind, N)]
    if nudged:
        x = nudge("box" if kind == "sbox" else kind, d, x, _seed(kind, N) + 1)
    ref = _oracle_backward(oracle, kind, d, x, epsilon)
    got, s = _host_backward(bwdsys, kind, N, d, x, epsilon)
    print("%s N=%d nudged=%d eps=%g: tests true/false %s, nn == 0: %d, both bounds: %d, steps %s"
          % (kind, N, nudged, epsilon, s[:4].tolist(), s[4], s[5], np.unique(ref["steps"]).tolist()))
    # both sides of every test of the header: the dual test and the active test (box kinds: lower and upper bound)
    assert (s[:4] > 0).all(), s[:4]
    if nudged and (kind, N, epsilon) in NN_ZERO:
        assert s[4] > 0 or s[5] > 0
    for k, r in ref.items():
        assert np.array_equal(got[k], r), k


@pytest.mark.parametrize("N", [3, 4])
def test_pinned_coordinates_have_both_multipliers(oracle, bwdsys, forward, N):
    """What nudge() never produces: l_min = l_max = x on a coordinate, so both of its multipliers exist (a two-column row of
    Id2, a rank-deficient dual system), as tests/test_hostcore.py pins them for the diagonal blocks."""
    d, x = forward[("box", N)]
    d, x = dict(d), x.copy()
    d["l_max"] = d["l_max"].copy()
    d["l_max"][::5, 1, 0] = d["l_min"][::5, 1, 0]
    x[::5, 1, 0] = d["l_min"][::5, 1, 0]
    ref = _oracle_backward(oracle, "box", d, x, 1e-10)
    got, s = _host_backward(bwdsys, "box", N, d, x, 1e-10)
    assert s[5] >= len(x[::5])
    for k, r in ref.items():
        assert np.array_equal(got[k], r), k
