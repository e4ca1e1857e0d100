"""csrc/newton_core.h's newton_jac_problem on one CPU thread (tests/hostcore/newton_jac_check.cpp, through ctypes) against the
numpy restatement tests/jac_reference.py, bit for bit: every kind, the compact block form against the full form on the same
diagonal given as (n,n), each output alone, and the statuses.  The same file as a stand-alone program under the address and
undefined-behaviour sanitizers is run once."""
import subprocess

import numpy as np
import pytest

import jac_cases as C
import jac_reference as JR
import newton_cases as NC
import polish_cases as PC

same = C.same_bits


@pytest.mark.parametrize("kind,N,structure", C.BATCHES)
def test_host_core_equals_the_restatement(kind, N, structure):
    P, q, ex, x = NC.problem(kind, N, structure)
    host = C.host_jac(kind, P, q, ex, x)
    ref = JR.jacobians_batch(kind, P, q, ex, x)
    nout = 1 if kind == "qp" else 3
    assert all(same(host[i], ref[i]) for i in range(nout)) and np.array_equal(host[3], ref[3]) and not host[3].any()
    if kind == "qp":
        assert host[1] is None and host[2] is None
    if structure == "diag":   # the block form on the compact diagonal: the full form's bits on the blocks, zeros elsewhere
        ch = C.host_jac(kind, PC.compact(P), q, ex, x, diag=True)
        assert np.array_equal(ch[3], host[3])
        for i in range(nout):
            assert same(ch[i], JR.compact(kind, host[i], i)), i
            assert (host[i][:, JR.off_block_mask(kind, N, i)] == 0.0).all(), i


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("structure", ["diag", "dense"])
def test_each_output_alone(kind, structure):
    P, q, ex, x = NC.problem(kind, 8, structure)
    for diag in ((False, True) if structure == "diag" else (False,)):
        Pa = PC.compact(P) if diag else P
        full = C.host_jac(kind, Pa, q, ex, x, diag=diag)
        for i in range(1 if kind == "qp" else 3):
            one = C.host_jac(kind, Pa, q, ex, x, tuple(j == i for j in range(3)), diag=diag, status=False)
            assert same(one[i], full[i]) and all(one[j] is None for j in range(3) if j != i)


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("structure", ["diag", "dense"])
def test_statuses_and_nan_outputs(kind, structure):
    N = 8
    P, q, ex, x = NC.problem(kind, N, structure)
    B = x.shape[0]
    P, q, x = P.copy(), q.copy(), x.copy()
    ex = tuple(e.copy() for e in ex)
    # status 1: P = 0 on a row at a coordinate that is free whatever the kind (tests/test_newton_hostcore.py)
    P[3, 0, :] = 0.0
    x[3, 0], q[3, 0] = 0.01, -0.01
    if kind == "qcqp":
        P[3, 1, :] = 0.0
        P[3, 1, 1] = 1.0
        x[3, 1], q[3, 1] = 0.0, 0.0
        ex[0][3, 0], ex[1][3, 0] = 1.0, 1.0
    elif kind != "qp":
        ex[0][3, 0], ex[1][3, 0] = -1.0, 1.0
        if kind == "sbox":
            ex[2][3, 0] = -1.0
    # status 2: NaN in q, NaN in P and x, an infinite bound
    P[5, 2, 2] = np.nan
    q[7, 1] = np.nan
    x[9, 0] = np.inf
    want = np.zeros(B, dtype=np.int32)
    want[3] = 1
    want[[5, 7, 9]] = 2
    if kind != "qp":
        ex[1][11, 0] = np.inf
        want[11] = 2
    for compact in ((False, True) if structure == "diag" else (False,)):
        out = C.host_jac(kind, PC.compact(P) if compact else P, q, ex, x, diag=compact)
        assert np.array_equal(out[3], want), out[3]
        for arr in out[:3]:
            if arr is not None:
                flat = arr.reshape(B, -1)
                assert np.isnan(flat[want != 0]).all() and np.isfinite(flat[want == 0]).all()
        if not compact:
            ref = JR.jacobians_batch(kind, P, q, ex, x)
            assert np.array_equal(out[3], ref[3]) and all(same(out[i], ref[i]) for i in range(3) if ref[i] is not None)


def test_sanitized_stand_alone_program_runs_clean():
    r = subprocess.run([C.hostcore_program()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "0 failures" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
