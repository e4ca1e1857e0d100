"""csrc/newton_core.h on one CPU thread (tests/hostcore/newton_core_check.cpp, through ctypes) against the numpy restatement
tests/newton_reference.py, bit for bit: every kind, both modes, the block form on a compact diagonal against the full form on the
same diagonal as (n,n), NULL tangents and NULL outputs, and the statuses.  The same file as a stand-alone program under the
address and undefined-behaviour sanitizers is run once."""
import subprocess

import numpy as np
import pytest

import newton_cases as C
import newton_reference as NR
import polish_cases as PC

same = C.same_bits


def _all_same(host, ref):
    return all(same(h, r) for h, r in zip(host, ref) if r is not None)


@pytest.mark.parametrize("kind,N,structure", C.BATCHES)
def test_host_core_equals_the_restatement(kind, N, structure):
    P, q, ex, x = C.problem(kind, N, structure)
    tan, g = C.inputs(kind, N, x.shape[0], structure)
    dx, sj = C.host_jvp(kind, P, q, ex, x, tan)
    rdx, rsj = NR.jvp_batch(kind, P, q, ex, x, *tan)
    assert same(dx, rdx) and np.array_equal(sj, rsj) and not sj.any()
    host = C.host_backward(kind, P, q, ex, x, g)
    ref = NR.backward_batch(kind, P, q, ex, x, g)
    assert _all_same(host, ref) and not host[4].any()
    if kind == "qp":
        assert host[2] is None and host[3] is None
    if structure == "diag":   # the block form on the compact diagonal: the same bits
        Pd, dPd = PC.compact(P), PC.compact(tan[0])
        cdx, csj = C.host_jvp(kind, Pd, q, ex, x, (dPd,) + tan[1:], diag=True)
        assert same(cdx, dx) and np.array_equal(csj, sj)
        ch = C.host_backward(kind, Pd, q, ex, x, g, diag=True)
        assert same(ch[0], PC.compact(host[0])) and _all_same(ch[1:], host[1:])


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("structure", ["diag", "dense"])
def test_null_tangents_and_null_outputs(kind, structure):
    N = 8
    P, q, ex, x = C.problem(kind, N, structure)
    B = x.shape[0]
    tan, g = C.inputs(kind, N, B, structure)
    diag = structure == "diag"
    Pa = PC.compact(P) if diag else P
    tana = ((PC.compact(tan[0]),) if diag else (tan[0],)) + tan[1:]
    full = C.host_jvp(kind, Pa, q, ex, x, tana, diag=diag)[0]
    for i in range(len(tana)):   # a NULL tangent is a zero tangent, bit for bit
        part = tuple(None if j == i else t for j, t in enumerate(tana))
        zeros = tuple(np.zeros_like(t) if j == i else t for j, t in enumerate(tana))
        assert same(C.host_jvp(kind, Pa, q, ex, x, part, diag=diag)[0], C.host_jvp(kind, Pa, q, ex, x, zeros, diag=diag)[0])
    none = C.host_jvp(kind, Pa, q, ex, x, (), diag=diag, status=False)[0]
    assert same(none, np.zeros_like(full)) or np.array_equal(none, np.zeros_like(full))
    whole = C.host_backward(kind, Pa, q, ex, x, g, diag=diag)
    for i in range(2 if kind == "qp" else 4):   # a single requested output equals the full call's
        need = tuple(j == i for j in range(4))
        one = C.host_backward(kind, Pa, q, ex, x, g, need, diag=diag, status=False)
        assert same(one[i], whole[i]) and all(one[j] is None for j in range(4) if j != i)


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("structure", ["diag", "dense"])
def test_statuses_and_nan_outputs(kind, structure):
    N = 8
    P, q, ex, x = C.problem(kind, N, structure)
    B = x.shape[0]
    tan, g = C.inputs(kind, N, B, structure)
    P, q, x, g = P.copy(), q.copy(), x.copy(), g.copy()
    ex = tuple(e.copy() for e in ex)
    tan = tuple(t.copy() for t in tan)
    # status 1: a zero row of P at a coordinate that is free whatever the kind (contact 0 inside its disc)
    P[3, 0, :] = 0.0
    x[3, 0], q[3, 0] = 0.01, -0.01          # z_0 = 0.02
    if kind == "qcqp":
        P[3, 1, :] = 0.0
        P[3, 1, 1] = 1.0
        x[3, 1], q[3, 1] = 0.0, 0.0
        ex[0][3, 0], ex[1][3, 0] = 1.0, 1.0
    elif kind != "qp":
        ex[0][3, 0], ex[1][3, 0] = -1.0, 1.0
        if kind == "sbox":
            ex[2][3, 0] = -1.0
    # status 2: NaN / Inf in P, q, x, an extra, the cotangent / a tangent
    P[5, 2, 2] = np.nan
    q[7, 1] = np.inf
    x[9, 0] = np.nan
    if kind != "qp":
        ex[1][11, 0] = np.inf           # an infinite bound / radius is such an entry
    gj, tj = g.copy(), tuple(t.copy() for t in tan)
    gj[13, 3] = np.nan
    tj[1][13, 3] = -np.inf
    want = np.zeros(B, dtype=np.int32)
    want[3] = 1
    want[[5, 7, 9, 13]] = 2
    if kind != "qp":
        want[11] = 2
    diag = structure == "diag"
    for compact in ((False, True) if diag else (False,)):
        Pa = PC.compact(P) if compact else P
        ta = ((PC.compact(tj[0]),) if compact else (tj[0],)) + tj[1:]
        dx, sj = C.host_jvp(kind, Pa, q, ex, x, ta, diag=compact)
        out = C.host_backward(kind, Pa, q, ex, x, gj, diag=compact)
        assert np.array_equal(sj, want) and np.array_equal(out[4], want), (sj, out[4])
        for arr in (dx,) + tuple(o for o in out[:4] if o is not None):
            flat = arr.reshape(B, -1)
            assert np.isnan(flat[want != 0]).all() and np.isfinite(flat[want == 0]).all()
        if not compact:
            rdx, rsj = NR.jvp_batch(kind, P, q, ex, x, *tj)
            ref = NR.backward_batch(kind, P, q, ex, x, gj)
            assert same(dx, rdx) and np.array_equal(sj, rsj) and _all_same(out, ref)


def test_sanitized_stand_alone_program_runs_clean():
    r = subprocess.run([C.hostcore_program()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "0 failures" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
