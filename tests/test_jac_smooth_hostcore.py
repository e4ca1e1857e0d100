"""csrc/smooth_core.h's newton_jac_problem_smooth on one CPU thread (tests/hostcore/jac_smooth_core_check.cpp, through ctypes)
against the numpy restatement tests/jac_smooth_reference.py, bit for bit: dense N = 3 (4 for the QCQP) and 8, compact N = 2 and 8,
kappa in {0, 1e-4, 1e-2, 1}, every kind and every subset of outputs; a NaN and an Inf problem in the middle of the batch give
status 2 and NaN in their own rows only.  The same file as a stand-alone program runs plain and under the address and
undefined-behaviour sanitizers."""
import subprocess

import numpy as np
import pytest

import jac_smooth_cases as C
import jac_smooth_reference as JS
import reg_reference as RG

same = C.same_bits
B = 7


def _n(kind, N):
    return N + (N % 2 if kind == "qcqp" else 0)


@pytest.mark.parametrize("kappa", C.KAPPAS)
@pytest.mark.parametrize("form,N", [("dense", 3), ("dense", 8), ("compact", 2), ("compact", 8)])
@pytest.mark.parametrize("kind", C.KINDS)
def test_host_core_equals_the_restatement(kind, form, N, kappa):
    N = _n(kind, N)
    P, q, ex, x = C.problem(kind, N, B, "dense" if form == "dense" else "diag")
    P, q, ex, x = C.with_bad_rows(kind, P, q, ex, x, 2, 4)
    want = np.zeros(B, dtype=np.int32)
    want[[2, 4]] = 2
    for reg in C.REGS:
        full = JS.jacobians_batch(kind, P, q, ex, x, (True, True, True), reg, kappa)
        assert np.array_equal(full[3], want)
        for need in C.subsets(kind):
            host = C.host_jac(kind, C.compact(P) if form == "compact" else P, q, ex, x, need, diag=form == "compact", reg=reg, kappa=kappa)
            assert np.array_equal(host[3], want), (need, host[3])
            for i in range(3):
                if not need[i] or (kind == "qp" and i):
                    assert host[i] is None
                    continue
                ref = JS.compact(kind, full[i], i) if form == "compact" else full[i]
                assert same(host[i], ref), (need, i, reg)
                flat = host[i].reshape(B, -1)
                assert np.isnan(flat[want != 0]).all() and np.isfinite(flat[want == 0]).all()


@pytest.mark.parametrize("structure", ["dense", "diag"])
@pytest.mark.parametrize("kind", C.KINDS)
def test_kappa_zero_with_a_weight_is_the_hard_restatement_with_that_weight(kind, structure):
    """The run-time branch at reg > 0 against tests/reg_reference.py, the independent restatement of the hard family with a proximal
    weight (column by column through its own JVP); the compact form on the same diagonal given as (n,n)."""
    N = 8
    P, q, ex, x = C.problem(kind, N, B, structure)
    ref = RG.jacobian_batch(kind, P, q, ex, x, C.REG)
    assert not ref[3].any()
    host = C.host_jac(kind, P, q, ex, x, reg=C.REG, kappa=0.0)
    assert np.array_equal(host[3], ref[3])
    for i in range(1 if kind == "qp" else 3):
        assert same(host[i], ref[i]), i
    assert not same(host[0], C.host_jac(kind, P, q, ex, x, reg=0.0, kappa=0.0)[0])      # (the weight is looked at)
    if structure == "diag":
        ch = C.host_jac(kind, C.compact(P), q, ex, x, diag=True, reg=C.REG, kappa=0.0)
        for i in range(1 if kind == "qp" else 3):
            assert same(ch[i], JS.compact(kind, ref[i], i)), i


@pytest.mark.parametrize("sanitized", [False, True])
def test_stand_alone_program_runs_clean(sanitized):
    r = subprocess.run([C.hostcore_program(sanitized)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "0 failures" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
