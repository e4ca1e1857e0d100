"""CPU checks of the host core with the proximal weight (tests/hostcore/reg_core_check.cpp: csrc/polish_core.h and
csrc/newton_core.h on one thread): bit-equal to the numpy restatement tests/reg_reference.py at every weight, bit-equal to the
parents' host cores at reg = 0, and clean under the address and undefined-behaviour sanitizers as a stand-alone program."""
import subprocess

import numpy as np
import pytest

import newton_cases as NC
import polish_cases as PC
import polish_reference as R
import reg_cases as C
import reg_reference as RR

BATCHES = [(k, 8, m) for k in C.KINDS for m in C.MODES] + [(k, 20, "lowrank") for k in C.KINDS]


def test_program_under_sanitizers():
    out = subprocess.run([C.hostcore_program()], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "reg_core_check: 0 failures" in out.stdout


@pytest.mark.parametrize("kind,N,mode", BATCHES)
@pytest.mark.parametrize("reg", (0.0,) + C.REGS)
def test_host_core_is_the_restatement(kind, N, mode, reg):
    d = C.batch(kind, N, mode)
    P, q, ex, x = d["P"], d["q"], d["ex"], d["x"]
    tan, g = C.inputs(kind, N, C.B)
    dx, sj = C.host_jvp(kind, P, q, ex, x, tan, reg)
    want = RR.jvp_batch(kind, P, q, ex, x, *tan, reg=reg)
    assert C.same_bits(dx, want[0]) and np.array_equal(sj, want[1])
    got = C.host_backward(kind, P, q, ex, x, g, reg)
    want = RR.backward_batch(kind, P, q, ex, x, g, reg=reg)
    assert all(C.same_bits(a, b) for a, b in zip(got[:4], want[:4])) and np.array_equal(got[4], want[4])
    x0 = np.stack([R.project(kind, x[b] + 1e-3 * np.sin(np.arange(N) + b), tuple(e[b] for e in ex), N) for b in range(C.B)])
    got = C.host_polish(kind, P, q, ex, x0, 8, reg)
    want = RR.polish_batch(kind, P, q, ex, x0, 8, reg=reg)
    assert C.same_bits(got[0], want[0]) and C.same_bits(got[1], want[1])
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    if N == 8:
        got = C.host_jacobian(kind, P, q, ex, x, reg)
        want = RR.jacobian_batch(kind, P, q, ex, x, reg=reg)
        assert all(C.same_bits(a, b) for a, b in zip(got[:3], want[:3])) and np.array_equal(got[3], want[3])
    if mode == "diagzero":     # the compact diagonal: the general elimination's bits
        assert C.same_bits(C.host_jvp(kind, d["pdiag"], q, ex, x, (None,) + tuple(tan[1:]), reg, diag=True)[0],
                           C.host_jvp(kind, P, q, ex, x, (None,) + tuple(tan[1:]), reg)[0])
        assert C.same_bits(C.host_polish(kind, d["pdiag"], q, ex, x0, 8, reg, diag=True)[0], C.host_polish(kind, P, q, ex, x0, 8, reg)[0])


@pytest.mark.parametrize("kind,N,structure", NC.BATCHES)
def test_reg_zero_is_the_parents_host_core(kind, N, structure):
    """On newton_cases' inputs (polish_cases' golden batches): the new arguments at their defaults change no bit."""
    P, q, ex, x = NC.problem(kind, N, structure)
    tan, g = NC.inputs(kind, N, x.shape[0], structure)
    diag = structure == "diag"
    Pc = np.ascontiguousarray(np.einsum("bii->bi", P)) if diag else P
    tc = ((np.ascontiguousarray(np.einsum("bii->bi", tan[0])),) + tuple(tan[1:])) if diag else tan
    assert C.same_bits(C.host_jvp(kind, Pc, q, ex, x, tc, 0.0, diag)[0], NC.host_jvp(kind, Pc, q, ex, x, tc, diag)[0])
    for a, b in zip(C.host_backward(kind, Pc, q, ex, x, g, 0.0, diag)[:4], NC.host_backward(kind, Pc, q, ex, x, g, diag=diag)[:4]):
        assert C.same_bits(a, b)
    d, x0 = PC.frozen(kind, N, structure)
    x0 = np.ascontiguousarray(x0[:, :, 0])
    want = PC.host_polish(kind, Pc, q, ex, x0, diag=diag)
    got = C.host_polish(kind, Pc, q, ex, x0, PC.MAX_STEPS, 0.0, diag)
    assert C.same_bits(got[0], want[0]) and C.same_bits(got[1], want[1]) and np.array_equal(got[2], want[2])
