"""CPU check of the polish path's host core (diffqcqp_amd/csrc/path_core.h on one thread, behind
tests/hostcore/path_core_check.cpp, a stand-alone program with its own main; here its build with the address and
undefined-behaviour sanitizers, run directly as a program) against the numpy restatement tests/path_reference.py: every output bit
for bit on the frozen batches of tests/golden/smooth and on the cold-start batches of tests/golden/polish_ls, the compact diagonal
form included, in place and not.  The host build is a test artefact; the product never calls it."""
import numpy as np
import pytest

import path_cases as PC
import path_reference as PR
import polish_ls_reference as L
import smooth_cases as SC

SCHEDULES = ((PR.KAPPAS, PR.STEPS), PC.SHORT, PC.LONG, ((0.0,), (20,)), ((1e-2,), (12,)))


def _twice(*a, **kw):
    """The sanitizer build -- and, the first time, that the plain build the device tests use gives its bits."""
    out = PC.host_path(*a, sanitized=True, **kw)
    if not _twice.compared:
        _twice.compared = True
        PC.equal(PC.host_path(*a, **kw), out)
    return out


_twice.compared = False


@pytest.mark.parametrize("kind,structure", SC.ROWS)
def test_host_core_on_the_frozen_smooth_rows(kind, structure):
    P, q, ex, x, xh, _ = SC.frozen(kind, structure)
    for kappas, steps in SCHEDULES:
        for start in (x, xh):
            ref = PR.polish_path_batch(kind, P, q, ex, start, kappas, steps, 8, 0.0)
            PC.equal(_twice(kind, P, q, ex, start, kappas, steps, 8, 0.0), ref)
            PC.equal(_twice(kind, P, q, ex, start, kappas, steps, 8, 0.0, in_place=True), ref)
            if structure == "diag":          # the block-by-block form on the compact diagonal: the general form's bits
                PC.equal(_twice(kind, PC.compact(P), q, ex, start, kappas, steps, 8, 0.0, diag=True), ref)
                PC.equal(_twice(kind, PC.compact(P), q, ex, start, kappas, steps, 8, 0.0, diag=True, in_place=True), ref)
    kappas, steps = PC.SHORT
    PC.equal(_twice(kind, P, q, ex, x, kappas, steps, 0, 1e-3), PR.polish_path_batch(kind, P, q, ex, x, kappas, steps, 0, 1e-3))


@pytest.mark.parametrize("name,kind,N", L.ROWS)
def test_host_core_on_the_cold_start_batches(name, kind, N):
    P, q, ex, x = L.frozen(name, kind)
    for kappas, steps in (SCHEDULES[0], PC.SHORT):
        ref = PR.polish_path_batch(kind, P, q, ex, x, kappas, steps, 8, 0.0)
        PC.equal(_twice(kind, P, q, ex, x, kappas, steps, 8, 0.0), ref)
        if "figure" in name:
            PC.equal(_twice(kind, PC.compact(P), q, ex, x, kappas, steps, 8, 0.0, diag=True, in_place=True), ref)
    PC.equal(_twice(kind, P, q, ex, x, PC.SHORT[0], PC.SHORT[1], 8, 1e-3, in_place=True),
             PR.polish_path_batch(kind, P, q, ex, x, PC.SHORT[0], PC.SHORT[1], 8, 1e-3))


@pytest.mark.parametrize("kind,N", [("qp", 5), ("qcqp", 6), ("box", 5), ("sbox", 4)])
def test_non_finite_problems(kind, N):
    P, q, ex, x = (np.array(a) if not isinstance(a, tuple) else tuple(np.array(e) for e in a) for a in SC.problem(kind, N, 6, "dense"))
    x[1, N - 1] = np.nan
    P[2, 0, N - 1] = np.inf
    q[3, 0] = -np.inf
    if kind in ("box", "sbox"):
        ex[0][4, 0] = -np.inf            # one-sided boxes are not admitted by this entry
    ref = PR.polish_path_batch(kind, P, q, ex, x, *PC.SHORT)
    nbad = 4 if kind in ("box", "sbox") else 3
    assert list(ref[3][1:1 + nbad]) == [2] * nbad and ref[3][0] == 0
    got = _twice(kind, P, q, ex, x, *PC.SHORT)
    PC.equal(got, ref)
    bad = ref[3] == 2
    assert SC.same_bits(got[0][bad], x[bad]) and not got[2][bad].any() and not got[4][bad].any() and not got[6][bad].any()
