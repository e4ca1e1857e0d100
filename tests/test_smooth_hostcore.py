"""CPU check of the smoothed Newton family's host core (diffqcqp_amd/csrc/smooth_core.h on one thread, behind
tests/hostcore/smooth_core_check.cpp, a stand-alone program; here its build with the address and undefined-behaviour sanitizers,
run directly) against the numpy restatement tests/smooth_reference.py: every output of the three entries bit for bit on the frozen
batches of tests/golden/smooth (the ones the measured tolerances belong to) and on the cold-start batches of tests/golden/polish_ls for kappa in {0, 1e-4, 1e-2, 1} and max_halvings in {0, 8}, the compact diagonal
block form included.  The host build is a test artefact; the product never calls it."""
import numpy as np
import pytest

import polish_ls_reference as L
import smooth_cases as SC
import smooth_reference as S

KAPPAS = (0.0, 1e-4, 1e-2, 1.0)
STEPS = 20


def _equal(got, ref):
    for g, r in zip(got, ref):
        assert (g is None and r is None) or (g.dtype == r.dtype and SC.same_bits(g, r)), (g, r)


def _twice(fn, *a, **kw):
    """The sanitizer build -- and, the first time per entry, that the plain build the device tests use gives its bits."""
    out = fn(*a, sanitized=True, **kw)
    if fn not in _twice.compared:
        _twice.compared.add(fn)
        _equal(fn(*a, **kw), out)
    return out


_twice.compared = set()


@pytest.mark.parametrize("name,kind,N", L.ROWS)
def test_host_core_is_the_numpy_restatement_bit_for_bit(name, kind, N):
    P, q, ex, x = L.frozen(name, kind)
    B = x.shape[0]
    dP, dq, da, db, gx = SC.tangents(kind, N, B, "diag" if "figure" in name else "dense")
    for kappa in KAPPAS:
        for h in (0, 8):
            ref = S.polish_batch(kind, P, q, ex, x, STEPS, h, 0.0, kappa)
            _equal(_twice(SC.host_polish, kind, P, q, ex, x, STEPS, h, 0.0, kappa), ref)
            if "figure" in name:         # the block-by-block form on the compact diagonal: the general form's bits
                _equal(_twice(SC.host_polish, kind, SC.compact(P), q, ex, x, STEPS, h, 0.0, kappa, diag=True), ref)
        xs = ref[0]
        reg = 1e-3 if kappa else 0.0     # (the hard derivatives with reg have a restatement of their own)
        rb = S.backward_batch(kind, P, q, ex, xs, gx, reg, kappa)
        rj = S.jvp_batch(kind, P, q, ex, xs, dP, dq, da, db, reg, kappa)
        _equal(_twice(SC.host_backward, kind, P, q, ex, xs, gx, reg, kappa), rb)
        _equal(_twice(SC.host_jvp, kind, P, q, ex, xs, dP, dq, da, db, reg, kappa), rj)
        if "figure" in name:
            got = _twice(SC.host_backward, kind, SC.compact(P), q, ex, xs, gx, reg, kappa, diag=True)
            _equal((got[0],) + got[1:], (SC.compact(rb[0]),) + rb[1:])
            _equal(_twice(SC.host_jvp, kind, SC.compact(P), q, ex, xs, SC.compact(dP), dq, da, db, reg, kappa, diag=True), rj)
    _equal(_twice(SC.host_polish, kind, P, q, ex, x, 5, 8, 1e-3, 1e-2, in_place=True), S.polish_batch(kind, P, q, ex, x, 5, 8, 1e-3, 1e-2))
    _equal(_twice(SC.host_polish, kind, P, q, ex, x, 0, 8, 0.0, 1e-2), S.polish_batch(kind, P, q, ex, x, 0, 8, 0.0, 1e-2))


@pytest.mark.parametrize("kind,structure", SC.ROWS)
def test_host_core_on_the_batches_the_records_are_taken_on(kind, structure):
    """tests/golden/smooth: from the cold start and from the frozen hard solution, the compact diagonal form where P is diagonal."""
    P, q, ex, x, xh, (dP, dq, da, db, gx) = SC.frozen(kind, structure)
    for kappa in KAPPAS:
        for h in (0, 8):
            for start in (x, xh):
                ref = S.polish_batch(kind, P, q, ex, start, STEPS, h, 0.0, kappa)
                _equal(_twice(SC.host_polish, kind, P, q, ex, start, STEPS, h, 0.0, kappa), ref)
                if structure == "diag":
                    _equal(_twice(SC.host_polish, kind, SC.compact(P), q, ex, start, STEPS, h, 0.0, kappa, diag=True), ref)
        xs = ref[0]
        _equal(_twice(SC.host_backward, kind, P, q, ex, xs, gx, 0.0, kappa), S.backward_batch(kind, P, q, ex, xs, gx, 0.0, kappa))
        _equal(_twice(SC.host_jvp, kind, P, q, ex, xs, dP, dq, da, db, 0.0, kappa), S.jvp_batch(kind, P, q, ex, xs, dP, dq, da, db, 0.0, kappa))


@pytest.mark.parametrize("kind,N", [("qp", 5), ("qcqp", 6), ("box", 5), ("sbox", 4)])
def test_non_finite_problems(kind, N):
    P, q, ex, x = (np.array(a) if not isinstance(a, tuple) else tuple(np.array(e) for e in a) for a in SC.problem(kind, N, 6, "dense"))
    dP, dq, da, db, gx = SC.tangents(kind, N, 6, "dense")
    x[1, N - 1] = np.nan
    P[2, 0, N - 1] = np.inf
    q[3, 0] = -np.inf
    if kind in ("box", "sbox"):
        ex[0][4, 0] = -np.inf            # one-sided boxes are not admitted under smoothing
    ref = S.polish_batch(kind, P, q, ex, x, 8, 8, 0.0, 1e-2)
    nbad = 4 if kind in ("box", "sbox") else 3
    assert list(ref[3][1:1 + nbad]) == [2] * nbad and ref[3][0] == 0
    got = _twice(SC.host_polish, kind, P, q, ex, x, 8, 8, 0.0, 1e-2)
    _equal(got, ref)
    bad = ref[3] == 2
    assert SC.same_bits(got[0][bad], x[bad]) and not got[2][bad].any() and not got[4][bad].any()
    rb = S.backward_batch(kind, P, q, ex, x, gx, 0.0, 1e-2)
    _equal(_twice(SC.host_backward, kind, P, q, ex, x, gx, 0.0, 1e-2), rb)
    _equal(_twice(SC.host_jvp, kind, P, q, ex, x, dP, dq, da, db, 0.0, 1e-2), S.jvp_batch(kind, P, q, ex, x, dP, dq, da, db, 0.0, 1e-2))
    assert list(rb[4][bad]) == [2] * nbad and np.isnan(rb[1][bad]).all() and np.isfinite(rb[1][~bad]).all()
