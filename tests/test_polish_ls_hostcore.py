"""CPU check of the damped polish's host core (diffqcqp_amd/csrc/polish_core.h: polish_problem_ls on one thread, behind
tests/hostcore/polish_ls_core_check.cpp, a stand-alone program; here its build with the address and undefined-behaviour
sanitizers, run directly) against the numpy restatement tests/polish_ls_reference.py: x_out, resid, steps, status and halvings
bit for bit on the frozen cold-start batches, the compact diagonal block form included.  The host build is a test artefact;
the product never calls it."""
import numpy as np
import pytest

import polish_ls_cases as C
import polish_ls_reference as L

HALVINGS = (0, 1, 8, 60)


def _equal(got, ref):
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype and C.same_bits(g, r), (g, r)


def _host(*a, **kw):
    """The sanitizer build -- and, the first time, that the plain build the device tests use gives its bits."""
    out = C.host_polish_ls(*a, sanitized=True, **kw)
    if not _host.compared:
        _host.compared = True
        _equal(C.host_polish_ls(*a, **kw), out)
    return out


_host.compared = False


@pytest.mark.parametrize("name,kind,N", L.ROWS)
def test_host_core_is_the_numpy_restatement_bit_for_bit(name, kind, N):
    P, q, ex, x = L.frozen(name, kind)
    for h in HALVINGS:
        ref = L.polish_ls_batch(kind, P, q, ex, x, L.MAX_STEPS, h)
        _equal(_host(kind, P, q, ex, x, L.MAX_STEPS, h), ref)
        if h in (0, 8):
            assert int(L.converged(P, q, ref).sum()) == L.COUNTS[name][h == 8]
        if "figure" in name:         # the block-by-block form on the compact diagonal: the general form's bits
            _equal(_host(kind, C.compact(P), q, ex, x, L.MAX_STEPS, h, diag=True), ref)
    _equal(_host(kind, P, q, ex, x, 5, 8, in_place=True), L.polish_ls_batch(kind, P, q, ex, x, 5, 8))
    _equal(_host(kind, P, q, ex, x, 5, 8, reg=1e-3), L.polish_ls_batch(kind, P, q, ex, x, 5, 8, 1e-3))
    _equal(_host(kind, P, q, ex, x, 0, 8), L.polish_ls_batch(kind, P, q, ex, x, 0, 8))


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("N", (2, 8))
def test_compact_diagonal_blocks(kind, N):
    P, q, ex, x = C.problem(kind, N, 24, "diag")
    for h in HALVINGS:
        ref = L.polish_ls_batch(kind, P, q, ex, x, 10, h)
        _equal(_host(kind, C.compact(P), q, ex, x, 10, h, diag=True), ref)
        _equal(_host(kind, P, q, ex, x, 10, h), ref)
    assert (ref[4].any() or kind in ("qp", "qcqp")) and (ref[3] == 0).sum() >= 12   # (a separable QP's full step is exact)


@pytest.mark.parametrize("kind,N", [("qp", 5), ("qcqp", 6), ("box", 5), ("sbox", 4)])
def test_non_finite_problems_keep_their_x(kind, N):
    P, q, ex, x = (np.array(a) if not isinstance(a, tuple) else tuple(np.array(e) for e in a) for a in C.problem(kind, N, 6, "dense"))
    x[1, N - 1] = np.nan
    P[2, 0, N - 1] = np.inf
    q[3, 0] = -np.inf
    ref = L.polish_ls_batch(kind, P, q, ex, x, 8, 8)
    assert list(ref[3][1:4]) == [2, 2, 2] and ref[3][0] == 0
    got = _host(kind, P, q, ex, x, 8, 8)
    _equal(got, ref)
    bad = ref[3] == 2
    assert C.same_bits(got[0][bad], x[bad]) and not got[2][bad].any() and not got[4][bad].any()
