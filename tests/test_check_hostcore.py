"""CPU check of the solution check's arithmetic (diffqcqp_amd/csrc/check_core.h), compiled for the host with the lanes of a
problem as an array (tests/hostcore/check_core_check.cpp), against the numpy restatement of the definitions
(tests/check_ref.py): status exactly, the four scalars within the bound derived there from the inputs."""
import numpy as np
import pytest

import check_ref as R

NS = (1, 2, 3, 8, 16, 17, 64, 65, 130)
CASES = [(k, N, d) for k in R.KINDS for N in NS for d in (False, True) if not (k == "qcqp" and N % 2)]


@pytest.fixture(scope="module")
def core():
    return R.hostcore()


def _check(core, kind, P, q, extras, x, iters=None, max_iter=0, diag=False):
    st, rs = R.host_check(core, kind, P, q, extras, x, iters, max_iter, diag)
    st0, rs0 = R.reference(kind, P, q, extras, x, iters, max_iter, diag)
    assert np.array_equal(st, st0), (st, st0)
    R.assert_close(rs, rs0, P, q, x, diag, "%s N=%d" % (kind, x.shape[1]))
    return st, rs


@pytest.mark.parametrize("kind,N,diag", CASES)
def test_core_matches_the_definitions(core, kind, N, diag):
    """A random x, and an x that is infeasible in every coordinate (below every lower bound, outside every disc)."""
    P, q, extras, x = R.make_batch(kind, 5, N, 100 + N, diag)
    st, rs = _check(core, kind, P, q, extras, x, diag=diag)
    assert (st == 0).all()
    st, rs = _check(core, kind, P, q, extras, -(1.0 + np.abs(x)), diag=diag)
    assert (st == 0).all() and (rs[:, 1] >= 1.0 - 0.9).all()


def _optimum(kind, B, N, seed):
    """A feasible optimum in closed form: diagonal P, the active set chosen first, q built from it.  -> (p, q, extras, x)."""
    r = np.random.default_rng(seed)
    p = r.uniform(0.1, 1.1, (B, N))
    slack = r.uniform(0.1, 1.0, (B, N))          # |g| on the active coordinates
    if kind == "qp":
        act = r.random((B, N)) < 0.5
        x = np.where(act, 0.0, r.uniform(0.1, 1.0, (B, N)))
        g = np.where(act, slack, 0.0)
        extras = ()
    elif kind in ("box", "sbox"):
        lo, hi = -r.uniform(0.5, 1.5, (B, N)), r.uniform(0.5, 1.5, (B, N))
        extras = (lo, hi)
        elo, ehi = lo, hi                         # the effective interval
        if kind == "sbox":
            v = r.uniform(-1.0, 1.0, (B, N))
            v[:, 0] = 0.0
            extras += (v,)
            elo, ehi = np.where(v >= 0, lo, 0.0), np.where(v <= 0, hi, 0.0)
            elo, ehi = np.where(v == 0, 0.0, elo), np.where(v == 0, 0.0, ehi)
        state = r.integers(0, 3, (B, N))          # 0 interior, 1 at the lower end, 2 at the upper end
        mid = elo + (ehi - elo) * r.uniform(0.25, 0.75, (B, N))
        x = np.where(state == 0, mid, np.where(state == 1, elo, ehi))
        g = np.where(state == 0, 0.0, np.where(state == 1, slack, -slack))
        g = np.where(elo == ehi, slack * np.where(state == 2, -1.0, 1.0), g)   # a pinned coordinate: any g
    else:
        ln, mu = r.uniform(0.2, 1.0, (B, N // 2)), r.uniform(0.2, 1.0, (B, N // 2))
        extras = (ln, mu)
        rad = ln * mu
        act = r.random((B, N // 2)) < 0.5         # contacts on the circle
        ang = r.uniform(0, 2 * np.pi, (B, N // 2))
        scale = np.where(act, rad, rad * r.uniform(0.1, 0.9, (B, N // 2)))
        x = np.empty((B, N))
        x[:, 0::2], x[:, 1::2] = scale * np.cos(ang), scale * np.sin(ang)
        lam = np.repeat(np.where(act, slack[:, : N // 2], 0.0), 2, axis=1)
        g = -lam * x                              # the gradient points into the disc along -x
    q = g - p * x
    return p, q, extras, x


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("N", (2, 8, 16, 64, 130))
def test_a_built_optimum_has_no_residual(core, kind, N):
    p, q, extras, x = _optimum(kind, 6, N, 7 + N)
    for diag in (True, False):
        P = p if diag else np.stack([np.diag(r) for r in p])
        st, rs = _check(core, kind, P, q, extras, x, diag=diag)
        b, _ = R.bounds(P, q, x, diag)
        assert (st == 0).all()
        assert (rs[:, 0] <= b).all(), "natural residual of an optimum: %s over the bound %s" % (rs[:, 0], b)
        assert (rs[:, 1] <= b).all(), "infeasibility of a feasible point"


@pytest.mark.parametrize("kind,N,diag", [c for c in CASES if c[1] in (3, 8, 17, 130)])
def test_non_finite_input_is_status_2(core, kind, N, diag):
    P, q, extras, x = R.make_batch(kind, 4, N, 300 + N, diag)
    x[1, N - 1] = np.nan                           # x with one NaN
    if diag:
        P[2, N // 2] = np.inf                      # P with one Inf
    else:
        P[2, N - 1, N // 2] = np.inf
    st, _ = _check(core, kind, P, q, extras, x, diag=diag)
    assert list(st) == [0, 2, 2, 0]


@pytest.mark.parametrize("kind,N,diag", [c for c in CASES if c[1] in (2, 8, 65)])
def test_iters_against_max_iter(core, kind, N, diag):
    P, q, extras, x = R.make_batch(kind, 6, N, 400 + N, diag)
    iters = np.array([9, 10, 11, -1, -1, 10], dtype=np.int32)   # below, at, above; -1 = could not be queued
    x[4] = np.nan                                  # ... whose x is NaN: status 2, as for problem 5's Inf
    x[5, 0] = np.inf
    st, _ = _check(core, kind, P, q, extras, x, iters, 10, diag=diag)
    assert list(st) == [0, 1, 1, 0, 2, 2]
    st, _ = _check(core, kind, P, q, extras, x, diag=diag)    # without iters nothing is capped
    assert list(st) == [0, 0, 0, 0, 2, 2]
