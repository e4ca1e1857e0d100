"""-m gpu: the persistent dense kernels of dqq_polish_path_f64 past their first trip through the batch (tests/path_trip_cases.py:
two full trips of every team and a ragged third).  A team keeps its slice and its registers where it found them -- the matrix
possibly left eliminated by its last problem's last stage, xc, the stage loop's counters --, and only the routine's own
re-initialisation and fences separate one problem from the next.  (The diagonal kernel is not persistent: a tile per wave.)
  1. the base alone is the host core's, bit for bit;
  2. every output of problem b of the B-problem call is problem b mod nb of the one-trip call, bit for bit;
  3. with a NaN in x of problem 1 and P[0,0] = inf in problem 4, both of the first trip: status 2 there, x kept, the launch
     returns and every other problem keeps the bits of (2)."""
import numpy as np
import pytest

import path_cases as PC
import path_trip_cases as TC
import test_gpu_path as G

pytestmark = pytest.mark.gpu
SCHEDULE = (PC.KAPPAS, PC.STEPS)       # the default one: on every row's base the problems end after three or more different step counts


def _same(what, got, ref, rows=None):
    for i, (g, r) in enumerate(zip(got, ref)):
        if rows is not None:
            g, r = g[rows], r[rows]
        if not (g.dtype == r.dtype and PC.same_bits(g, r)):
            bad = np.nonzero((g != r).reshape(g.shape[0], -1).any(1) & ~(np.isnan(g) & np.isnan(r)).reshape(g.shape[0], -1).all(1))[0]
            raise AssertionError("%s: %s differs on %d problems, first %s" % (what, G.NAMES[i], bad.size, bad[:3]))


@pytest.mark.parametrize("kind,N", TC.ROWS, ids=lambda v: str(v))
def test_every_team_solves_its_later_problems_as_its_first(kind, N):
    per, B, nb = TC.geometry(kind, N)
    assert B >= 2 * per + 1 and B % per != 0 and nb > 7
    P, q, ex, x = PC.problem(kind, N, nb, "dense")
    ref = G.host(kind, P, q, ex, x, G.DENSE, SCHEDULE)
    assert np.unique(ref[2]).size >= 3       # heterogeneous: the teams leave their problems after different numbers of steps
    try:
        one = G.path(kind, P, q, ex, x, G.DENSE, SCHEDULE)
        _same("the base alone against the host core", one, ref)
        idx = np.arange(B) % nb
        full = [np.ascontiguousarray(P[idx]), np.ascontiguousarray(q[idx]), tuple(np.ascontiguousarray(e[idx]) for e in ex),
                np.ascontiguousarray(x[idx])]
        many = G.path(kind, *full, G.DENSE, SCHEDULE)
        _same("all %d problems (per trip %d)" % (B, per), many, tuple(o[idx] for o in one))
        # poison in the first trip does not ride to the second and third
        full[3][TC.POISON_NAN, N // 2] = np.nan
        full[0][TC.POISON_INF, 0, 0] = np.inf
        bad = G.path(kind, *full, G.DENSE, SCHEDULE)
    except RuntimeError as e:   # a device fault: nothing more is started on this GPU
        pytest.exit("path trips %s N=%d: %s" % (kind, N, e), returncode=3)
    keep = np.ones(B, dtype=bool)
    rows = [TC.POISON_NAN, TC.POISON_INF]
    keep[rows] = False
    _same("beside the poisoned problems", bad, many, keep)
    assert list(bad[3][rows]) == [2, 2] and PC.same_bits(bad[0][rows], full[3][rows])
    assert not bad[2][rows].any() and not bad[4][rows].any() and not bad[6][rows].any()
