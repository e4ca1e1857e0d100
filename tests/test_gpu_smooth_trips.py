"""-m gpu: every persistent kernel of the smoothed Newton family past its first trip through the batch.  The dense routes of
dqq_polish_smooth_f64 and dqq_newton_{bwd,jvp}_smooth_f64 run a fixed grid over the batch (polish_dense_smooth.hip,
newton_dense_smooth.hip: the LDS teams' grid is capped at 256 * 8 workgroups, the any-N form runs any_grid's 512): a team keeps its
slice and its registers where it found them, and only the routine's own re-initialisation and fences separate one problem from the
next.  (The diagonal kernels are not persistent: a tile per wave.)  The geometry is the parents' -- tests/newton_trip_cases.py's
per_trip and batch_size, the functions tests/test_gpu_newton_trips.py takes it from; the smoothed kernels launch with the parents'
slice sizes (polish_team.h: polish_slice_doubles; newton_dense_smooth.hip: newton_smooth_slice_doubles).

Per row a heterogeneous base of trip_cases.base_size(N) cold-start problems (a prime number: a team meets other problems on its
second trip than on its first), tiled to B = 2 per_trip + 3: two full trips of every team and a ragged third.
  1. the base alone is the host core's, bit for bit;
  2. every output of problem b of the B-problem call is problem b mod nb of the one-trip call, bit for bit;
  3. with a NaN in x of problem 1 (first trip) and P[0,0] = inf in problem 4: status 2 there, x kept / NaN derivatives, the
     launch returns and every other problem keeps the bits of (2)."""
import numpy as np
import pytest
import torch

import newton_trip_cases as T
import smooth_cases as SC
import test_gpu_smooth as G
from trip_cases import base_size

pytestmark = pytest.mark.gpu
KAPPA = 1e-2
# (entry, the parent entry whose geometry it launches with, kind, N): every width -- T = 8, 32, 64 (four waves per workgroup at
# N = 34, one at N = 64), the any-N form and T = 16 (N = 12) --, the kinds rotating
ROWS = SC.TRIP_ROWS


def _tile(a, idx):
    return None if a is None else np.ascontiguousarray(a[idx])


def _call(entry, kind, P, q, ex, x, tang, N):
    dP, dq, da, db, gx = tang
    if entry == "polish":
        return G.polish(kind, P, q, ex, x, G.DENSE, KAPPA)
    if entry == "bwd":
        return G.backward(kind, P, q, ex, x, gx, G.DENSE, KAPPA)
    return G.jvp(kind, P, q, ex, x, (dP, dq, da, db), G.DENSE, KAPPA)


def _host(entry, kind, P, q, ex, x, tang):
    dP, dq, da, db, gx = tang
    if entry == "polish":
        return SC.host_polish(kind, P, q, ex, x, SC.MAX_STEPS, G.H, 0.0, KAPPA)
    if entry == "bwd":
        return SC.host_backward(kind, P, q, ex, x, gx, 0.0, KAPPA)
    return SC.host_jvp(kind, P, q, ex, x, dP, dq, da, db, 0.0, KAPPA)


def _same(what, got, ref, rows=None):
    for i, (g, r) in enumerate(zip(got, ref)):
        if g is None and r is None:
            continue
        if rows is not None:
            g, r = g[rows], r[rows]
        if not (g.dtype == r.dtype and SC.same_bits(g, r)):
            bad = np.nonzero((g != r).reshape(g.shape[0], -1).any(1) & ~(np.isnan(g) & np.isnan(r)).reshape(g.shape[0], -1).all(1))[0]
            raise AssertionError("%s: output %d differs on %d problems, first %s" % (what, i, bad.size, bad[:3]))


@pytest.mark.parametrize("entry,parent,kind,N", ROWS, ids=lambda v: str(v))
def test_every_team_solves_its_later_problems_as_its_first(entry, parent, kind, N):
    per = T.per_trip(parent, kind, N)
    B, nb = T.batch_size(per), base_size(N)
    assert B >= 2 * per + 1 and B % per != 0 and nb > 7
    P, q, ex, x = SC.problem(kind, N, nb, "dense")
    tang = SC.tangents(kind, N, nb, "dense")
    if entry != "polish":                       # the derivatives at the smoothed polish's point
        x = SC.host_polish(kind, P, q, ex, x, SC.MAX_STEPS, G.H, 0.0, KAPPA)[0]
    ref = _host(entry, kind, P, q, ex, x, tang)
    if entry == "polish":                       # heterogeneous: the teams leave their problems after different numbers of steps
        assert np.unique(ref[2]).size >= 3 and np.unique(ref[4]).size >= 2
    try:
        one = _call(entry, kind, P, q, ex, x, tang, N)
        _same("the base alone against the host core", one, ref)
        idx = np.arange(B) % nb
        full = [_tile(P, idx), _tile(q, idx), tuple(_tile(e, idx) for e in ex), _tile(x, idx), tuple(_tile(t, idx) for t in tang)]
        many = _call(entry, kind, *full, N)
        _same("all %d problems (per trip %d)" % (B, per), many, tuple(None if o is None else o[idx] for o in one))
        # poison in the first trip does not ride to the second and third
        full[3][1, N // 2] = np.nan
        full[0][4, 0, 0] = np.inf
        bad = _call(entry, kind, *full, N)
    except RuntimeError as e:   # a device fault: nothing more is started on this GPU
        pytest.exit("smoothed trips %s %s N=%d: %s" % (entry, kind, N, e), returncode=3)
    keep = np.ones(B, dtype=bool)
    keep[[1, 4]] = False
    _same("beside the poisoned problems", bad, many, keep)
    status = bad[3] if entry == "polish" else bad[-1]
    assert list(status[[1, 4]]) == [2, 2]
    if entry == "polish":
        assert SC.same_bits(bad[0][[1, 4]], full[3][[1, 4]]) and not bad[2][[1, 4]].any() and not bad[4][[1, 4]].any()
    else:
        for o in bad[:-1]:
            assert o is None or np.isnan(o[[1, 4]]).all()
