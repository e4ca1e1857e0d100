"""-m gpu: the persistent dense kernels of dqq_newton_jac_smooth_f64 past their first trip through the batch
(newton_jac_dense_smooth.hip: the LDS teams' grid is capped at 256 * 8 workgroups, the any-N form runs any_grid's 512; a team keeps
its slice where it found it, and only the routine's own re-initialisation and fences separate one problem from the next).  The
geometry is the hard Jacobian kernels' -- tests/newton_trip_cases.py's per_trip and batch_size for the entry "jac" -- since the
smoothed kernels launch with the same slice sizes.  (The diagonal kernel is not persistent: a tile per wave.)

Per row a heterogeneous base of trip_cases.base_size(N) problems (a prime number: a team meets other problems on its second trip
than on its first), tiled to B = 2 per_trip + 3: two full trips of every team and a ragged third.
  1. the base alone is the host core's, bit for bit;
  2. every output of problem b of the B-problem call is problem b mod nb of the one-trip call, bit for bit;
  3. with a NaN in x of problem 1 (first trip) and P[0,0] = inf in problem 4: status 2 and NaN there, the launch returns and every
     other problem keeps the bits of (2)."""
import numpy as np
import pytest

import jac_smooth_cases as C
import newton_trip_cases as T
import test_gpu_jac_smooth as G
from trip_cases import base_size

pytestmark = pytest.mark.gpu
KAPPA = C.KAPPA
# every width -- T = 8, 16, 32 (several waves per workgroup), 64 (one) -- and the any-N form, the kinds rotating
ROWS = [("box", 8), ("qcqp", 12), ("sbox", 20), ("qp", 64), ("qcqp", 66)]


def _same(what, got, ref, rows=None):
    for i, (g, r) in enumerate(zip(got, ref)):
        if g is None and r is None:
            continue
        if rows is not None:
            g, r = g[rows], r[rows]
        if not (g.dtype == r.dtype and C.same_bits(g, r)):
            bad = np.nonzero((g != r).reshape(g.shape[0], -1).any(1) & ~(np.isnan(g) & np.isnan(r)).reshape(g.shape[0], -1).all(1))[0]
            raise AssertionError("%s: output %d differs on %d problems, first %s" % (what, i, bad.size, bad[:3]))


@pytest.mark.parametrize("kind,N", ROWS, ids=lambda v: str(v))
def test_every_team_solves_its_later_problems_as_its_first(kind, N):
    per = T.per_trip("jac", kind, N)
    B, nb = T.batch_size(per), base_size(N)
    assert B >= 2 * per + 1 and B % per != 0 and nb > 7
    P, q, ex, x = C.problem(kind, N, nb, "dense")
    ref = C.host_jac(kind, P, q, ex, x, kappa=KAPPA)
    try:
        one = G.jac(kind, P, q, ex, x, G.DENSE, KAPPA)
        _same("the base alone against the host core", one, ref)
        idx = np.arange(B) % nb
        full = [np.ascontiguousarray(P[idx]), np.ascontiguousarray(q[idx]), tuple(np.ascontiguousarray(e[idx]) for e in ex),
                np.ascontiguousarray(x[idx])]
        many = G.jac(kind, *full, G.DENSE, KAPPA)
        _same("all %d problems (per trip %d)" % (B, per), many, tuple(None if o is None else o[idx] for o in one))
        # poison in the first trip does not ride to the second and third
        full[3][1, N // 2] = np.nan
        full[0][4, 0, 0] = np.inf
        bad = G.jac(kind, *full, G.DENSE, KAPPA)
    except RuntimeError as e:   # a device fault: nothing more is started on this GPU
        pytest.exit("smoothed Jacobian trips %s N=%d: %s" % (kind, N, e), returncode=3)
    keep = np.ones(B, dtype=bool)
    keep[[1, 4]] = False
    _same("beside the poisoned problems", bad, many, keep)
    assert list(bad[3][[1, 4]]) == [2, 2]
    for o in bad[:3]:
        assert o is None or np.isnan(o[[1, 4]]).all()
