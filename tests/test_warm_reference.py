"""CPU: tests/warm_reference.py (the numpy restatement the warm GPU tests are held against) pinned to the oracle, and the
conditions on the restatement alone that keep those tests honest.

  * x0 = None: the oracle's iteration counts exactly and its x within 1e-12, on a 256-problem N = 8 batch per kind -- the
    oracle knows no warm start, so this is what ties the restatement's loop to it; the warm start changes the state at entry only;
  * on the GPU tests' own N = 8 batches (tests/warm_cases.py), diagonal and dense P, per kind:
      - x0 = the cold solution of q perturbed by 1 %: total warm iterations <= 0.85 x total cold iterations;
      - x0 = the problem's own cold solution: mean <= 4 iterations;
    (the measured figures are printed, and recorded in DESIGN.md 4.8)
  * max_iter = 0 returns x0; x0 = 0 is not the cold start."""
import numpy as np
import pytest

import warm_reference as W
from conftest import make_problem
from warm_cases import EXTRAS, extras_of, n8_rows, reference, row_id


def _oracle(O, kind, d, eps=1e-7, max_iter=1000):
    a = {k: v.numpy() for k, v in d.items()}
    if kind == "qp":
        return O.qp_fwd_batch(a["P"], a["q"], eps, max_iter, nthreads=8)
    if kind == "qcqp":
        return O.qcqp_fwd_batch(a["P"], a["q"], a["l_n"], a["mu"], eps, max_iter, nthreads=8)
    return O.boxqp_fwd_batch(a["P"], a["q"], a["l_min"], a["l_max"], eps, max_iter, v=a.get("v"), nthreads=8)


@pytest.mark.parametrize("kind", sorted(EXTRAS))
def test_cold_restatement_is_the_oracle(oracle, kind):
    d = make_problem(kind, 256, 8, 4100 + len(kind), "mixed")
    xo, ito = _oracle(oracle, kind, d)
    x, it = W.solve(kind, d["P"].numpy(), d["q"].numpy(), 1e-7, 1000, extras_of(kind, d))
    assert np.array_equal(it, ito), "iteration counts differ on %d problems" % int((it != ito).sum())
    assert np.abs(x - xo).max() <= 1e-12
    # and off the defaults: another eps, another mu_prox, no adaptation
    for kw, okw in ((dict(eps=1e-10), dict(eps=1e-10)),):
        xo, ito = _oracle(oracle, kind, d, **okw)
        x, it = W.solve(kind, d["P"].numpy(), d["q"].numpy(), kw["eps"], 1000, extras_of(kind, d))
        assert np.array_equal(it, ito) and np.abs(x - xo).max() <= 1e-12


@pytest.mark.parametrize("row", n8_rows(), ids=row_id)
def test_warm_start_saves_iterations_in_the_restatement(row):
    _, _, cold, out = reference(row)
    ratio = out["perturbed"][2].sum() / cold[1].sum()
    own = out["own"][2].mean()
    print("%s: cold mean %.2f its; perturbed-start / cold = %.3f; re-solve from own solution: mean %.2f (max %d)"
          % (row_id(row), cold[1].mean(), ratio, own, out["own"][2].max()))
    assert (cold[1] < 1000).all() and np.isfinite(cold[0]).all()
    assert ratio <= 0.85
    assert own <= 4.0
    for name in ("perturbed", "own", "zero", "infeasible"):   # every start converges (where to: the stopping rule's business)
        assert (out[name][2] < 1000).all() and np.isfinite(out[name][1]).all(), name


@pytest.mark.parametrize("kind", sorted(EXTRAS))
def test_start_state_consequences(kind):
    d = make_problem(kind, 64, 8, 77, "mixed")
    P, q, ex = d["P"].numpy(), d["q"].numpy(), extras_of(kind, d)
    x0 = np.random.default_rng(5).standard_normal(q.shape)
    x, it = W.solve(kind, P, q, 1e-7, 0, ex, x0=x0)
    assert np.array_equal(x, x0) and (it == 0).all()                    # max_iter = 0 returns x0
    xc, itc = W.solve(kind, P, q, 1e-7, 1, ex)
    xz, itz = W.solve(kind, P, q, 1e-7, 1, ex, x0=np.zeros_like(q))
    assert not np.array_equal(xc, xz)                                   # x0 = 0 is not the cold start (u = -q)
