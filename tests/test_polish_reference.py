"""CPU checks of the polish's definition as tests/polish_reference.py restates it: monotone, exact where it keeps x, and
reaching machine-precision KKT from the oracle's early-stopped forwards on well-conditioned batches and on the reference's
figure workload.  RESIDUAL_CPU of tests/polish_cases.py is measured here again."""
import numpy as np
import pytest

import polish_cases as C
import polish_reference as R


def _has_polish():
    """The feature these tests belong to: the C ABI declares the entry point."""
    from diffqcqp_amd import _capi
    return "dqq_polish_f64" in _capi.SIGNATURES


@pytest.fixture(scope="module")
def results(oracle):
    """Every batch of C.BATCHES, as frozen under tests/golden/polish, polished once by the restatement:
    {batch: (P, q, ex, x, x_out, resid, steps, status)}."""
    assert _has_polish()
    out = {}
    for kind, N, structure in C.BATCHES:
        d, x = C.frozen(kind, N, structure)
        P, q, ex = C.flat(d, kind)
        x = x[:, :, 0]
        out[(kind, N, structure)] = (P, q, ex, x) + R.polish_batch(kind, P, q, ex, x, C.MAX_STEPS)
    return out


def _relative(P, q, x, resid):
    return resid[:, 1] / R.scale(P, q, x)


@pytest.mark.parametrize("batch", C.BATCHES, ids=lambda b: "%s-%d-%s" % b)
def test_polish_reaches_the_bar_and_never_makes_a_point_worse(results, batch):
    P, q, ex, x, xo, resid, steps, status = results[batch]
    assert (resid[:, 1] <= resid[:, 0]).all()
    kept = status == 1
    assert np.array_equal(xo[kept].view(np.int64), x[kept].view(np.int64)) and (steps[kept] == 0).all()
    assert ((status == 0) == (steps > 0)).all() and (steps <= C.MAX_STEPS).all()
    rel = _relative(P, q, xo, resid)
    print("%s: before %.1e .. %.1e, after max %.2e, steps max %d" % (
        batch, (resid[:, 0] / R.scale(P, q, x)).min(), (resid[:, 0] / R.scale(P, q, x)).max(), rel.max(), steps.max()))
    assert (rel <= C.BAR).all(), rel.max()
    # every accepted point is a projected point: inside the box exactly; on a disc, whose projection rounds (a scaling by
    # rad / |z|: three roundings), within 4 ulp of the radius
    kind, N, _ = batch
    for b in np.nonzero(status == 0)[0]:
        exb = tuple(e[b] for e in ex)
        if kind == "qcqp":
            assert (np.hypot(xo[b, 0::2], xo[b, 1::2]) <= exb[0] * exb[1] * (1 + 4 * 2.0 ** -52)).all()
        else:
            assert np.array_equal(R.project(kind, xo[b], exb, N), xo[b])


def test_the_recorded_residual_is_the_measured_one(results, oracle):
    worst = max(_relative(P, q, xo, resid).max() for P, q, ex, x, xo, resid, steps, status in results.values())
    d, x = C.frozen("qp", 8, "figure")
    P, q, _ = C.flat(d, "qp")
    xo, resid, steps, status = R.polish_batch("qp", P, q, (), x[:, :, 0], C.MAX_STEPS)
    worst = max(worst, _relative(P, q, xo, resid).max())
    assert float("%.1e" % worst) == C.RESIDUAL_CPU, "measured %.3e, recorded %.1e" % (worst, C.RESIDUAL_CPU)


def test_figure_workload_from_twenty_iterations(oracle):
    assert _has_polish()
    d, x = C.frozen("qp", 8, "figure")
    P, q, _ = C.flat(d, "qp")
    x = x[:, :, 0]
    xo, resid, steps, status = R.polish_batch("qp", P, q, (), x, C.MAX_STEPS)
    rel = _relative(P, q, xo, resid)
    print("figure workload: before max %.1e, after max %.2e, steps max %d" % ((resid[:, 0] / R.scale(P, q, x)).max(), rel.max(), steps.max()))
    assert (resid[:, 1] <= resid[:, 0]).all() and (rel <= C.BAR).all(), rel.max()


@pytest.mark.parametrize("kind", C.KINDS)
def test_ill_conditioned_rough_start_is_monotone(oracle, kind):
    """Condition number about 60, ten iterations of the forward: polish is a local method and no share of the batch is
    demanded -- only that nothing gets worse and that a problem that converged says so."""
    assert _has_polish()
    d, x = C.ill_conditioned(kind, 8, C.B_CPU)
    P, q, ex = C.flat(d, kind)
    x = x[:, :, 0]
    xo, resid, steps, status = R.polish_batch(kind, P, q, ex, x, C.MAX_STEPS)
    assert (resid[:, 1] <= resid[:, 0]).all() and np.isin(status, (0, 1)).all()
    converged = (resid[:, 1] / R.scale(P, q, xo) <= C.BAR) & (resid[:, 0] / R.scale(P, q, x) > C.BAR)
    print("%s: %d of %d converged" % (kind, converged.sum(), len(converged)))
    assert (status[converged] == 0).all()
    kept = status == 1
    assert np.array_equal(xo[kept].view(np.int64), x[kept].view(np.int64))


@pytest.mark.parametrize("batch", C.BATCHES, ids=lambda b: "%s-%d-%s" % b)
def test_a_polished_batch_is_a_fixed_point(results, batch):
    P, q, ex, x, xo, resid, steps, status = results[batch]
    xo2, resid2, steps2, status2 = R.polish_batch(batch[0], P, q, ex, xo, C.MAX_STEPS)
    assert np.array_equal(xo2.view(np.int64), xo.view(np.int64))
    assert ((status2 == 1) | (resid2[:, 0] == 0.0)).all() and (steps2 == 0).all()
    assert np.array_equal(resid2[:, 0], resid[:, 1]) and np.array_equal(resid2[:, 1], resid[:, 1])


def test_max_steps_zero_and_non_finite_inputs():
    assert _has_polish()
    r = np.random.default_rng(3)
    P = np.eye(4) + 0.1
    q, x = r.standard_normal(4), np.abs(r.standard_normal(4))
    xo, resid, steps, status = R.polish("qp", P, q, (), x, 0)
    assert np.array_equal(xo, x) and steps == 0 and status == 1 and resid[0] == resid[1]
    for bad in (np.nan, np.inf):
        xb = x.copy()
        xb[2] = bad
        xo, resid, steps, status = R.polish("qp", P, q, (), xb, 8)
        assert status == 2 and steps == 0 and np.array_equal(xo, xb, equal_nan=True)
        Pb = P.copy()
        Pb[1, 3] = bad
        assert R.polish("qp", Pb, q, (), x, 8)[3] == 2


@pytest.mark.parametrize("batch", C.BATCHES + [("qp", 8, "figure")], ids=lambda b: "%s-%d-%s" % b)
def test_the_frozen_batches_are_the_builders_batches(oracle, batch):
    """tests/golden/polish holds what problem() / figure_workload() build, up to the host's last bits: P and q to 1e-9 of
    their size; the start x, an ADMM iterate stopped at eps 1e-3 (or after 20 iterations), wherever this host's forward stops
    -- only its shape is compared."""
    kind, N, structure = batch
    d0, x0 = C.frozen(kind, N, structure)
    d1, x1 = C.figure_workload() if structure == "figure" else C.problem(kind, N, C.B_CPU, structure)
    assert sorted(d0) == sorted(d1) and x0.shape == x1.shape == (C.B_CPU, N, 1)
    for k in d0:
        assert d0[k].shape == d1[k].shape and np.allclose(d0[k], d1[k], rtol=1e-9, atol=1e-9 * np.abs(d1[k]).max()), k
