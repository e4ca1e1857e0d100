"""What the power-of-two equilibration buys, on the CPU oracle alone: the reference's figure workload
(tests/golden/qcqp_figure_n8.npz: P = diag(exp(U(-10, 10))), the fixture's own eps and max_iter) solved as it is and solved
scaled (tests/equil_ref.py), then unscaled.  Asserted: the scaled diagonal's interval and FEWER iterations at the batch's
maximum -- no ratio.  Measured here (DESIGN.md 4.18 has the same figures): QP maximum 450 -> 30, mean 80.8 -> 22.8; QCQP
maximum 92 -> 74, mean 40.0 -> 50.3 (a contact's two coordinates share one exponent, so the spread inside a contact stays)."""
import os

import numpy as np
import pytest

import equil_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def figure():
    d = np.load(os.path.join(GOLDEN, "qcqp_figure_n8.npz"))
    return d, float(d["eps"]), int(d["max_iter"])


@pytest.mark.parametrize("kind", ("qp", "qcqp"))
def test_scaling_lowers_the_largest_iteration_count(oracle, figure, kind):
    d, eps, mi = figure
    P, q = d["P"], d["q"][:, :, 0]
    extras = (d["l_n"][:, :, 0], d["mu"][:, :, 0]) if kind == "qcqp" else ()
    Pt, qt, ext, _, e = R.equilibrate(kind, P, q, extras)
    dg = np.diagonal(Pt, axis1=1, axis2=2)
    if kind == "qcqp":
        # a contact's exponent is that of its larger entry (a disc must stay a disc): that entry lies in [1/2, 2], the other at
        # or below it -- the interval cannot hold for both whatever the rule, since they take the same factor
        assert np.array_equal(e[:, 0::2], e[:, 1::2])
        assert (dg <= 2.0).all()
        dg = np.maximum(dg[:, 0::2], dg[:, 1::2])
    assert ((dg >= 0.5) & (dg <= 2.0)).all()
    if kind == "qp":
        x, it = oracle.qp_fwd_batch(P, d["q"], eps, mi, nthreads=8)
        y, its = oracle.qp_fwd_batch(Pt, qt[:, :, None], eps, mi, nthreads=8)
    else:
        x, it = oracle.qcqp_fwd_batch(P, d["q"], d["l_n"], d["mu"], eps, mi, nthreads=8)
        y, its = oracle.qcqp_fwd_batch(Pt, qt[:, :, None], ext[0][:, :, None], ext[1][:, :, None], eps, mi, nthreads=8)
    xs = R.unscale(y[:, :, 0], e)
    print("%s: iterations unscaled max %d mean %.2f, scaled max %d mean %.2f" % (kind, it.max(), it.mean(), its.max(), its.mean()))
    assert its.max() < mi and np.isfinite(xs).all()
    assert its.max() < it.max()
    # both are solutions of the caller's problem: the natural residual of the unscaled x of the scaled solve, on the caller's data
    g = np.einsum("bij,bj->bi", P, xs) + q
    if kind == "qp":
        nat = np.abs(xs - np.maximum(xs - g, 0.0)).max(axis=1)
        scale = np.maximum(np.abs(np.einsum("bij,bj->bi", np.abs(P), np.abs(xs))).max(axis=1), np.abs(q).max(axis=1))
        assert (nat <= 1e-6 * scale).all(), (nat / scale).max()
