"""The scaled merit of the damped polish (scaling="pow2" on ops.*_polish), counted on the CPU with the numpy
restatements: tests/equil_ref.py's power-of-two equilibration of the frozen box figure batches (tests/golden/polish_ls/
box_figure_n{8,20}.npz), the cold start carried into the scaled units, tests/polish_ls_reference.py's damped polish on the scaled
problem, the unscaled point.  The counts are asserted exactly, beside the 13 / 11 the unscaled polish reaches."""
import numpy as np
import pytest

import equil_ref as E
import polish_ls_reference as L
import polish_reference as R

# problems of 30 that reach the bar from the cold start in MAX_STEPS accepted steps, (max_halvings = 0, max_halvings = 8), judged on
# the scaled problem (whose resid and status the op returns)
POW2_COUNTS = {"box_figure_n8": (30, 30), "box_figure_n20": (30, 30)}


def scaled_polish(name, kind, h):
    """-> (P~, q~, the restatement's outputs on the scaled problem, x_out in the caller's units)"""
    P, q, ex, x = L.frozen(name, kind)
    Pt, qt, ext, x0t, e = E.equilibrate(kind, P, q, ex, x)
    out = L.polish_ls_batch(kind, Pt, qt, ext, x0t, L.MAX_STEPS, h)
    return Pt, qt, out, E.unscale(out[0], e)


@pytest.mark.parametrize("name", sorted(POW2_COUNTS))
def test_scaled_merit_counts_on_the_frozen_figure_batches(name):
    kind = "box"
    P, q, ex, x = L.frozen(name, kind)
    Pt, qt, ext, x0t, e = E.equilibrate(kind, P, q, ex, x)
    assert np.array_equal(x0t, L.cold_start(kind, ext, *x.shape))        # the scaled start is the scaled problem's own PI~(0)
    d = np.diagonal(Pt, axis1=1, axis2=2)
    assert (d >= 0.5).all() and (d <= 2.0).all()
    for i, h in enumerate((0, 8)):
        Pt, qt, out, xu = scaled_polish(name, kind, h)
        count = int(L.converged(Pt, qt, out).sum())
        print("%s max_halvings=%d: %d of %d at the bar scaled (unscaled polish: %d)" % (name, h, count, L.B_COLD, L.COUNTS[name][i]))
        assert count == POW2_COUNTS[name][i] and count >= L.COUNTS[name][i]
        # the caller's problem at the unscaled point: its own bar
        r = np.array([R.evaluate(kind, P[b], q[b], tuple(a[b] for a in ex), xu[b])[2] for b in range(L.B_COLD)])
        assert int(((out[3] == 0) & (r <= L.BAR * R.scale(P, q, xu))).sum()) == L.B_COLD
