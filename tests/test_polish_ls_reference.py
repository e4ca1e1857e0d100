"""CPU checks of the damped polish's numpy restatement (tests/polish_ls_reference.py) alone: with no halving allowed it is
tests/polish_reference.py's polish bit for bit; it never leaves a point worse; and from the cold start x = PI(0) it reaches
machine-precision KKT on the frozen batches of tests/golden/polish_ls exactly as often as recorded (COUNTS) -- the restatement is
elementwise IEEE arithmetic, the same on every host."""
import numpy as np
import pytest

import polish_ls_cases as C
import polish_ls_reference as L
import polish_reference as R

CASES = [(k, N, s) for k in C.KINDS for N in (2, 8, 20) for s in ("diag", "dense")]


@pytest.mark.parametrize("kind,N,structure", CASES)
def test_no_halving_is_the_plain_polish_bit_for_bit(kind, N, structure):
    P, q, ex, x = C.problem(kind, N, 12, structure)
    r = np.random.default_rng(N)
    for start in (x, np.array(L.polish_ls_batch(kind, P, q, ex, x, 40, 8)[0]) + 1e-6 * r.standard_normal(x.shape)):
        for steps in (0, 1, 8):
            ref = R.polish_batch(kind, P, q, ex, start, steps)
            got = L.polish_ls_batch(kind, P, q, ex, start, steps, 0)
            assert all(g.dtype == e.dtype and C.same_bits(g, e) for g, e in zip(got[:4], ref)) and not got[4].any()
    assert (ref[3] == 0).sum() >= 3          # (the second start is near a solution: steps are accepted)
    # a problem whose full steps are all accepted: the plain polish's bits at any cap, and no halvings
    damped = L.polish_ls_batch(kind, P, q, ex, start, 8, 8)
    never_rejected = (ref[2] == 8) | (ref[1][:, 1] == 0.0)
    assert not damped[4][never_rejected].any()
    same = damped[4] == 0          # (a rejected last step that no halving repairs leaves the plain polish's result too)
    assert same.any()
    for g, e in zip(damped[:4], ref):
        assert C.same_bits(g[same], e[same])


@pytest.mark.parametrize("kind,N,structure", CASES)
def test_residual_never_grows(kind, N, structure):
    P, q, ex, x = C.problem(kind, N, 12, structure)
    for h in (0, 1, 8, 60):
        for reg in (0.0, 1e-3):
            out = L.polish_ls_batch(kind, P, q, ex, x, 6, h, reg)
            assert (out[1][:, 1] <= out[1][:, 0]).all() and ((out[3] == 0) == (out[2] > 0)).all()
            assert (out[4] <= h * out[2]).all()


@pytest.mark.parametrize("name,kind,N", L.ROWS)
def test_cold_start_counts_on_the_frozen_batches(name, kind, N):
    P, q, ex, x = L.frozen(name, kind)
    assert q.shape == (L.B_COLD, N)
    got = []
    for h in (0, 8):
        out = L.polish_ls_batch(kind, P, q, ex, x, L.MAX_STEPS, h)
        assert (out[1][:, 1] <= out[1][:, 0]).all()
        got.append(int(L.converged(P, q, out).sum()))
        print("%s max_halvings=%d: %d of %d at the bar, most accepted steps %d, most halvings %d" % (
            name, h, got[-1], L.B_COLD, out[2][L.converged(P, q, out)].max(initial=0), out[4].max()))
    assert tuple(got) == L.COUNTS[name]
    if "k60" in name:       # what keeps the row meaningful: damping makes a solver of the polish
        assert got[1] >= 28 and got[1] >= got[0] + 9
