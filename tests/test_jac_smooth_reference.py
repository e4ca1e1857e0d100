"""The numpy restatement of the smoothed Newton Jacobians (tests/jac_smooth_reference.py) against its own definition: at kappa = 0
it is jac_reference's bits; at kappa > 0 every column is the restated smoothed JVP on the unit tangent bit for bit, for every kind,
dense and compact, with and without a proximal weight; every subset of outputs has the same bits.  Then what the Jacobians are for,
on the batches frozen under tests/golden/smooth at kappa = 1e-2: columns against central differences of the smoothed polish's own
solution and ops.newton_jacobian_vjp against the restated smoothed backward, both inside 10 x the recorded figure
(tests/jac_smooth_cases.py); the column of an inactive bound or radius is finite and not zero where the hard Jacobian's is exactly
zero; dx_i/dl_min_i > 0 at a free coordinate.  No GPU."""
import numpy as np
import pytest

import jac_reference as JR
import jac_smooth_cases as C
import jac_smooth_reference as JS
import newton_reference as NR
import polish_reference as R
import smooth_cases as SC
import smooth_reference as S

same = C.same_bits
N, B = 8, 6


@pytest.mark.parametrize("structure", ["dense", "diag"])
@pytest.mark.parametrize("kind", C.KINDS)
def test_kappa_zero_is_the_hard_restatement(kind, structure):
    P, q, ex, x = C.problem(kind, N, B, structure)
    got, ref = JS.jacobians_batch(kind, P, q, ex, x, kappa=0.0), JR.jacobians_batch(kind, P, q, ex, x)
    assert np.array_equal(got[3], ref[3])
    for g, r in zip(got[:3], ref[:3]):
        assert (g is None and r is None) or same(g, r)


@pytest.mark.parametrize("reg", C.REGS)
@pytest.mark.parametrize("kappa", C.KAPPAS[1:])
@pytest.mark.parametrize("structure", ["dense", "diag"])
@pytest.mark.parametrize("kind", C.KINDS)
def test_every_column_is_the_smoothed_jvp_of_the_unit_tangent(kind, structure, kappa, reg):
    P, q, ex, x = C.problem(kind, N, B, structure)
    J = JS.jacobians_batch(kind, P, q, ex, x, (True, True, True), reg, kappa)
    assert not J[3].any()
    for which in range(1 if kind == "qp" else 3):
        for j in range(J[which].shape[2]):
            dx, st = S.jvp_batch(kind, P, q, ex, x, *C.unit_tangents(kind, B, N, which, j), reg=reg, kappa=kappa)
            assert not st.any() and same(J[which][:, :, j], dx), (which, j)
    if structure == "diag":     # the compact form: the blocks carry everything, the rest is zero
        for which in range(1 if kind == "qp" else 3):
            assert (J[which][:, JS.off_block_mask(kind, N, which)] == 0.0).all()
            assert np.isfinite(JS.compact(kind, J[which], which)).all()


@pytest.mark.parametrize("kind", C.KINDS)
def test_every_subset_of_outputs_has_the_same_bits(kind):
    P, q, ex, x = C.problem(kind, N, B, "dense")
    full = JS.jacobians_batch(kind, P, q, ex, x, (True, True, True), C.REG, C.KAPPA)
    for need in C.subsets(kind):
        part = JS.jacobians_batch(kind, P, q, ex, x, need, C.REG, C.KAPPA)
        assert np.array_equal(part[3], full[3])
        for i in range(3):
            assert (part[i] is None) if not need[i] or (kind == "qp" and i) else same(part[i], full[i]), (need, i)


@pytest.mark.parametrize("kind", C.KINDS)
def test_columns_against_central_differences_of_the_smoothed_solution(kind):
    """Measured (tests/jac_smooth_cases.py: FINITE_DIFF = 1.63e-09 over the four kinds); every moved point is asserted converged
    inside fd_columns (smooth_cases.converged_point), and no problem is left out."""
    gap = C.fd_gap(kind)
    print("%s: finite-difference gap %.3g, bar %.3g" % (kind, gap, C.MARGIN * C.FINITE_DIFF))
    assert gap <= C.MARGIN * C.FINITE_DIFF


@pytest.mark.parametrize("kind", C.KINDS)
def test_jacobian_vjp_is_the_smoothed_backward(kind):
    gap = C.adjoint_gap(kind)
    print("%s: adjoint gap %.3g, bar %.3g" % (kind, gap, C.MARGIN * C.ADJOINT_GAP))
    assert gap <= C.MARGIN * C.ADJOINT_GAP


@pytest.mark.parametrize("kind", C.KINDS[1:])
def test_inactive_bounds_and_radii_get_columns_that_are_not_zero(kind):
    """Where the hard Jacobian's column of l_min / l_max / l_n / mu is exactly zero (the bound or radius is inactive at the hard
    solution), the smoothed one at x_kappa is finite and carries information."""
    P, q, ex, _, xh, _ = SC.frozen(kind, "dense")
    hard = JR.jacobians_batch(kind, P, q, ex, xh)
    soft = C.frozen_jacobians(kind)
    assert not hard[3].any()
    seen = 0
    for which in (1, 2):
        dead = (hard[which] == 0.0).all(axis=1)             # (B, ne): a column of zeros
        if kind == "sbox":      # a bound the sign constraint has replaced is not the caller's any more: its column stays zero
            eff = np.stack([R.effective_bounds(kind, tuple(e[b] for e in ex), 8)[which - 1] for b in range(xh.shape[0])])
            assert (soft[which][:, :, :][(eff != ex[which - 1])[:, None, :].repeat(8, axis=1)] == 0.0).all()
            dead &= eff == ex[which - 1]
        col = np.abs(soft[which]).max(axis=1)
        assert np.isfinite(soft[which]).all() and (col[dead] > 0.0).all()
        seen += int(dead.sum())
    assert seen > 0


@pytest.mark.parametrize("kind", ["box", "sbox"])
def test_a_free_coordinate_follows_its_lower_bound(kind):
    """dx_i/dl_min_i > 0 where coordinate i is free at the hard solution (the hard derivative is zero there) and l_min is the
    caller's own bound."""
    P, q, ex, _, xh, _ = SC.frozen(kind, "dense")
    Ja = C.frozen_jacobians(kind)[1]
    free = np.stack([NR.box_state(kind, NR._setup(kind, P[b], q[b], tuple(e[b] for e in ex), xh[b])[1], tuple(e[b] for e in ex), 8) == 0
                     for b in range(xh.shape[0])])
    if kind == "sbox":                  # where the sign constraint has replaced l_min its column stays zero
        free &= np.stack([R.effective_bounds(kind, tuple(e[b] for e in ex), 8)[0] == ex[0][b] for b in range(xh.shape[0])])
    d = Ja[:, np.arange(8), np.arange(8)]
    assert free.any() and (d[free] > 0.0).all()
