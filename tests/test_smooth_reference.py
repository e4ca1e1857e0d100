"""CPU checks of the numpy restatement of the smoothed Newton family (tests/smooth_reference.py; csrc/smooth_core.h is the same
definition): kappa = 0 is the parents' restatements bit for bit; the box identity D + E_lo + E_hi = 1; the QP's central-path
identity x_i g_i = kappa^2; the adjoint gap between the two modes; the JVP against central differences of the smoothed polish's
own solution (no problem set aside); what the feature is for -- inactive bounds and radii get gradients --; and |x_kappa - x|
shrinking with kappa.  The three tolerances are 10 x the records of tests/smooth_cases.py."""
import numpy as np
import pytest

import newton_reference as NR
import polish_ls_reference as L
import smooth_cases as SC
import smooth_reference as S


@pytest.mark.parametrize("kind", SC.KINDS)
@pytest.mark.parametrize("N", (2, 8, 20))
@pytest.mark.parametrize("structure", ("diag", "dense"))
def test_kappa_zero_is_the_parents_bit_for_bit(kind, N, structure):
    B = 5
    P, q, ex, x = SC.problem(kind, N, B, structure)
    dP, dq, da, db, gx = SC.tangents(kind, N, B, structure)
    for h in (0, 8):
        ref = L.polish_ls_batch(kind, P, q, ex, x, 10, h, 1e-3)
        got = S.polish_batch(kind, P, q, ex, x, 10, h, 1e-3, 0.0)
        assert all(SC.same_bits(g, r) for g, r in zip(got, ref))
    xs = got[0]
    for g, r in zip(S.backward_batch(kind, P, q, ex, xs, gx), NR.backward_batch(kind, P, q, ex, xs, gx)):
        assert (g is None and r is None) or SC.same_bits(g, r)
    for g, r in zip(S.jvp_batch(kind, P, q, ex, xs, dP, dq, da, db), NR.jvp_batch(kind, P, q, ex, xs, dP, dq, da, db)):
        assert SC.same_bits(g, r)
    # and the smoothed formulas are another function: at a kappa that is not zero the bits differ
    assert not SC.same_bits(S.polish_batch(kind, P, q, ex, x, 10, 8, 1e-3, 1e-2)[0], got[0])


@pytest.mark.parametrize("kappa", (1e-4, 1e-2, 1.0))
def test_box_identity_to_one_rounding(kappa):
    r = np.random.default_rng(5)
    z = np.concatenate([r.uniform(-2.0, 2.0, 4000), [-1.0, 1.0, 0.0]])
    n = z.size
    ex = (np.full(n, -1.0) + 0.3 * r.random(n), np.full(n, 1.0) - 0.3 * r.random(n))
    _, D, elo, ehi = S.box("box", z, ex, n, kappa)
    # D + E_hi is p'(z - lo) to one rounding (<= 2^-53, everything lies in [0, 1]); adding E_lo = 1 - p'(z - lo) rounds once more
    assert np.abs((D + ehi) + elo - 1.0).max() <= 2.0 ** -52
    assert (D > 0).all() and (D < 1).all() and (elo >= 0).all() and (ehi >= 0).all()
    pi = S.box("box", z, ex, n, kappa)[0]
    assert (pi > ex[0]).all() and (pi < ex[1]).all()


@pytest.mark.parametrize("kappa", SC.KAPPAS)
def test_qp_solution_is_on_the_central_path(kappa):
    worst = 0.0
    for structure in ("dense", "diag"):
        P, q, _, _, xh, _ = SC.frozen("qp", structure)
        worst = max(worst, SC.central_path_gap(P, q, xh, kappa))
    print("kappa %g: max |x g - kappa^2| / kappa^2 = %.3g (record %.3g)" % (kappa, worst, SC.CENTRAL_PATH[kappa]))
    assert worst <= SC.MARGIN * SC.CENTRAL_PATH[kappa]


@pytest.mark.parametrize("kappa", SC.KAPPAS)
@pytest.mark.parametrize("kind", SC.KINDS)
def test_backward_is_the_adjoint_of_the_jvp(kind, kappa):
    P, q, ex, x, xh, tang = SC.frozen(kind)
    gap = SC.adjoint_gap(kind, P, q, ex, SC.converged_point(kind, P, q, ex, xh, kappa), tang, kappa)
    print("%s kappa %g: adjoint gap %.3g (record %.3g)" % (kind, kappa, gap, SC.ADJOINT_GAP[kappa]))
    assert gap <= SC.MARGIN * SC.ADJOINT_GAP[kappa]
    assert SC.adjoint_gap(kind, P, q, ex, np.array(x), tang, kappa, reg=1e-3) <= SC.MARGIN * SC.ADJOINT_GAP[kappa]     # any x, with reg


@pytest.mark.parametrize("kappa", SC.KAPPAS)
@pytest.mark.parametrize("kind", SC.KINDS)
def test_jvp_agrees_with_central_differences_of_the_smoothed_solution(kind, kappa):
    """Every problem of the batch takes part and every point differenced is a converged one (fd_gap asserts it): the share left
    out is 0."""
    P, q, ex, _, xh, tang = SC.frozen(kind)
    gap = SC.fd_gap(kind, P, q, ex, xh, tang, kappa)
    print("%s kappa %g: JVP vs central differences %.3g (record %.3g)" % (kind, kappa, gap, SC.FINITE_DIFF[kappa]))
    assert gap <= SC.MARGIN * SC.FINITE_DIFF[kappa]


def test_frozen_batches_are_what_the_generator_describes():
    for kind, structure in SC.ROWS:
        P, q, ex, x, xh, tang = SC.frozen(kind, structure)
        assert P.shape == (SC.B, SC.N, SC.N) and x.shape == xh.shape == (SC.B, SC.N)
        hard = L.polish_ls_batch(kind, P, q, ex, xh, 1, 0)
        assert (hard[1][:, 0] <= SC.CONVERGED).all()                       # xh is the hard solution


@pytest.mark.parametrize("kind", ("box", "sbox", "qcqp"))
def test_inactive_constraints_get_gradients(kind):
    """Hard: grad_l_min, grad_l_max, grad_l_n (and grad_mu) of a constraint that is not active are exactly +0.0.  kappa = 1e-2:
    finite and not zero.  Box: dx_i / dl_min_i > 0 for a free coordinate."""
    kappa = 1e-2
    P, q, ex, _, xh, tang = SC.frozen(kind)         # every problem of the frozen batch: xh and x_kappa are solutions
    gx = tang[4]
    xs = SC.converged_point(kind, P, q, ex, xh, kappa)
    gh = NR.backward_batch(kind, P, q, ex, xh, gx)
    gs = S.backward_batch(kind, P, q, ex, xs, gx, 0.0, kappa)
    seen = 0
    for a, b in ((gh[2], gs[2]), (gh[3], gs[3])):
        idle = a == 0.0
        if kind == "sbox":          # a bound the sign constraint has replaced stays without a gradient under smoothing too
            idle &= b != 0.0
        seen += int(idle.sum())
        assert not np.signbit(a[idle]).any() and np.isfinite(b).all() and (b[idle] != 0.0).all()
    assert seen > 0
    if kind == "box":
        free = (gh[2] == 0.0) & (gh[3] == 0.0)
        for i in range(SC.N):
            e = np.zeros((SC.B, SC.N))
            e[:, i] = 1.0
            dx, st = S.jvp_batch(kind, P, q, ex, xs, None, None, e, None, 0.0, kappa)
            assert not st.any() and (dx[:, i][free[:, i]] > 0.0).all()
        assert free.any()
        # ... and a coordinate on its bound gets a grad_q that is not zero
        assert (gh[1] == 0.0).any() and (gs[1] != 0.0).all()


@pytest.mark.parametrize("kind", SC.KINDS)
def test_the_smoothed_point_approaches_the_solution(kind):
    P, q, ex, _, xh, _ = SC.frozen(kind)
    d = np.array([np.abs(SC.converged_point(kind, P, q, ex, xh, kappa) - xh).max(axis=1) for kappa in (1e-1, 1e-2, 1e-3, 1e-4)])
    print("%s: max |x_kappa - x| over kappa = 1e-1 .. 1e-4: %s on all %d problems" % (kind, d.max(axis=1), SC.B))
    assert (d[1:] < d[:-1]).all()
