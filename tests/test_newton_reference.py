"""CPU checks of the numpy restatement of the Newton derivatives (tests/newton_reference.py), which every other Newton test
stands on: the JVP against central differences of the oracle's forward, the backward against the JVP through the adjoint
identity (measured, and held to the record in tests/newton_cases.py), and the backward against the oracle's regularised backward
at the same polished point on strictly complementary problems."""
import numpy as np
import pytest

import jvp_cases as JC
import jvp_reference as JR
import newton_cases as C
import newton_reference as NR
import polish_cases as PC
import polish_reference as R
from test_bwd_systems_hostcore import _oracle_backward

H = 1e-6   # tests/test_gpu_fd.py
FD_BAR = {"qp": (2e-4, 1e-3), "qcqp": (5e-5, 2e-3), "box": (5e-5, 1e-3), "sbox": (5e-5, 1e-3)}   # ... its bars, abs + rel
B = 32


def _forward(oracle, kind, P, q, ex):
    if kind == "qp":
        return oracle.qp_fwd_batch(P, q, JC.EPS_FWD, JC.MAX_ITER)[0]
    if kind == "qcqp":
        return oracle.qcqp_fwd_batch(P, q, ex[0], ex[1], JC.EPS_FWD, JC.MAX_ITER)[0]
    return oracle.boxqp_fwd_batch(P, q, ex[0], ex[1], JC.EPS_FWD, JC.MAX_ITER, v=ex[2] if kind == "sbox" else None)[0]


def _pattern(kind, P, q, ex, x):
    """What D and E are decided by: the state of every coordinate / whether each contact is outside its disc."""
    z = R.evaluate(kind, P, q, ex, x)[0]
    if kind == "qcqp":
        return np.array([NR.disc_u(float(z[2 * k]), float(z[2 * k + 1]), float(ex[0][k]) * float(ex[1][k]))[0]
                         for k in range(x.shape[0] // 2)])
    return NR.box_state(kind, z, ex, x.shape[0])


@pytest.mark.parametrize("kind", C.KINDS)
def test_jvp_matches_central_differences_of_the_oracles_forward(oracle, kind):
    N = 8
    d, x = JC.problem(kind, N, B)
    P, q, ex = JR.flat(d, kind)
    xp = R.polish_batch(kind, P, q, ex, np.ascontiguousarray(x[:, :, 0]), PC.MAX_STEPS)[0]
    tan = JR.random_tangents(kind, B, N, 7 + R.KIND[kind])
    tan = (0.5 * (tan[0] + tan[0].transpose(0, 2, 1)),) + tan[1:]   # (the solver reads a symmetric P: move it symmetrically)
    names = JC.EXTRAS[kind]
    xs, moved = {}, {}
    for sign in (1.0, -1.0):
        exs = [np.asarray(d[n]) + (sign * H * tan[2 + i].reshape(d[n].shape) if i < 2 else 0.0) for i, n in enumerate(names)]
        moved[sign] = (P + sign * H * tan[0], q + sign * H * tan[1], [e.reshape(B, -1) for e in exs])
        xs[sign] = _forward(oracle, kind, moved[sign][0], np.asarray(d["q"]) + sign * H * tan[1][:, :, None], exs)[:, :, 0]
    fd = (xs[1.0] - xs[-1.0]) / (2 * H)
    dx, st = NR.jvp_batch(kind, P, q, ex, xp, *tan)
    assert not st.any()
    a, r = FD_BAR[kind]
    kinked, left, worst = [], [], 0.0
    for b in range(B):
        base = _pattern(kind, P[b], q[b], tuple(e[b] for e in ex), xp[b])
        if not all(np.array_equal(base, _pattern(kind, moved[s][0][b], moved[s][1][b], tuple(e[b] for e in moved[s][2]), xs[s][b]))
                   for s in (1.0, -1.0)):
            kinked.append(b)   # the active set changes inside the step: the central difference straddles a kink
            continue
        if np.abs(xp[b] - x[b, :, 0]).max() > 1e-6:
            left.append(b)     # the polish left the oracle's x: differences of that forward say nothing about this point
            continue
        err = np.abs(fd[b] - dx[b])
        assert (err - (a + r * np.abs(dx[b]))).max() <= 0, (kind, b, float(err.max()))
        worst = max(worst, float(err.max()))
    print("%s: %d of %d straddle a kink, %d left by the polish %s, worst |fd - jvp| %.3g" % (kind, len(kinked), B, len(left), left, worst))
    assert len(kinked) <= B // 4, kinked
    # The known cases: problems 1, 21 and 24 of the signed box batch, where the oracle's forward stops away from the KKT point
    # (its x leaves a natural residual above 1e-3, the polished point one below 1e-14).  On problem 1 it returns coordinate 0
    # on its lower bound, x_0 = l_min = -0.662, residual 0.1; the polish moves it to x_0 = -0.562, free.
    assert left == ([1, 21, 24] if kind == "sbox" else []), left
    for b in left:
        exb = tuple(e[b] for e in ex)
        r_oracle, r_polished = R.evaluate(kind, P[b], q[b], exb, x[b, :, 0])[2], R.evaluate(kind, P[b], q[b], exb, xp[b])[2]
        print("  problem %d: natural residual %.3g at the oracle's x, %.3g polished" % (b, r_oracle, r_polished))
        assert r_oracle > 1e-3 and r_polished < 1e-14
    if left:
        exb = tuple(e[1] for e in ex)
        assert x[1, 0, 0] == exb[0][0] and NR.box_state(kind, R.evaluate(kind, P[1], q[1], exb, xp[1])[0], exb, N)[0] == 0


@pytest.mark.parametrize("kind", C.KINDS)
def test_adjoint_gap_is_what_was_recorded(kind):
    """newton_cases.ADJOINT_GAP_CPU is this measurement to the two digits recorded; every batch's gap is
    rounding (far below the 1e-12 asserted here), against 0.054 / 0.060 / 2.6e-4 of the reference derivatives."""
    gaps = [C.restatement_gap(k, N, s) for k, N, s in C.BATCHES if k == kind]
    print("%s: adjoint gaps %s" % (kind, ["%.3g" % g for g in gaps]))
    assert max(gaps) < 1e-12
    assert float("%.2g" % max(gaps)) == C.ADJOINT_GAP_CPU[kind]


@pytest.mark.parametrize("kind", C.KINDS)
def test_agreement_with_the_oracles_backward_on_strictly_complementary_problems(oracle, kind):
    worst = 0.0
    for k, structure in C.AGREE_BATCHES:
        if k != kind:
            continue
        d, P, q, ex, x = C.agree_problem(kind, structure)
        ok, active, free = C.strictly_complementary(kind, P, q, ex, x)
        assert ok.mean() >= 0.9 and active >= 0.25 and free >= 0.25, (structure, float(ok.mean()), active, free)
        # the multiplier margin the batches were built with holds on the oracle's polished solutions, for every problem
        assert C.strictly_complementary(kind, P, q, ex, x, C.MARGIN_OF_SCALE)[0].all(), structure
        ref = _oracle_backward(oracle, kind, d, np.ascontiguousarray(x[:, :, None]), 1e-10)
        got = NR.backward_batch(kind, P, q, ex, x, d["grad_x"].reshape(x.shape))
        assert not got[4].any()
        a = C.agreement(kind, ref, got, np.nonzero(ok)[0])
        print("%s %s: %d of %d strictly complementary, active %.2f, agreement %.3g" % (kind, structure, ok.sum(), ok.size, active, a))
        worst = max(worst, a)
    assert worst <= 10 * C.AGREE_CPU[kind], worst
