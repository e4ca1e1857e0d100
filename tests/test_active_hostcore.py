"""dqq_newton_active_f64 on the CPU: csrc/active_core.h on one thread (tests/hostcore/active_core_check.cpp, a stand-alone
program, built plain and with the address and undefined-behaviour sanitizers) against the numpy restatement
tests/active_reference.py bit for bit in state, mult, margin, where and status; the conditions that keep that comparison from
passing vacuously; the property the margin is for, on the restatement; and the status rules."""
import numpy as np
import pytest

import active_cases as C
import active_reference as AR
import inf_bounds_cases as IC
import newton_cases as NC
import polish_cases as PC
import polish_reference as R

INF = float("inf")
B_INF = 16
INF_BATCHES = [(k, N, s) for k in IC.KINDS for N in (3, 8) for s in ("diag", "dense")]


def _both_builds(kind, P, q, ex, x, **kw):
    plain = C.host_active(kind, P, q, ex, x, **kw)
    san = C.host_active(kind, P, q, ex, x, sanitized=True, **kw)
    assert C.same_outputs(san, plain) is None
    return plain


@pytest.mark.parametrize("kind,N,structure", C.BATCHES)
def test_host_core_equals_the_restatement(kind, N, structure):
    """Items 2 and 3: every output bit for bit, from the plain and from the sanitized program; on a diagonal P also in the compact
    layout; and every batch holds every state its kind has."""
    P, q, ex, x = NC.problem(kind, N, structure)
    ref = AR.active_batch(kind, P, q, ex, x)
    host = _both_builds(kind, P, q, ex, x)
    assert C.same_outputs(host, ref) is None
    assert not host[4].any()
    assert set(np.unique(host[0])) == set(C.STATES[kind]), np.unique(host[0])
    active = host[0] != 0
    assert (host[1][active] >= 0.0).all() and (host[1][~active] == 0.0).all() and not np.signbit(host[1][~active]).any()
    assert (host[2] > 0.0).all() and np.isfinite(host[2]).all()
    if structure == "diag":
        assert C.same_outputs(_both_builds(kind, PC.compact(P), q, ex, x, diag=True), host) is None


@pytest.mark.parametrize("kind,N,structure", INF_BATCHES)
def test_one_sided_batches_under_the_flag(kind, N, structure):
    P, q, ex, x, _, _ = IC.problem(kind, B_INF, N, structure)
    assert all(np.isinf(e).any() and np.isfinite(e).any() for e in ex[:2])
    ref = AR.active_batch(kind, P, q, ex, x, flag=True)
    host = _both_builds(kind, P, q, ex, x, flag=True)
    assert C.same_outputs(host, ref) is None and not host[4].any()
    assert set(np.unique(host[0])) == set(C.STATES[kind]), np.unique(host[0])
    if structure == "diag":
        assert C.same_outputs(_both_builds(kind, IC.compact(P), q, ex, x, diag=True, flag=True), host) is None
    # an infinite side takes no part: its large finite stand-in gives the same states and multipliers, and the same margin
    # wherever the nearest bound is a finite one -- which it is, unless the coordinate has none
    plain = C.host_active(kind, P, q, IC.large_finite(ex), x)
    assert np.array_equal(plain[0], host[0]) and PC.same_bits(plain[1], host[1]) and np.array_equal(plain[4], host[4])
    finite = np.isfinite(host[2])
    assert finite.any() and PC.same_bits(plain[2][finite], host[2][finite]) and np.array_equal(plain[3][finite], host[3][finite])


@pytest.mark.parametrize("structure", ["diag", "dense"])
def test_a_disc_of_radius_zero(structure):
    """Item 3: the QCQP's state 3, on a built problem: l_n = 0 with z off the origin is outside (D = 0), with z = 0 inside."""
    P, q, ex, x = C.zero_disc_problem(structure)
    ref = AR.active_batch("qcqp", P, q, ex, x)
    host = _both_builds("qcqp", P, q, ex, x)
    assert C.same_outputs(host, ref) is None and host[4][0] == 0
    assert host[0][0, 0] == 3 and host[0][0, 1] == 0 and set(host[0][0, 2:]) <= {0, 1}
    z = R.evaluate("qcqp", P[0], q[0], tuple(e[0] for e in ex), x[0])[0]
    assert host[1][0, 0] == np.sqrt(R.fma(z[1], z[1], z[0] * z[0])) and host[1][0, 1] == 0.0
    assert host[2][0] == 0.0 and host[3][0] == 1           # the contact at the origin of a zero disc sits on its kink


@pytest.mark.parametrize("kind,structure", NC.AGREE_BATCHES)
def test_margin_on_the_agreement_batches(kind, structure):
    """Item 3: margin is the dist.min() of newton_cases.strictly_complementary, and at least AGREE_MARGIN of the width (radius)
    of the element that attains it."""
    _, P, q, ex, x = NC.agree_problem(kind, structure)
    B, n = x.shape
    state, mult, margin, where, status = C.host_active(kind, P, q, ex, x)
    assert not status.any()
    for b in range(B):
        exb = tuple(e[b] for e in ex)
        z = R.evaluate(kind, P[b], q[b], exb, x[b])[0]
        if kind == "qcqp":
            width = exb[0] * exb[1]
            dist = np.abs(np.hypot(z[0::2], z[1::2]) - width)
        else:
            lo, hi = R.effective_bounds(kind, exb, n)
            width = hi - lo if kind != "qp" else np.ones(n)
            dist = np.minimum(np.abs(z - lo), np.abs(z - hi))
        assert abs(margin[b] - dist.min()) <= 1e-12 * dist.min(), (b, margin[b], dist.min())
        assert dist[where[b]] <= dist.min() * (1 + 1e-12)
        assert margin[b] >= NC.AGREE_MARGIN * width[where[b]] * (1 - 1e-9), (b, margin[b], width[where[b]])
    ok = NC.strictly_complementary(kind, P, q, ex, x)[0]
    assert ok.all() and (margin / R.scale(P, q, x) >= NC.STRICT).all()


@pytest.mark.parametrize("kind,N,structure", [b for b in C.BATCHES if b[0] in C.BOX_LIKE])
def test_half_the_margin_keeps_the_state_and_the_solution(kind, N, structure):
    """Item 4, on the restatement: dq scaled so that max |dz| = margin / 2 leaves state as it is, elementwise and on every problem
    of the batch, and x + Jq dq solves the problem at q + dq to rounding: the residual over the check's scale within BAR x the
    record PREDICT_CPU."""
    P, q, ex, x = NC.problem(kind, N, structure)
    st0, st1, resid, margin = C.predicted_residual(kind, P, q, ex, x, seed=77000 + N)
    print("predict %s n%d %s: worst residual / scale %.2e (record %.2e), margin %.2e .. %.2e"
          % (kind, N, structure, resid.max(), C.PREDICT_CPU[kind], margin.min(), margin.max()))
    assert st0.shape[0] == NC.B_CPU and np.array_equal(st0, st1)
    assert resid.max() <= C.BAR * C.PREDICT_CPU[kind]


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("structure", ["diag", "dense"])
def test_status_rules(kind, structure):
    """Item 5: a NaN in P, q, x or a bound is status 2 with -1 / NaN in that problem's rows and no other row touched."""
    N = 8
    P, q, ex, x = NC.problem(kind, N, structure)
    clean = C.host_active(kind, P, q, ex, x)
    P, q, x, ex = P.copy(), q.copy(), x.copy(), tuple(e.copy() for e in ex)
    P[5, 2, 2] = np.nan
    q[7, 1] = np.nan
    x[9, 0] = np.nan
    bad = [5, 7, 9]
    if kind != "qp":
        ex[1][11, 0] = np.nan
        ex[0][13, 1] = INF            # an infinite bound / radius without the flag
        bad += [11, 13]
    keep = np.ones(x.shape[0], dtype=bool)
    keep[bad] = False
    for compact in ((False, True) if structure == "diag" else (False,)):
        out = C.host_active(kind, PC.compact(P) if compact else P, q, ex, x, diag=compact)
        assert (out[4][bad] == 2).all() and not out[4][keep].any()
        assert (out[0][bad] == -1).all() and (out[3][bad] == -1).all()
        assert np.isnan(out[1][bad]).all() and np.isnan(out[2][bad]).all()
        assert C.same_outputs([o[keep] for o in out], [o[keep] for o in clean]) is None
        if not compact:
            assert C.same_outputs(out, AR.active_batch(kind, P, q, ex, x)) is None


@pytest.mark.parametrize("kind", IC.KINDS)
def test_an_infinite_upper_bound_needs_the_flag(kind):
    """Item 5: l_max = +inf is status 2 without the flag and 0 with it, and that coordinate's e ignores the infinite side."""
    N = 8
    P, q, ex, x = NC.problem(kind, N, "dense")
    ex = tuple(e.copy() for e in ex)
    ex[1][4, :] = INF
    plain = C.host_active(kind, P, q, ex, x)
    flagged = C.host_active(kind, P, q, ex, x, flag=True)
    assert plain[4][4] == 2 and flagged[4][4] == 0 and not np.delete(plain[4], 4).any() and not flagged[4].any()
    assert C.same_outputs([np.delete(o, 4, axis=0) for o in flagged], [np.delete(o, 4, axis=0) for o in plain]) is None
    z = R.evaluate(kind, P[4], q[4], tuple(e[4] for e in ex), x[4])[0]
    lo, hi = R.effective_bounds(kind, tuple(e[4] for e in ex), N)
    e = np.where(np.isinf(hi), np.abs(z - lo), np.minimum(np.abs(z - lo), np.abs(z - hi)))
    assert flagged[2][4] == e.min() and flagged[3][4] == int(np.argmin(e)) and np.isinf(hi).any()
    assert C.same_outputs(flagged, AR.active_batch(kind, P, q, ex, x, flag=True)) is None


@pytest.mark.parametrize("structure", ["diag", "dense"])
def test_box_on_the_nonnegative_orthant_is_the_qp_kind(structure):
    """Item 5: the box on [0, +inf) under the flag equals the QP kind bit for bit -- but for state, which is 1 on the box's own
    lower bound where the QP reports the constant's 3."""
    P, q, _, x = NC.problem("qp", 8, structure)
    ex = (np.zeros_like(x), np.full_like(x, INF))
    for compact in ((False, True) if structure == "diag" else (False,)):
        Pa = PC.compact(P) if compact else P
        qp = C.host_active("qp", Pa, q, (), x, diag=compact)
        box = C.host_active("box", Pa, q, ex, x, diag=compact, flag=True)
        assert C.same_outputs(box[1:], qp[1:]) is None
        assert (qp[0] == 3).any() and np.array_equal(box[0], np.where(qp[0] == 3, 1, qp[0]))


def test_a_fully_unbounded_box():
    P, q, _, x = NC.problem("qp", 8, "dense")
    ex = (np.full_like(x, -INF), np.full_like(x, INF))
    out = C.host_active("box", P, q, ex, x, flag=True)
    assert not out[0].any() and not out[1].any() and (out[2] == INF).all() and not out[3].any() and not out[4].any()
    assert C.same_outputs(out, AR.active_batch("box", P, q, ex, x, flag=True)) is None


@pytest.mark.parametrize("kind", C.KINDS)
def test_a_requested_output_does_not_depend_on_the_others(kind):
    P, q, ex, x = NC.problem(kind, 8, "dense")
    whole = C.host_active(kind, P, q, ex, x)
    for i in range(4):
        one = C.host_active(kind, P, q, ex, x, mask=1 << i)
        assert C.same_outputs([one[i], one[4]], [whole[i], whole[4]]) is None
        for j in range(4):
            if j != i:
                assert (one[j] == (-7 if one[j].dtype.kind == "i" else 7.0)).all()
