"""CPU checks of the numpy restatement of dqq_jvp_f64 (tests/jvp_reference.py), which every other JVP test stands on.  These
tests check the YARDSTICK, not the product: none of them calls dqq_jvp_f64 or Function.jvp, and they pass on a tree without the
entry point.  The product is held to the yardstick by tests/test_jvp_hostcore.py (through bwd_systems.h's helpers),
tests/test_jvp_routes.py and tests/test_gpu_jvp.py.

1. Pinning: run with the matrix UN-transposed (mode "bwd") the restatement is the backward, and must reproduce the oracle's
   backward bit for bit -- on make_problem batches (the cases of tests/test_bwd_systems_hostcore.py) and on batches of
   tests/warm_cases.py.  The JVP mode shares the matrix, the duals, the active sets, the placements and the refinement routine.
2. Finite differences: the JVP against central differences of the oracle's forward (eps = 1e-10) along a random tangent, at the
   step and with the bars of tests/test_gpu_fd.py, split as there: finite differences against an EXACT solve of the system the
   restatement assembled, then the restatement's Tikhonov iterate against that solve within the bound its step count implies.
   Problems whose active set changes inside the step are left out, at most a quarter of a batch.
3. The adjoint identity of the two truncated refinements, measured: the number the GPU test's bar is derived from -- on
   jvp_cases' batches and on the reference's ill-conditioned fixtures (jvp_cases.FIXTURE_GAP_CPU).
4. The inputs of the GPU tests do what they are there for: epsilon moves dx on jvp_cases.loose_problem's batches, and the
   ill-conditioned fixtures reach the refinement's long exits on the host core."""
import numpy as np
import pytest

import jvp_cases as C
import jvp_reference as R
import warm_cases as WC
from test_bwd_systems_hostcore import _oracle_backward

H = 1e-6   # tests/test_gpu_fd.py
FD_BAR = {"qp": (2e-4, 1e-3), "qcqp": (5e-5, 2e-3), "box": (5e-5, 1e-3), "sbox": (5e-5, 1e-3)}   # ... its bars, abs + rel
PIN = [("qp", 5), ("qp", 8), ("qcqp", 4), ("qcqp", 6), ("box", 3), ("box", 4), ("sbox", 3), ("sbox", 4)]
B = 32


def _check_pinned(oracle, kind, d, x):
    ref = _oracle_backward(oracle, kind, d, x, C.EPSILON)
    P, q, ex = R.flat(d, kind)
    g = np.asarray(d["grad_x"]).reshape(q.shape)
    for b in range(q.shape[0]):
        got = R.derivative(kind, P[b], q[b], tuple(e[b] for e in ex), x[b, :, 0], C.EPSILON, "bwd", g=g[b])
        got["steps"] = np.atleast_1d(np.array(got["steps"], dtype=np.int32))
        for k, r in ref.items():
            assert np.array_equal(got[k], r[b]), (kind, b, k)


@pytest.mark.parametrize("kind,N", PIN)
def test_untransposed_restatement_is_the_oracles_backward(oracle, kind, N):
    d, x = C.problem(kind, N, B)
    _check_pinned(oracle, kind, d, x)


@pytest.mark.parametrize("row", WC.n8_rows()[1::2], ids=WC.row_id)
def test_untransposed_restatement_on_warm_case_batches(oracle, row):
    """The dense N = 8 rows of tests/warm_cases.py, one per kind: their base batch, the oracle's own solution."""
    kind = row[1]
    base, _ = WC.problem(row)
    d = {k: np.ascontiguousarray(v.numpy()[:16]) for k, v in base.items()}
    ex = WC.extras_of(kind, {k: v[:16] for k, v in base.items()})
    if kind == "qp":
        x, _ = oracle.qp_fwd_batch(d["P"], d["q"], C.EPS_FWD, C.MAX_ITER)
    elif kind == "qcqp":
        x, _ = oracle.qcqp_fwd_batch(d["P"], d["q"], ex[0], ex[1], C.EPS_FWD, C.MAX_ITER)
    else:
        x, _ = oracle.boxqp_fwd_batch(d["P"], d["q"], ex[0], ex[1], C.EPS_FWD, C.MAX_ITER, v=d.get("v"))
    _check_pinned(oracle, kind, d, x)


def _forward(oracle, kind, P, q, ex):
    if kind == "qp":
        return oracle.qp_fwd_batch(P, q, C.EPS_FWD, C.MAX_ITER)[0]
    if kind == "qcqp":
        return oracle.qcqp_fwd_batch(P, q, ex[0], ex[1], C.EPS_FWD, C.MAX_ITER)[0]
    return oracle.boxqp_fwd_batch(P, q, ex[0], ex[1], C.EPS_FWD, C.MAX_ITER, v=ex[2] if kind == "sbox" else None)[0]


@pytest.mark.parametrize("kind", ["qp", "qcqp", "box", "sbox"])
def test_jvp_matches_central_differences_of_the_oracles_forward(oracle, kind):
    N = 8
    d, x = C.problem(kind, N, B)
    P, q, ex = R.flat(d, kind)
    tan = R.random_tangents(kind, B, N, 7 + R.KIND[kind])
    tan = (0.5 * (tan[0] + tan[0].transpose(0, 2, 1)),) + tan[1:]   # (the solver reads a symmetric P: move it symmetrically)
    shaped = lambda a, like: a.reshape(like.shape)   # noqa: E731
    names = C.EXTRAS[kind]
    xs = {}
    for sign in (1.0, -1.0):
        exs = [np.asarray(d[n]) + (sign * H * shaped(tan[2 + i], d[n]) if i < 2 else 0.0) for i, n in enumerate(names)]
        xs[sign] = _forward(oracle, kind, P + sign * H * tan[0], np.asarray(d["q"]) + sign * H * tan[1][:, :, None], exs)
    fd = ((xs[1.0] - xs[-1.0]) / (2 * H))[:, :, 0]
    kept, worst = 0, 0.0
    for b in range(B):
        exb = tuple(e[b] for e in ex)
        o = R.derivative(kind, P[b], q[b], exb, x[b, :, 0], C.EPSILON, "jvp", tangents=tuple(t[b] for t in tan))
        same = True
        for sign in (1.0, -1.0):
            exs = tuple(e + (sign * H * tan[2 + i][b] if i < 2 else 0.0) for i, e in enumerate(exb))
            o2 = R.derivative(kind, P[b] + sign * H * tan[0][b], q[b] + sign * H * tan[1][b], exs, xs[sign][b, :, 0], C.EPSILON,
                              "jvp", tangents=(None, None))
            same = same and np.array_equal(o2["active"], o["active"])
        if not same:
            continue
        kept += 1
        live = np.abs(o["A"]).sum(axis=0) + np.abs(o["A"]).sum(axis=1) > 0   # (QP: an active coordinate's block is x_i = 0)
        Ar = o["A"][np.ix_(live, live)]
        w = np.zeros(len(o["s"]))
        w[live] = np.linalg.solve(Ar, o["s"][live])
        exact = o["place"](w)
        a, r = FD_BAR[kind]
        e1 = np.abs(fd[b] - exact) - (a + r * np.abs(exact))
        assert e1.max() <= 0, ("FD vs exact solve", kind, b, float(np.abs(fd[b] - exact).max()))
        smin = np.linalg.svd(Ar, compute_uv=False).min()
        damp = (R.MU_IR / (smin ** 2 + R.MU_IR)) ** int(np.atleast_1d(o["steps"])[-1])
        scale = max(1.0, float(np.abs(exact).max()))
        bound = 2.0 * damp * scale * np.sqrt(len(o["s"])) + 1e-6 * scale
        e2 = float(np.abs(o["dx"] - exact).max())
        assert e2 <= bound, ("restatement vs exact beyond the Tikhonov bound", kind, b, e2, bound, smin)
        worst = max(worst, float(np.abs(fd[b] - o["dx"]).max()))
    print("%s: kept %d of %d, worst |fd - jvp| %.3g" % (kind, kept, B, worst))
    assert kept >= 0.75 * B, kept


@pytest.mark.parametrize("kind", ["qp", "qcqp", "box", "sbox"])
def test_adjoint_gap_of_the_two_refinements_is_what_was_recorded(kind):
    """The recorded figures (jvp_cases.ADJOINT_GAP_CPU) are this measurement to the two digits recorded: the GPU
    test's bar is ten times the record."""
    gaps = [C.adjoint_gap_cpu(kind, N, B_, s) for N, B_, s in C.ADJOINT_BATCHES]
    print("%s: adjoint gaps %s" % (kind, ["%.3g" % g for g in gaps]))
    assert float("%.2g" % max(gaps)) == C.ADJOINT_GAP_CPU[kind]


@pytest.mark.parametrize("kind,N,B,structure", C.EPSILON_ROWS)
def test_epsilon_selects_different_active_sets_on_the_loose_batches(oracle, kind, N, B, structure):
    """What tests/test_gpu_jvp.py's epsilon test stands on, shown on the restatement: between epsilon = 1e-10 and 1e-3 dx changes
    on at least MIN_MOVED of the batch (measured: 0.95 to 1.0 of every row), and 1e-6 is the host core's too."""
    moved = C.moved_by_epsilon(kind, N, B, structure)
    print("%s N=%d %s: dx moved by epsilon on %.3f of the batch" % (kind, N, structure, moved))
    assert moved >= C.MIN_MOVED
    d, x = C.loose_problem(kind, N, B, structure)
    P, q, ex = R.flat(d, kind)
    tan = C.epsilon_tangents(kind, N, B, structure)
    for e in C.EPSILONS:
        host, ref = C.host_jvp(kind, d, x, tan, epsilon=e), R.jvp_batch(kind, P, q, ex, x[:, :, 0], tan, e)
        assert np.array_equal(host[0], ref[0]) and np.array_equal(host[1].reshape(ref[1].shape), ref[1]), e


def test_ill_conditioned_fixtures_reach_the_refinements_long_exits():
    """tests/test_gpu_jvp_conditioning.py cannot pass on easy inputs: over the fixtures the host core's refinement leaves after 1
    body, after 3 (no progress twice), in between, and at the cap of 10 steps."""
    seen = set()
    for name in C.fixture_names():
        kind, d, x, tan, _, _ = C.fixture(name)
        seen |= set(C.host_jvp(kind, d, x, tan)[1].ravel().tolist())
    print("refinement step counts over the fixtures:", sorted(seen))
    assert {1, 3, R.IR_MAX} <= seen and seen - {1, 3, R.IR_MAX}


def test_fixture_adjoint_gaps_are_what_was_recorded():
    """jvp_cases.FIXTURE_GAP_CPU is this measurement, the largest over a family's files, to the two digits recorded."""
    gaps = {}
    for name in C.fixture_names():
        fam = C.fixture_family(name)
        gaps[fam] = max(gaps.get(fam, 0.0), C.fixture_gap_cpu(name))
    print({k: "%.3g" % v for k, v in gaps.items()})
    assert {k: float("%.2g" % v) for k, v in gaps.items()} == C.FIXTURE_GAP_CPU
