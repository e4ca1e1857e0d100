"""dqq_newton_active_f64 on the device (-m gpu): every route family and kind against the host core
(tests/hostcore/active_core_check.cpp, held bit-equal to the numpy restatement on the CPU) bit for bit in state, mult, margin,
where and status -- ragged, one-problem and empty batches, a batch slice that starts at an odd problem, a NaN and an Inf problem
in the middle, each output requested alone, the one-sided batches under the flag, a nearest element in the second chunk of rows;
a diagonal P through the general kernel; consistency with dqq_newton_bwd_f64 on the same x; the property the margin is for,
through the ops; and forward -> polish -> active replayed from a captured graph."""
import numpy as np
import pytest
import torch

import active_cases as C
import inf_bounds_cases as IC
import newton_cases as NC
import polish_cases as PC
import polish_reference as R

pytestmark = pytest.mark.gpu

AUTO, DENSE, DIAG = PC.AUTO, PC.DENSE, PC.DIAG
B = C.TEAM_B


DIAG_ROWS, TEAM_ROWS, ANY_ROWS = C.DIAG_ROWS, C.TEAM_ROWS, C.ANY_ROWS


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def col(a):
    return dev(a[:, :, None])


def gpu_active(kind, P, q, ex, x, layout, need=(True,) * 5, flag=False):
    """-> (state, mult, margin, where, status) as numpy, None where not needed"""
    from diffqcqp_amd import ops
    out = ops._newton_active(R.KIND[kind], dev(P), col(q), [col(e) for e in ex], col(x), layout, need, infinite_bounds=flag)
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def same_all(got, ref, what):
    assert C.same_outputs(got, ref) is None, "%s: %s differs" % (what, C.same_outputs(got, ref))
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype and g.shape == r.shape


def with_bad_rows(P, q, x):
    m = x.shape[0] // 2
    P, q, x = P.copy(), q.copy(), x.copy()
    x[m, -1] = np.nan
    P[m + 1, 1, 1] = np.inf
    want = np.zeros(x.shape[0], dtype=np.int32)
    want[[m, m + 1]] = 2
    return P, q, x, want


def check_family(kind, N, layout, structure, flag=False, problem=None, B=B):
    P, q, ex, x = problem if problem is not None else C.random_problem(kind, B + 1, N, structure)
    diag = layout == DIAG
    form = (lambda M: PC.compact(M)) if diag else (lambda M: M)

    def run(Pi, qi, exi, xi, what):
        ref = C.host_active(kind, form(Pi), qi, exi, xi, diag=diag, flag=flag)
        got = gpu_active(kind, form(Pi), qi, exi, xi, layout, flag=flag)
        same_all(got, ref, "%s N=%d %s" % (kind, N, what))
        return got

    s = slice(1, None)   # B problems that start at an odd problem of the allocation
    cut = lambda t: tuple(a[s] for a in t)   # noqa: E731
    clean = run(P[s], q[s], cut(ex), x[s], "B=%d" % B)
    assert not clean[4].any()
    whole = run(P, q, ex, x, "B=%d" % (B + 1))
    same_all(cut(whole), clean, "slice")
    run(P[:1], q[:1], tuple(e[:1] for e in ex), x[:1], "B=1")
    Pb, qb, xb, want = with_bad_rows(P, q, x)      # a NaN and an Inf problem in the middle: their own rows, nobody else's
    got = run(Pb, qb, ex, xb, "bad rows")
    keep = want == 0
    assert np.array_equal(got[4], want) and (got[0][~keep] == -1).all() and (got[3][~keep] == -1).all()
    assert np.isnan(got[1][~keep]).all() and np.isnan(got[2][~keep]).all()
    same_all(tuple(a[keep] for a in got), tuple(a[keep] for a in whole), "neighbours")
    for i in range(5):   # each output alone: the same bits
        one = gpu_active(kind, form(P), q, ex, x, layout, tuple(j == i for j in range(5)), flag=flag)
        assert all(one[j] is None for j in range(5) if j != i)
        assert (np.array_equal(one[i], whole[i]) if one[i].dtype.kind == "i" else PC.same_bits(one[i], whole[i])), (kind, i)
    return P, q, ex, x, whole


@pytest.mark.parametrize("kind,N", DIAG_ROWS)
def test_diagonal_kernel_is_the_host_core(kind, N):
    P, q, ex, x, cd = check_family(kind, N, DIAG, "diag", B=C.diag_b(N))
    assert N == 2 or set(C.STATES[kind]) <= set(np.unique(cd[0]))
    # item 2: the same diagonal P as (B,N,N) through the general kernel: DQQ_P_DIAG's bits
    same_all(gpu_active(kind, P, q, ex, x, DENSE), cd, "a diagonal P given dense")


# DQQ_P_AUTO is DQQ_P_DENSE's route (tests/test_active_routes.py): one row per kind runs it
@pytest.mark.parametrize("kind,N,layout", [r + (DENSE,) for r in TEAM_ROWS] + [(k, 8, AUTO) for k in C.KINDS])
def test_team_kernel_is_the_host_core(kind, N, layout):
    check_family(kind, N, layout, "dense")


@pytest.mark.parametrize("kind,N", ANY_ROWS)
def test_workgroup_kernel_is_the_host_core(kind, N):
    check_family(kind, N, DENSE, "dense")


@pytest.mark.parametrize("kind", C.KINDS)
def test_workgroup_kernel_finds_the_nearest_element_in_its_second_chunk(kind):
    """N = 258: two chunks of 256 rows.  The built problem's nearest element is its last -- rows 256 and 257 --, among random
    problems of the same size."""
    N = 258
    P, q, ex, x = C.random_problem(kind, 5, N, "dense")
    P1, q1, ex1, x1, where = C.two_chunk_problem(kind, N)
    P[2], q[2], x[2] = P1[0], q1[0], x1[0]
    for e, e1 in zip(ex, ex1):
        e[2] = e1[0]
    ref = C.host_active(kind, P, q, ex, x)
    got = gpu_active(kind, P, q, ex, x, DENSE)
    same_all(got, ref, "%s N=258" % kind)
    assert got[3][2] == where and where * (2 if kind == "qcqp" else 1) >= 256 and abs(got[2][2] - 0.01) < 1e-9
    assert not got[4].any()


def test_the_empty_batch_is_a_no_op():
    from diffqcqp_amd import ops
    for layout, pshape in ((DENSE, (0, 8, 8)), (DIAG, (0, 8))):
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")   # noqa: E731
        out = ops._newton_active(2, z(*pshape), z(0, 8, 1), [z(0, 8, 1), z(0, 8, 1)], z(0, 8, 1), layout)
        assert out.state.shape == (0, 8) and out.margin.shape == (0,) and out.status.dtype == torch.int32
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", IC.KINDS)
@pytest.mark.parametrize("N,layout,structure", [(8, DIAG, "diag"), (3, DENSE, "dense"), (8, DENSE, "dense"), (65, DENSE, "dense")])
def test_one_sided_batches_under_the_flag(kind, N, layout, structure):
    P, q, ex, x, _, _ = IC.problem(kind, B + 1, N, structure)
    assert np.isinf(ex[0]).any() and np.isinf(ex[1]).any()
    check_family(kind, N, layout, structure, flag=True, problem=(P, q, ex, x))
    # without the flag every problem with an infinite bound is refused
    Pa = PC.compact(P) if layout == DIAG else P
    plain = gpu_active(kind, Pa, q, ex, x, layout)
    has_inf = np.isinf(ex[0]).any(axis=1) | np.isinf(ex[1]).any(axis=1)
    assert np.array_equal(plain[4], np.where(has_inf, 2, 0)) and has_inf.any()


@pytest.mark.parametrize("kind", [k for k in C.KINDS if k != "qp"])     # (the QP has no bound gradients)
@pytest.mark.parametrize("N,layout,structure", [(8, DIAG, "diag"), (8, DENSE, "dense"), (20, DENSE, "dense"), (66, DENSE, "dense")])
def test_state_is_the_newton_backward_s_active_set(kind, N, layout, structure):
    """Item 3: on the same x, dqq_newton_bwd_f64's grad_a is exactly +0.0 wherever state != 1, grad_b wherever state != 2 (the
    QCQP: grad_l_n and grad_mu wherever state != 1)."""
    from diffqcqp_amd import ops
    P, q, ex, x = C.random_problem(kind, B, N, structure)
    Pa = PC.compact(P) if layout == DIAG else P
    g = np.random.default_rng(9).standard_normal(x.shape)
    k = R.KIND[kind]
    args = (dev(Pa), col(q), [col(e) for e in ex], col(x))
    act = ops._newton_active(k, *args, layout)
    _, _, ga, gb, st = ops._newton_backward(k, *args, col(g), (False, False, True, True), layout, return_status=True)
    ga, gb, state = ga.cpu().numpy()[:, :, 0], gb.cpu().numpy()[:, :, 0], act.state.cpu().numpy()
    ok = st.cpu().numpy() == 0
    assert ok.sum() >= B // 2 and not act.status.cpu().numpy().any()
    ga, gb, state = ga[ok], gb[ok], state[ok]
    off_a, off_b = state != 1, state != (1 if kind == "qcqp" else 2)
    assert off_a.any() and (~off_a).any() and (ga[~off_a] != 0.0).any()
    for grad, off in ((ga, off_a), (gb, off_b)):
        assert (grad[off] == 0.0).all() and not np.signbit(grad[off]).any()


@pytest.mark.parametrize("kind", C.BOX_LIKE)
@pytest.mark.parametrize("N,layout,structure", [(8, DIAG, "diag"), (8, DENSE, "dense"), (20, DENSE, "dense")])
def test_half_the_margin_keeps_the_state_and_the_solution(kind, N, layout, structure):
    """Item 4: tests/test_active_hostcore.py's property test with the device's Jacobians (ops._newton_jacobian), active sets
    (ops._newton_active) and scale (ops.solution_check), at the same bar."""
    from diffqcqp_amd import ops
    P, q, ex, x = NC.problem(kind, N, structure)
    k = R.KIND[kind]
    form = (lambda M: PC.compact(M)) if layout == DIAG else (lambda M: M)

    def active(kind_, P_, q_, ex_, x_):
        return gpu_active(kind_, form(P_), q_, ex_, x_, layout)

    def jacobian(kind_, P_, q_, ex_, x_):
        Jq = ops._newton_jacobian(k, dev(form(P_)), col(q_), [col(e) for e in ex_], col(x_), (True, False, False), layout)[0]
        Jq = Jq.cpu().numpy()
        return np.stack([np.diag(v) for v in Jq]) if layout == DIAG else Jq

    st0, st1, resid, margin = C.predicted_residual(kind, P, q, ex, x, seed=77000 + N, active=active, jacobian=jacobian)
    assert st0.shape[0] == NC.B_CPU and np.array_equal(st0, st1)
    # the residual of x + dx at q + dq and its scale, from the device's check
    st0_, _, m_, _, _ = active(kind, P, q, ex, x)
    Jq = jacobian(kind, P, q, ex, x)
    dq = np.random.default_rng(77000 + N).standard_normal(x.shape)
    dx = np.einsum("bij,bj->bi", Jq, dq)
    dz = dx - np.einsum("bij,bj->bi", P, dx) - dq
    s = 0.5 * m_ / np.abs(dz).max(axis=1)
    x1, q1 = x + dx * s[:, None], q + dq * s[:, None]
    _, res, _ = ops.solution_check(k, dev(form(P)), col(q1), [col(e) for e in ex], col(x1), layout=layout)
    res = res.cpu().numpy()
    worst = float((res[:, 0] / res[:, 3]).max())
    print("predict %s n%d layout %d: restated residual %.2e, the check's %.2e of the scale (record %.2e)"
          % (kind, N, layout, resid.max(), worst, C.PREDICT_CPU[kind]))
    assert resid.max() <= C.BAR * C.PREDICT_CPU[kind] and worst <= C.BAR * C.PREDICT_CPU[kind]


@pytest.mark.parametrize("kind", C.KINDS)
def test_forward_polish_active_replay_from_a_captured_graph(oracle, kind):
    """Item 5: the chain on one stream, captured and replayed on new data, bit-equal to eager."""
    from diffqcqp_amd import ops
    N, Bg = 8, 67
    k = R.KIND[kind]
    d0, _ = PC.problem(kind, N, Bg, "dense")
    d1, _ = PC.problem(kind, N, Bg, "diag")   # new data: another batch of the same shapes (a diagonal P as (B,N,N))
    names = ["P", "q"] + list(PC.EXTRAS[kind])

    def chain(P, q, *ex):
        x = ops._forward(k, P, q, ex, 1e-4, 1000, layout=DENSE)
        ops._polish(k, P, q, ex, x, PC.MAX_STEPS, DENSE, out=x)
        return x, ops._newton_active(k, P, q, ex, x, DENSE)

    static = [dev(d0[n]) for n in names]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        chain(*static)            # warm-up on the capture stream
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            xg, out = chain(*static)
    torch.cuda.current_stream().wait_stream(stream)
    for data in (d1, d0):
        for t, n in zip(static, names):
            t.copy_(dev(data[n]))
        graph.replay()
        torch.cuda.synchronize()
        xe, eager = chain(*[dev(data[n]) for n in names])
        assert torch.equal(xg, xe) and not eager.status.any().item()
        same_all(tuple(t.cpu().numpy() for t in out), tuple(t.cpu().numpy() for t in eager), "replay")
