"""dqq_newton_jac_f64 on the device (-m gpu): every route family and kind against the host core
(tests/hostcore/newton_jac_check.cpp, held bit-equal to the numpy restatement on the CPU) bit for bit -- Jq, Ja, Jb and the
status --, with NaN and singular problems in the middle of the batch, a batch slice that starts at an odd problem, each output
requested alone, and a diagonal P through the general kernel; every column against dqq_newton_jvp_f64 of its unit tangent; the
torch helpers that apply the Jacobians against the single-vector entries; solve_*_sensitivities replayed from a captured graph;
and the global-memory kernel past its first trips through the batch.  Inputs: tests/newton_cases.py over tests/polish_cases.py."""
import numpy as np
import pytest
import torch

import jac_cases as C
import jac_reference as JR
import newton_cases as NC
import polish_cases as PC
import polish_reference as R
from test_gpu_newton import batch, col, dev, gpu_jvp, with_bad_rows

pytestmark = pytest.mark.gpu

AUTO, DENSE, DIAG = PC.AUTO, PC.DENSE, PC.DIAG
DIAG_ROWS, TEAM_ROWS, ANY_ROWS = C.DIAG_ROWS, C.TEAM_ROWS, C.ANY_ROWS


def nout(kind):
    return 1 if kind == "qp" else 3


def gpu_jac(kind, P, q, ex, x, layout, need=(True, True, True), **kw):
    """-> (Jq, Ja, Jb as numpy or None, status)"""
    from diffqcqp_amd import ops
    out = ops._newton_jacobian(R.KIND[kind], dev(P), col(q), [col(e) for e in ex], col(x), need, layout, return_status=True, **kw)
    J = [None if t is None else t.cpu().numpy() for t in out[:-1]] + [None] * (3 - len(out[:-1]))
    return J[0], J[1], J[2], out[-1].cpu().numpy()


def same_all(got, ref, what):
    for i, (g, r) in enumerate(zip(got, ref)):
        assert (g is None) == (r is None), (what, i)
        if r is not None:
            assert g.dtype == r.dtype and C.same_bits(g, r), "%s output %d: %s vs %s" % (what, i, g.ravel()[:4], r.ravel()[:4])


def check_family(kind, N, B, layout, structure, **kw):
    P, q, ex, x = batch(kind, N, B, structure)
    Pb, qb, exb, xb, want = with_bad_rows(kind, P, q, ex, x)
    diag = layout == DIAG

    def run(Pi, qi, exi, xi, wi):
        Pa = PC.compact(Pi) if diag else Pi
        ref = C.host_jac(kind, Pa, qi, exi, xi, diag=diag)
        assert np.array_equal(ref[3], wi)
        got = gpu_jac(kind, Pa, qi, exi, xi, layout, **kw)
        same_all(got, ref, "%s N=%d B=%d" % (kind, N, B))
        return got

    clean = run(P, q, ex, x, np.zeros(B, dtype=np.int32))
    if want.any():   # bad problems in the middle: NaN in their own rows, the neighbours what they were
        got = run(Pb, qb, exb, xb, want)
        keep = want == 0
        same_all(tuple(None if a is None else a[keep] for a in got), tuple(None if a is None else a[keep] for a in clean),
                 "neighbours")
        for a in got[:3]:
            assert a is None or np.isnan(a[~keep]).all()
    Pa = PC.compact(P) if diag else P
    for i in range(nout(kind)):   # each output alone: the same bits, the same status
        one = gpu_jac(kind, Pa, q, ex, x, layout, tuple(j == i for j in range(3)), **kw)
        assert C.same_bits(one[i], clean[i]) and np.array_equal(one[3], clean[3]), (kind, i)
        assert all(one[j] is None for j in range(3) if j != i)
    if B > 8:   # a batch slice that starts at an odd problem
        s = slice(3, B)
        cut = lambda t: tuple(None if a is None else a[s] for a in t)   # noqa: E731
        same_all(gpu_jac(kind, Pa[s], q[s], cut(ex), x[s], layout, **kw), cut(clean), "slice")
    return P, q, ex, x, clean


@pytest.mark.parametrize("kind,N,B", DIAG_ROWS)
def test_diagonal_kernel_is_the_host_core(oracle, kind, N, B):
    P, q, ex, x, cj = check_family(kind, N, B, DIAG, "diag")
    # the same diagonal P as (B,N,N) through the general kernel: DQQ_P_DIAG's bits on the blocks, zeros elsewhere
    full = gpu_jac(kind, P, q, ex, x, DENSE)
    for i in range(nout(kind)):
        assert C.same_bits(JR.compact(kind, full[i], i), cj[i]), (kind, i)
        assert (full[i][:, JR.off_block_mask(kind, N, i)] == 0.0).all()
    assert np.array_equal(full[3], cj[3])


# DQQ_P_AUTO is DQQ_P_DENSE's route (tests/test_jac_routes.py): one row per kind runs it
@pytest.mark.parametrize("kind,N,B,layout", [r + (DENSE,) for r in TEAM_ROWS] + [(k, 8, 67, AUTO) for k in C.KINDS])
def test_team_kernel_is_the_host_core(oracle, kind, N, B, layout):
    check_family(kind, N, B, layout, "dense")


@pytest.mark.parametrize("kind,N,B", ANY_ROWS)
def test_global_memory_kernel_is_the_host_core(oracle, kind, N, B):
    from diffqcqp_amd import ops
    ws = ops.newton_jac_workspace(torch.device("cuda"), R.KIND[kind], N, B)
    assert ws is not None and ws.numel() * 4 == ops._capi.lib().dqq_newton_jac_scratch_bytes(R.KIND[kind], N, B)
    assert ops.newton_jac_workspace(torch.device("cuda"), R.KIND[kind], 64, B) is None
    check_family(kind, N, B, DENSE, "dense", workspace=ws)


@pytest.mark.parametrize("kind,N,layout", [(k, N, lay) for k in C.KINDS for N, lay in ((8, DENSE), (8, DIAG), (64, DENSE), (66, DENSE))])
def test_every_column_is_the_jvp_of_its_unit_tangent(oracle, kind, N, layout):
    """By value, NaNs in the same places: every column at N = 8, the first, a middle and the last at N = 64 and 66."""
    B = 32 if N == 8 else 5
    if N == 8:
        P, q, ex, x = NC.problem(kind, N, "diag" if layout == DIAG else "dense")
    else:
        P, q, ex, x = batch(kind, N, B, "dense")
    Pa = PC.compact(P) if layout == DIAG else P
    J = gpu_jac(kind, Pa, q, ex, x, layout)
    assert not J[3].any()
    for which in range(nout(kind)):
        w = N if which == 0 else C.extra_cols(kind, N)
        for j in (range(w) if N == 8 else (0, w // 2, w - 1)):
            tan = C.unit_tangents(kind, B, N, which, j)
            dx, st = gpu_jvp(kind, Pa, q, ex, x, tan, layout)
            assert not st.any()
            if layout != DIAG:
                got = J[which][:, :, j]
            else:   # the compact blocks: the column's entries inside its block; the JVP is zero outside it
                inside = ~JR.off_block_mask(kind, N, which)[:, j]
                assert (dx[:, ~inside] == 0.0).all()
                rows = np.nonzero(inside)[0]
                got = np.zeros_like(dx)
                got[:, rows] = J[which][:, rows, j & 1] if (kind == "qcqp" and which == 0) else J[which][:, rows]
            assert np.array_equal(got, dx, equal_nan=True), (kind, which, j)


def _fronts(kind):
    from diffqcqp_amd import ops
    return {"qp": (ops.qp_newton_jacobian, ops.qp_newton_backward, ops.qp_newton_jvp),
            "qcqp": (ops.qcqp_newton_jacobian, ops.qcqp_newton_backward, ops.qcqp_newton_jvp),
            "box": (ops.boxqp_newton_jacobian, ops.boxqp_newton_backward, ops.boxqp_newton_jvp),
            "sbox": (ops.signedboxqp_newton_jacobian, ops.signedboxqp_newton_backward, ops.signedboxqp_newton_jvp)}[kind]


@pytest.mark.parametrize("kind,structure,layout", [(k, s, lay) for k in C.KINDS for s, lay in (("dense", DENSE), ("diag", DIAG))])
def test_helpers_agree_with_the_single_vector_entries(oracle, kind, structure, layout):
    """ops.newton_jacobian_vjp with K = 3 cotangents against three ops.*_newton_backward calls, ops.newton_jacobian_jvp with K = 3
    tangent sets against three ops.*_newton_jvp calls: within 16 x JAC_ADJOINT_CPU of the check's scale, elementwise."""
    from diffqcqp_amd import ops
    K = 3
    d, P, q, ex, x = NC.agree_problem(kind, structure)
    B, N = x.shape
    Pa = PC.compact(P) if layout == DIAG else P
    ins = [dev(Pa), col(q)] + [col(e) for e in ex]
    xt = col(x)
    jac, bwd, jvp = _fronts(kind)
    J = jac(*ins, xt, layout=layout)
    scale = torch.from_numpy(R.scale(P, q, x)).cuda()
    bar = C.BAR * C.JAC_ADJOINT_CPU[kind]
    sets = [NC.inputs(kind, N, B, structure, seed=s) for s in range(K)]
    g = torch.stack([col(s[1]) for s in sets])
    got = ops.newton_jacobian_vjp(kind, J, xt, g)
    worst = 0.0
    for k in range(K):
        ref = bwd(*ins, xt, g[k], layout=layout)
        for a, b in zip(got, ref):
            err = ((a[k] - b).abs().reshape(B, -1).max(dim=1).values / scale).max().item()
            worst = max(worst, err)
    tans = [((PC.compact(s[0][0]) if layout == DIAG else s[0][0]),) + tuple(v[:, :, None] for v in s[0][1:]) for s in sets]
    stacked = tuple(torch.stack([dev(t[i]) for t in tans]) for i in range(len(tans[0])))
    dx = ops.newton_jacobian_jvp(kind, J, xt, stacked)
    worst_j = 0.0
    for k in range(K):
        ref = jvp(*ins, xt, *[s[k] for s in stacked], layout=layout)
        worst_j = max(worst_j, ((dx[k] - ref).abs().reshape(B, -1).max(dim=1).values / scale).max().item())
    print("%s %s: vjp helper %.3g, jvp helper %.3g of the scale (bar %.3g)" % (kind, structure, worst, worst_j, bar))
    assert worst <= bar and worst_j <= bar


@pytest.mark.parametrize("kind", C.KINDS)
def test_sensitivities_replay_from_a_captured_graph(oracle, kind):
    from diffqcqp_amd import diagnostics
    N, B = 8, 67
    solve = {"qp": diagnostics.solve_qp_sensitivities, "qcqp": diagnostics.solve_qcqp_sensitivities,
             "box": diagnostics.solve_boxqp_sensitivities, "sbox": diagnostics.solve_signedboxqp_sensitivities}[kind]
    d0, _ = PC.problem(kind, N, B, "dense")
    d1, _ = PC.problem(kind, N, B, "diag")   # new data: another batch of the same shapes (a diagonal P as (B,N,N))
    names = ["P", "q"] + list(PC.EXTRAS[kind])
    static = [dev(d0[n]) for n in names]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        solve(*static, 1e-4, 1000, layout="dense")            # warm-up on the capture stream
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = solve(*static, 1e-4, 1000, layout="dense")
    torch.cuda.current_stream().wait_stream(stream)
    for data in (d1, d0):
        for t, n in zip(static, names):
            t.copy_(dev(data[n]))
        graph.replay()
        torch.cuda.synchronize()
        eager = solve(*[dev(data[n]) for n in names], 1e-4, 1000, layout="dense")
        assert torch.equal(out.x, eager.x) and torch.equal(out.polish_status, eager.polish_status)
        assert torch.equal(out.jacobian_status, eager.jacobian_status) and not eager.jacobian_status.any().item()
        assert len(out.jacobians) == nout(kind)
        for a, b in zip(out.jacobians, eager.jacobians):
            assert C.same_bits(a.cpu().numpy(), b.cpu().numpy())


def test_global_memory_kernel_past_its_first_trips(oracle):
    """B = 1030 at N = 66: two trips of any_grid's 512 workgroups and a ragged third; every problem equals its own B = 1 call."""
    from diffqcqp_amd import ops
    kind, N, B, base = "box", 66, 1030, 10
    P0, q0, ex0, x0 = batch(kind, N, base, "dense")
    idx = np.arange(B) % base
    f = (1.0 + 1e-3 * np.arange(B))[:, None]   # every problem its own: P scaled (the Jacobians are taken at the x given)
    P, q, x = dev(P0[idx] * f[:, :, None]), col(q0[idx]), col(x0[idx])
    ex = [col(e[idx]) for e in ex0]
    k = R.KIND[kind]
    ws = ops.newton_jac_workspace(torch.device("cuda"), k, N, B)
    J = ops._newton_jacobian(k, P, q, ex, x, layout=DENSE, return_status=True, workspace=ws)
    single = [torch.full_like(t, 7.0) for t in J[:3]]
    st = torch.full_like(J[3], -1)
    ws1 = ops.newton_jac_workspace(torch.device("cuda"), k, N, 1)
    for b in range(B):
        s = slice(b, b + 1)
        r = ops._newton_jacobian(k, P[s], q[s], [e[s] for e in ex], x[s], layout=DENSE, out=[t[s] for t in single],
                                 return_status=True, workspace=ws1)
        st[s] = r[3]
    assert torch.equal(st, J[3]) and not st.any().item()
    for a, b in zip(J[:3], single):
        assert C.same_bits(a.cpu().numpy(), b.cpu().numpy())
    assert not torch.equal(J[0][0], J[0][base])   # (the tiled problems do differ)
