"""dqq_newton_jac_smooth_f64 on the device (-m gpu): every route family, compiled size and kind against the host core
(tests/hostcore/jac_smooth_core_check.cpp, held bit-equal to the numpy restatement on the CPU) bit for bit -- Jq, Ja, Jb and the
status --, with a NaN and an Inf problem in the middle of the batch, every subset of outputs, a batch slice with a storage offset
and reg > 0; every column at N = 8 against the device's dqq_newton_jvp_smooth_f64 on the unit tangent, in both layouts; kappa = 0
against dqq_newton_jac_reg_f64; a diagonal P given as (B,N,N) against DQQ_P_DIAG; the Python fronts; solve_*_sensitivities(kappa=)
with its Jacobians fed to ops.newton_jacobian_vjp against ops.*_newton_backward(kappa=); a captured graph replayed twice.
Inputs: tests/jac_smooth_cases.py."""
import numpy as np
import pytest
import torch

import jac_smooth_cases as C
import jac_smooth_reference as JS
import polish_reference as R
import smooth_cases as SC

pytestmark = pytest.mark.gpu

AUTO, DENSE, DIAG = C.AUTO, C.DENSE, C.DIAG
KAPPA, REG = C.KAPPA, C.REG


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()


def nout(kind):
    return 1 if kind == "qp" else 3


def _stream():
    return torch.cuda.current_stream().cuda_stream


def jac(kind, P, q, ex, x, layout, kappa, need=(True, True, True), reg=0.0, first=0, parent=False):
    """dqq_newton_jac_smooth_f64 itself (parent: dqq_newton_jac_reg_f64) on flat numpy arrays, the problems from `first` on as
    views into the full batch's memory.  -> numpy (Jq, Ja, Jb: None where not requested, status)"""
    from diffqcqp_amd import _capi, ops
    lib = _capi.lib()
    B, N = x.shape
    k, diag = R.KIND[kind], (layout & 0xff) == DIAG
    t = [a[first:] for a in [dev(C.compact(P) if diag else P), dev(q)] + [dev(e) for e in ex] + [dev(x)]]
    n = B - first
    need = tuple(need) + (True,) * (3 - len(need))
    J = [torch.full((n,) + s[1:], 7.0, dtype=torch.float64, device="cuda") if s is not None and nd else None
         for s, nd in zip(C.out_shapes(kind, n, N, diag), need)]
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ws = ops.newton_jac_workspace(torch.device("cuda"), k, N, n) if not diag else None
    exp = [a.data_ptr() for a in t[2:-1]] + [None] * (3 - len(ex))
    head = (k, t[0].data_ptr(), t[1].data_ptr(), *exp, t[-1].data_ptr(), *[None if j is None else j.data_ptr() for j in J], n, N, layout, reg)
    tail = (status.data_ptr(), None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel() * 4, _stream())
    rc = lib.dqq_newton_jac_reg_f64(*head, *tail) if parent else lib.dqq_newton_jac_smooth_f64(*head, kappa, *tail)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return tuple(None if j is None else j.cpu().numpy() for j in J) + (status.cpu().numpy(),)


def same_all(got, ref, what):
    for i, (g, r) in enumerate(zip(got, ref)):
        assert (g is None) == (r is None), (what, i)
        if r is not None:
            assert g.dtype == r.dtype and C.same_bits(g, r), "%s output %d: %s vs %s" % (what, i, g.ravel()[:4], r.ravel()[:4])


def check_row(kind, N, B, layout, structure):
    """All three outputs and the status against the host core, with a NaN and an Inf problem in the middle of the batch."""
    P, q, ex, x = C.problem(kind, N, B, structure)
    m = B // 2
    P, q, ex, x = C.with_bad_rows(kind, P, q, ex, x, m, m + 1)
    diag = layout == DIAG
    ref = C.host_jac(kind, C.compact(P) if diag else P, q, ex, x, diag=diag, kappa=KAPPA)
    want = np.zeros(B, dtype=np.int32)
    want[[m, m + 1]] = 2
    assert np.array_equal(ref[3], want)
    got = jac(kind, P, q, ex, x, layout, KAPPA)
    same_all(got, ref, "%s N=%d B=%d" % (kind, N, B))
    for a in got[:nout(kind)]:
        flat = a.reshape(B, -1)
        assert np.isnan(flat[want != 0]).all() and np.isfinite(flat[want == 0]).all()
    return P, q, ex, x, got


@pytest.mark.parametrize("kind,N,B", C.DIAG_ROWS)
def test_diagonal_kernel_is_the_host_core(kind, N, B):
    check_row(kind, N, B, DIAG, "diag")


@pytest.mark.parametrize("kind,N,B", C.TEAM_ROWS)
def test_team_kernel_is_the_host_core(kind, N, B):
    check_row(kind, N, B, DENSE if N == 8 else AUTO, "dense")


@pytest.mark.parametrize("kind,N,B", C.ANY_ROWS)
def test_global_memory_kernel_is_the_host_core(kind, N, B):
    check_row(kind, N, B, DENSE, "dense")


@pytest.mark.parametrize("kind,N,layout,structure", [(k, N, lay, s) for k in C.KINDS for N, lay, s in ((8, DENSE, "dense"), (8, DIAG, "diag"), (66, DENSE, "dense"))])
def test_subsets_slices_and_a_weight(kind, N, layout, structure):
    """A requested output has the same bits whatever else is requested; a batch slice that starts at an odd problem (a storage
    offset into every array); reg > 0 against the host core."""
    B = 37 if N == 8 else 5
    P, q, ex, x = C.problem(kind, N, B, structure)
    diag = layout == DIAG
    full = jac(kind, P, q, ex, x, layout, KAPPA)
    assert not full[3].any()
    for need in C.subsets(kind):
        part = jac(kind, P, q, ex, x, layout, KAPPA, need)
        assert np.array_equal(part[3], full[3])
        for i in range(3):
            assert (part[i] is None) if not need[i] or (kind == "qp" and i) else C.same_bits(part[i], full[i]), (need, i)
    cut = jac(kind, P, q, ex, x, layout, KAPPA, first=3)
    same_all(cut, tuple(None if a is None else a[3:] for a in full), "slice")
    ref = C.host_jac(kind, C.compact(P) if diag else P, q, ex, x, diag=diag, reg=REG, kappa=KAPPA)
    got = jac(kind, P, q, ex, x, layout, KAPPA, reg=REG)
    same_all(got, ref, "reg")
    assert not C.same_bits(got[0], full[0])


@pytest.mark.parametrize("kind,layout,structure", [(k, lay, s) for k in C.KINDS for lay, s in ((DENSE, "dense"), (DIAG, "diag"))])
def test_every_column_is_the_device_jvp_of_its_unit_tangent(kind, layout, structure):
    from test_gpu_smooth import jvp
    N, B = 8, 37
    P, q, ex, x = C.problem(kind, N, B, structure)
    J = jac(kind, P, q, ex, x, layout, KAPPA, reg=REG)
    assert not J[3].any()
    for which in range(nout(kind)):
        for j in range(N if which == 0 else C.extra_cols(kind, N)):
            dx, st = jvp(kind, P, q, ex, x, C.unit_tangents(kind, B, N, which, j), layout, KAPPA, reg=REG)
            assert not st.any()
            if layout != DIAG:
                got = J[which][:, :, j]
            else:   # the compact blocks: the column's entries inside its block; the JVP is zero outside it
                inside = ~JS.off_block_mask(kind, N, which)[:, j]
                assert (dx[:, ~inside] == 0.0).all()
                rows = np.nonzero(inside)[0]
                got = np.zeros_like(dx)
                got[:, rows] = J[which][:, rows, j & 1] if (kind == "qcqp" and which == 0) else J[which][:, rows]
            assert C.same_bits(got, dx) if layout != DIAG else np.array_equal(got, dx), (kind, which, j)


@pytest.mark.parametrize("kind,N,layout,structure", [(k, N, lay, s) for k in C.KINDS for N, lay, s in ((8, DENSE, "dense"), (8, DIAG, "diag"), (20, AUTO, "dense"), (66, DENSE, "dense"))])
def test_kappa_zero_is_the_parents_bit_for_bit(kind, N, layout, structure):
    B = 37 if N <= 20 else 5
    P, q, ex, x = C.problem(kind, N, B, structure)
    for reg in (0.0, REG):
        same_all(jac(kind, P, q, ex, x, layout, 0.0, reg=reg), jac(kind, P, q, ex, x, layout, 0.0, reg=reg, parent=True), "kappa 0")


@pytest.mark.parametrize("kind,N", [(k, N) for k in C.KINDS for N in (8, 64)])
def test_a_diagonal_P_given_as_a_matrix_gives_the_compact_bits(kind, N):
    """An entry of M is an exact zero wherever P's is and an off-block right-hand-side entry is 0 - D 0: the elimination's zero-skip
    keeps the blocks apart, so the blocks are DQQ_P_DIAG's bits and every other entry is a zero."""
    B = 37
    P, q, ex, x = C.problem(kind, N, B, "diag")
    comp = jac(kind, P, q, ex, x, DIAG, KAPPA)
    full = jac(kind, P, q, ex, x, DENSE, KAPPA)
    assert np.array_equal(full[3], comp[3]) and not comp[3].any()
    for i in range(nout(kind)):
        assert C.same_bits(JS.compact(kind, full[i], i), comp[i]), (kind, i)
        assert (full[i][:, JS.off_block_mask(kind, N, i)] == 0.0).all()


def _fronts(kind):
    from diffqcqp_amd import diagnostics, ops
    return {"qp": (ops.qp_newton_jacobian, ops.qp_newton_backward, diagnostics.solve_qp_sensitivities),
            "qcqp": (ops.qcqp_newton_jacobian, ops.qcqp_newton_backward, diagnostics.solve_qcqp_sensitivities),
            "box": (ops.boxqp_newton_jacobian, ops.boxqp_newton_backward, diagnostics.solve_boxqp_sensitivities),
            "sbox": (ops.signedboxqp_newton_jacobian, ops.signedboxqp_newton_backward, diagnostics.solve_signedboxqp_sensitivities)}[kind]


def _col(a):
    return dev(a[:, :, None])


@pytest.mark.parametrize("kind", C.KINDS)
def test_the_python_fronts(kind):
    """ops.*_newton_jacobian(kappa=) is the entry's bits in both layouts; kappa = 0 stays the call it was; one-sided boxes and a bad
    kappa raise."""
    N, B = 8, 37
    front = _fronts(kind)[0]
    for layout, structure in ((DENSE, "dense"), (DIAG, "diag")):
        P, q, ex, x = C.problem(kind, N, B, structure)
        ins = [dev(C.compact(P) if layout == DIAG else P), _col(q)] + [_col(e) for e in ex] + [_col(x)]
        out = front(*ins, layout=layout, return_status=True, kappa=KAPPA, reg=REG)
        ref = jac(kind, P, q, ex, x, layout, KAPPA, reg=REG)
        same_all(tuple(t.cpu().numpy() for t in out[:-1]), ref[:nout(kind)], "front")
        assert np.array_equal(out[-1].cpu().numpy(), ref[3])
        hard = front(*ins, layout=layout)
        same_all(tuple(t.cpu().numpy() for t in hard), jac(kind, P, q, ex, x, layout, 0.0, parent=True)[:nout(kind)], "front at kappa 0")
    with pytest.raises(ValueError):
        front(*ins, layout=DIAG, kappa=-1.0)
    if kind in ("box", "sbox"):
        with pytest.raises(ValueError):
            front(*ins, layout=DIAG, kappa=KAPPA, infinite_bounds=True)


@pytest.mark.parametrize("kind", C.KINDS)
def test_sensitivities_on_the_central_path(kind):
    """solve_*_sensitivities(kappa=1e-2) on the frozen batches: the smoothed polish's status and residual come back and say
    converged; its Jacobians through ops.newton_jacobian_vjp are ops.*_newton_backward(kappa=)'s gradients inside the measured bar
    (tests/jac_smooth_cases.py: ADJOINT_GAP); with_active raises."""
    from diffqcqp_amd import ops
    _, bwd, solve = _fronts(kind)
    P, q, ex, _, _, tang = SC.frozen(kind, "dense")
    ins = [dev(P), _col(q)] + [_col(e) for e in ex]
    s = solve(*ins, 1e-6, 2000, layout="dense", kappa=KAPPA)
    assert type(s).__name__ == "SensitivitiesSmooth" and len(s.jacobians) == nout(kind)
    assert not s.smooth_status.any().item() and not s.jacobian_status.any().item()
    assert (s.smooth_resid[:, 1] <= SC.CONVERGED).all().item(), s.smooth_resid[:, 1].max().item()
    gx = _col(tang[4])
    got = ops.newton_jacobian_vjp(kind, s.jacobians, s.x, gx.unsqueeze(0))
    ref = bwd(*ins, s.x, gx, layout=DENSE, kappa=KAPPA)
    worst = max(C.rel_gap(g[0].cpu().numpy().reshape(r.shape), r.cpu().numpy()) for g, r in zip(got, ref))
    print("%s: vjp of the smoothed Jacobians against the smoothed backward %.3g, bar %.3g" % (kind, worst, C.MARGIN * C.ADJOINT_GAP))
    assert worst <= C.MARGIN * C.ADJOINT_GAP
    hard = solve(*ins, 1e-6, 2000, layout="dense")
    assert type(hard).__name__ == "Sensitivities"
    with pytest.raises(ValueError):
        solve(*ins, 1e-6, 2000, layout="dense", kappa=KAPPA, with_active=True)


@pytest.mark.parametrize("kind,N,layout,structure", [("box", 8, DIAG, "diag"), ("qcqp", 20, AUTO, "dense"), ("sbox", 66, DENSE, "dense")])
def test_a_captured_graph_replays_the_eager_bits(kind, N, layout, structure):
    from diffqcqp_amd import ops
    B = 37
    k = R.KIND[kind]
    data = [C.problem(kind, N, B, structure, seed=s) for s in (0, 1)]
    pack = lambda d: [dev(C.compact(d[0]) if layout == DIAG else d[0]), _col(d[1])] + [_col(e) for e in d[2]] + [_col(d[3])]   # noqa: E731
    static = pack(data[0])
    ws = ops.newton_jac_workspace(torch.device("cuda"), k, N, B) if layout != DIAG else None
    run = lambda t: ops._newton_jacobian(k, t[0], t[1], t[2:-1], t[-1], layout=layout, return_status=True, workspace=ws, kappa=KAPPA)   # noqa: E731
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run(static)                                # warm-up on the capture stream
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = run(static)
    torch.cuda.current_stream().wait_stream(stream)
    for d in (data[1], data[0]):                   # two replays, each on new data
        for t, new in zip(static, pack(d)):
            t.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(pack(d))
        for a, b in zip(out, eager):
            assert C.same_bits(a.cpu().numpy(), b.cpu().numpy())
