"""dqq_polish_ls_f64 on the device (-m gpu): every route family and kind against the host core
(tests/hostcore/polish_ls_core_check.cpp, held bit-equal to the numpy restatement on the CPU) bit for bit -- x_out, the residuals,
the step counts, the status and the halvings --, from cold starts, where tile neighbours accept at different step lengths; then
the properties of the entry point: batch slices, in place, NaN / Inf isolation, max_steps = 0, max_halvings = 0 against the
parents, the frozen cold-start counts of tests/polish_ls_reference.py, the solution check's view of the result, the Python
fronts, HIP-graph capture.  Inputs: tests/polish_ls_cases.py."""
import numpy as np
import pytest
import torch

import polish_ls_cases as C
import polish_ls_reference as L
import polish_reference as R

pytestmark = pytest.mark.gpu

AUTO, DENSE, DIAG, INFB = C.PC.AUTO, C.PC.DENSE, C.PC.DIAG, 0x800
H = 8
DIAG_ROWS, TEAM_ROWS, ANY_ROWS = C.DIAG_ROWS, C.TEAM_ROWS, C.ANY_ROWS
NAMES = ("x_out", "resid", "steps", "status", "halvings")


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()


def entry(kind, P, q, ex, x, layout, max_steps=C.MAX_STEPS, h=H, reg=0.0, in_place=False, first=0):
    """dqq_polish_ls_f64 itself (max_halvings = 0 included, which ops._polish sends to the parents) on flat numpy arrays, the
    problems from `first` on as views into the full batch's memory.  -> numpy (x_out, resid, steps, status, halvings)"""
    from diffqcqp_amd import _capi, ops
    lib = _capi.lib()
    B, N = x.shape
    k = R.KIND[kind]
    full = [dev(C.compact(P) if (layout & 0xff) == DIAG else P), dev(q)] + [dev(e) for e in ex] + [dev(x)]
    t = [a[first:] for a in full]
    assert all(a.is_contiguous() for a in t)
    n = B - first
    xo = t[-1] if in_place else torch.full((n, N), 7.0, dtype=torch.float64, device="cuda")
    resid = torch.empty((n, 2), dtype=torch.float64, device="cuda")
    steps, status, halv = (torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(3))
    ws = ops.polish_workspace(torch.device("cuda"), k, N, n)
    exp = [a.data_ptr() for a in t[2:-1]] + [None] * (3 - len(ex))
    rc = lib.dqq_polish_ls_f64(k, t[0].data_ptr(), t[1].data_ptr(), *exp, t[-1].data_ptr(), xo.data_ptr(), n, N, max_steps, layout, reg, h,
                               resid.data_ptr(), steps.data_ptr(), status.data_ptr(), halv.data_ptr(),
                               None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel() * 4,
                               torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in (xo, resid, steps, status, halv))


def host(kind, P, q, ex, x, layout, max_steps=C.MAX_STEPS, h=H, reg=0.0):
    diag = (layout & 0xff) == DIAG
    return C.host_polish_ls(kind, C.compact(P) if diag else P, q, ex, x, max_steps, h, reg, diag=diag, inf_ok=bool(layout & INFB))


def assert_same(got, ref, what=""):
    for name, g, r in zip(NAMES, got, ref):
        assert g.dtype == r.dtype and C.same_bits(g, r), "%s %s: %s vs %s" % (what, name, g[:4], r[:4])


def family_checks(kind, N, Bs, layout, structure):
    """The bit equality on every B of the family, and on the middle one the properties of the entry point."""
    for B in Bs:
        P, q, ex, x = C.problem(kind, N, B, structure)
        ref = host(kind, P, q, ex, x, layout)
        got = entry(kind, P, q, ex, x, layout)
        print("%s N=%d B=%d layout %d: status 0 on %d, steps up to %d, halvings up to %d (%d distinct), worst r after %.2e" % (
            kind, N, B, layout, (ref[3] == 0).sum(), ref[2].max(), ref[4].max(), np.unique(ref[4]).size, ref[1][:, 1].max()))
        assert_same(got, ref, "%s N=%d B=%d" % (kind, N, B))
        assert (ref[3] == 0).sum() >= (B + 1) // 2 and (got[1][:, 1] <= got[1][:, 0]).all()
    if structure == "dense" or kind != "qp":    # (a separable QP's full step is all but exact: next to nothing to halve)
        assert np.unique(ref[4]).size >= 3, "neighbours in the largest batch must accept at different step lengths"
    B = Bs[1]
    P, q, ex, x = C.problem(kind, N, B, structure)
    ref = host(kind, P, q, ex, x, layout)
    assert_same(entry(kind, P, q, ex, x, layout, first=3), tuple(r[3:] for r in ref), "a slice from an odd problem")
    assert_same(entry(kind, P, q, ex, x, layout, in_place=True), ref, "in place")
    for h in (0, 1, 60):
        assert_same(entry(kind, P, q, ex, x, layout, 5, h), host(kind, P, q, ex, x, layout, 5, h), "max_halvings=%d" % h)
    zero = entry(kind, P, q, ex, x, layout, 0)
    assert C.same_bits(zero[0], x) and not zero[2].any() and not zero[4].any() and (zero[3] == 1).all()
    assert C.same_bits(zero[1][:, 0], ref[1][:, 0]) and C.same_bits(zero[1][:, 1], ref[1][:, 0])
    # a NaN problem and an Inf problem in the middle of a tile: status 2, x kept, no other row changes
    P2, x2 = np.array(P), np.array(x)
    m1, m2 = B // 2, B // 2 + 1
    x2[m1, N - 1] = np.nan
    P2[m2, 1, 1] = np.inf
    bad = entry(kind, P2, q, ex, x2, layout)
    assert_same(bad, host(kind, P2, q, ex, x2, layout), "with bad rows")
    assert bad[3][m1] == 2 and bad[3][m2] == 2 and C.same_bits(bad[0][[m1, m2]], x2[[m1, m2]]) and not bad[2][[m1, m2]].any()
    keep = np.ones(B, dtype=bool)
    keep[[m1, m2]] = False
    assert_same(tuple(g[keep] for g in bad), tuple(r[keep] for r in ref), "other rows")


@pytest.mark.parametrize("kind,N", DIAG_ROWS)
def test_diagonal_kernel_is_the_host_core(kind, N):
    family_checks(kind, N, C.diag_bs(N), DIAG, "diag")


@pytest.mark.parametrize("kind,N", TEAM_ROWS)
def test_team_kernel_is_the_host_core(kind, N):
    family_checks(kind, N, C.TEAM_BS, C.team_layout(N), "dense")


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("N", C.DIAG_MATRIX_N)
def test_a_diagonal_P_given_as_a_matrix_gives_the_compact_bits(kind, N):
    """Two separately written kernels on the same problems: an entry of M is an exact zero wherever P's is, and the elimination
    skips exact zeros.  N = 16 runs on the teams of 16."""
    P, q, ex, x = C.problem(kind, N, C.diag_bs(N)[1], "diag")
    for reg in (0.0, 1e-3):
        compact = entry(kind, P, q, ex, x, DIAG, reg=reg)
        assert_same(entry(kind, P, q, ex, x, DENSE, reg=reg), compact, "%s N=%d reg=%g" % (kind, N, reg))
    assert (compact[3] == 0).any()


@pytest.mark.parametrize("kind,N", ANY_ROWS)
def test_global_memory_kernel_is_the_host_core(kind, N):
    P, q, ex, x = C.problem(kind, N, 3, "dense")
    ref = host(kind, P, q, ex, x, DENSE)
    assert_same(entry(kind, P, q, ex, x, DENSE), ref, kind)
    assert ref[4].any() and (ref[3] == 0).all()
    assert_same(entry(kind, P, q, ex, x, DENSE, first=1), tuple(r[1:] for r in ref), "a slice from an odd problem")
    assert_same(entry(kind, P, q, ex, x, DENSE, in_place=True), ref, "in place")
    zero = entry(kind, P, q, ex, x, DENSE, 0)
    assert C.same_bits(zero[0], x) and (zero[3] == 1).all() and not zero[4].any()
    x2 = np.array(x)
    x2[1, N - 1] = np.inf
    bad = entry(kind, P, q, ex, x2, DENSE)
    assert_same(bad, host(kind, P, q, ex, x2, DENSE), "with a bad row")
    assert bad[3][1] == 2 and all(C.same_bits(g[[0, 2]], r[[0, 2]]) for g, r in zip(bad, ref))


@pytest.mark.parametrize("kind,N,B,layout,structure", [("box", 8, 37, DIAG, "diag"), ("sbox", 8, 9, DENSE, "dense"), ("box", 20, 9, AUTO, "dense"),
                                                       ("sbox", 65, 3, DENSE, "dense")])
def test_one_sided_boxes_and_the_proximal_weight(kind, N, B, layout, structure):
    P, q, ex, x = C.problem(kind, N, B, structure)
    ex1 = C.one_sided(ex)
    ref = host(kind, P, q, ex1, x, layout | INFB)
    assert_same(entry(kind, P, q, ex1, x, layout | INFB), ref, "one-sided")
    assert (ref[3] == 0).any() and ref[4].any() and (entry(kind, P, q, ex1, x, layout)[3] == 2).any()    # without the flag: not finite
    for reg in (0.0, 1e-3):
        assert_same(entry(kind, P, q, ex, x, layout, reg=reg), host(kind, P, q, ex, x, layout, reg=reg), "reg=%g" % reg)


@pytest.mark.parametrize("kind,N,B,layout,structure", [(k, 8, 37, DIAG, "diag") for k in C.KINDS] + [(k, 8, 9, DENSE, "dense") for k in C.KINDS] +
                         [("box", 20, 9, AUTO, "dense"), ("qp", 65, 3, DENSE, "dense")])
def test_no_halving_is_the_parents_bit_for_bit(kind, N, B, layout, structure):
    from diffqcqp_amd import ops
    P, q, ex, x = C.problem(kind, N, B, structure)
    k = R.KIND[kind]
    args = (k, dev(C.compact(P) if layout == DIAG else P), dev(q[:, :, None]), [dev(e[:, :, None]) for e in ex], dev(x[:, :, None]))
    accepted = False
    for start in (x, host(kind, P, q, ex, x, layout, 40, H)[0] + 1e-6 * q):       # cold, and near the solution (full steps accepted)
        a = args[:4] + (dev(start[:, :, None]),)
        for reg in (0.0, 1e-3):
            parent = ops._polish(*a, C.MAX_STEPS, layout, return_info=True, reg=reg)      # dqq_polish_f64 / dqq_polish_reg_f64
            got = entry(kind, P, q, ex, start, layout, h=0, reg=reg)
            for name, g, p in zip(NAMES, got, parent):
                assert C.same_bits(g, p.cpu().numpy().reshape(g.shape)), (name, reg)
            assert not got[4].any()
            accepted = accepted or bool((got[3] == 0).any())
    assert accepted


@pytest.mark.parametrize("name,kind,N", L.ROWS)
def test_cold_start_counts_on_the_frozen_batches(name, kind, N):
    """The test that fails without the damped polish: from x = PI(0) the frozen batches reach machine-precision KKT on the
    recorded number of problems, through the public ops."""
    from diffqcqp_amd import ops
    P, q, ex, x = L.frozen(name, kind)
    figure = "figure" in name and N == 8       # the compact diagonal where the layout has the N; else the general kernels
    t = [dev(C.compact(P) if figure else P), dev(q[:, :, None])] + [dev(e[:, :, None]) for e in ex]
    front = {"qp": lambda **kw: ops.qp_polish(*t, dev(x[:, :, None]), **kw), "qcqp": lambda **kw: ops.qcqp_polish(*t, dev(x[:, :, None]), **kw),
             "box": lambda **kw: ops.boxqp_polish(*t, dev(x[:, :, None]), **kw),
             "sbox": lambda **kw: ops.boxqp_polish(*t[:4], dev(x[:, :, None]), v=t[4], **kw)}[kind]
    for i, h in enumerate((0, 8)):
        halv = torch.full((L.B_COLD,), -1, dtype=torch.int32, device="cuda")
        out = front(max_steps=L.MAX_STEPS, layout=DIAG if figure else AUTO, return_info=True, max_halvings=h, halvings=halv)
        got = (out[0].cpu().numpy()[:, :, 0], out[1].cpu().numpy(), out[2].cpu().numpy(), out[3].cpu().numpy(), halv.cpu().numpy())
        count = int(L.converged(P, q, got).sum())
        print("%s max_halvings=%d: %d of %d at the bar (recorded %d)" % (name, h, count, L.B_COLD, L.COUNTS[name][i]))
        assert count == L.COUNTS[name][i]
        assert_same(got, C.frozen_host(name, kind, h), name)


@pytest.mark.parametrize("kind,N,B,layout,structure", [(k, 8, 37, DIAG, "diag") for k in C.KINDS] +
                         [(k, 20, 9, DENSE, "dense") for k in C.KINDS] + [("qcqp", 66, 3, DENSE, "dense")])
def test_accepted_outputs_do_not_look_worse_to_the_solution_check(kind, N, B, layout, structure):
    """resid[0] of x_out <= resid[0] of x + N 2^-51 resid[3]: the check sums its rows in another order, so the term is the
    rounding of one row sum."""
    from diffqcqp_amd import ops
    P, q, ex, x = C.problem(kind, N, B, structure)
    Pd, qd, exd, xd = dev(C.compact(P) if layout == DIAG else P), dev(q[:, :, None]), [dev(e[:, :, None]) for e in ex], dev(x[:, :, None])
    xo = ops._polish(R.KIND[kind], Pd, qd, exd, xd, C.MAX_STEPS, layout, max_halvings=H)
    _, before, _ = ops.solution_check(R.KIND[kind], Pd, qd, exd, xd, layout=layout)
    st, after, _ = ops.solution_check(R.KIND[kind], Pd, qd, exd, xo, layout=layout)
    before, after = before.cpu().numpy(), after.cpu().numpy()
    print("%s N=%d: check's natural residual before max %.2e, after max %.2e" % (kind, N, before[:, 0].max(), after[:, 0].max()))
    assert (after[:, 0] <= before[:, 0] + N * 2.0 ** -51 * before[:, 3]).all()


def test_fronts_and_defaults():
    """max_halvings on diagnostics.solve_*_polished and qcqp.set_default_polish_halvings reach ops._polish; the defaults are the
    calls they were."""
    from diffqcqp_amd import diagnostics, ops, qcqp
    P, q, ex, _ = C.problem("qcqp", 8, 37, "dense")
    t = [dev(P), dev(q[:, :, None])] + [dev(e[:, :, None]) for e in ex]
    eps, max_iter = 1e-12, 3                # a forward stopped far from the solution
    fwd = ops._forward(1, t[0], t[1], t[2:], eps, max_iter, layout=DENSE)
    halv = torch.empty(37, dtype=torch.int32, device="cuda")
    pol = ops._polish(1, t[0], t[1], t[2:], fwd, 8, DENSE, return_info=True, max_halvings=H, halvings=halv)
    plain = ops._polish(1, t[0], t[1], t[2:], fwd, 8, DENSE, return_info=True)
    assert halv.any().item() and (pol[3] == 0).sum().item() > (plain[3] == 0).sum().item()
    xs, _, pinfo = diagnostics.solve_qcqp_polished(*t, eps, max_iter, layout="dense", max_halvings=H)
    assert torch.equal(xs, pol[0]) and torch.equal(pinfo.halvings, halv) and torch.equal(pinfo.steps, pol[2])
    xs, _, pinfo = diagnostics.solve_qcqp_polished(*t, eps, max_iter, layout="dense")
    assert torch.equal(xs, plain[0]) and not pinfo.halvings.any().item()
    assert qcqp.set_default_polish(8) == 0 and qcqp.set_default_polish_halvings(H) == 0
    try:
        x = qcqp.QCQPFn2.apply(*t, None, eps, max_iter)
    finally:
        assert qcqp.set_default_polish(0) == 8 and qcqp.set_default_polish_halvings(0) == H
    assert torch.equal(x, ops._polish(1, t[0], t[1], t[2:], ops._forward(1, t[0], t[1], t[2:], eps, max_iter), 8, max_halvings=H))
    for bad in (-1, 61, 1.5):
        with pytest.raises(ValueError):
            ops._polish(1, t[0], t[1], t[2:], fwd, 8, DENSE, max_halvings=bad)


def test_forward_plus_damped_polish_in_a_captured_graph():
    from diffqcqp_amd import ops
    for kind, N, B in (("qcqp", 8, 37), ("qp", 65, 3)):
        P, q, ex, _ = C.problem(kind, N, B, "dense")
        k = R.KIND[kind]
        Pd, qd, exd = dev(P), dev(q[:, :, None]), [dev(e[:, :, None]) for e in ex]
        halv_eager = torch.empty(B, dtype=torch.int32, device="cuda")
        eager = ops._polish(k, Pd, qd, exd, ops._forward(k, Pd, qd, exd, 1e-12, 3), 8, return_info=True, max_halvings=H, halvings=halv_eager)
        ws = ops.make_workspace(torch.device("cuda"), B, k, 0, N)
        pws = ops.polish_workspace(torch.device("cuda"), k, N, B)
        x = torch.zeros((B, N, 1), dtype=torch.float64, device="cuda")
        xo = torch.zeros_like(x)
        halv = torch.zeros(B, dtype=torch.int32, device="cuda")
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())   # the eager calls and the buffers' fills above are on the current stream
        with torch.cuda.stream(stream):
            ops._forward(k, Pd, qd, exd, 1e-12, 3, out=x, workspace=ws)          # warm-up on the capture stream
            ops._polish(k, Pd, qd, exd, x, 8, out=xo, workspace=pws, max_halvings=H, halvings=halv)
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                ops._forward(k, Pd, qd, exd, 1e-12, 3, out=x, workspace=ws)
                ops._polish(k, Pd, qd, exd, x, 8, out=xo, workspace=pws, max_halvings=H, halvings=halv)
        torch.cuda.current_stream().wait_stream(stream)
        xo.zero_()
        halv.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(xo, eager[0]) and torch.equal(halv, halv_eager) and halv.any().item(), kind
