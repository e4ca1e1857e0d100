"""dqq_polish_f64 on the device (-m gpu): every route family and kind against the host core (tests/hostcore/polish_core_check.cpp,
held bit-equal to the numpy restatement on the CPU) bit for bit -- x_out, the residuals, the step counts and the status --, then
the properties of the entry point: batch slices, NaN / Inf isolation, in place, max_steps = 0, a diagonal P through the general
kernel, the solution check's view of the result, set_default_polish on the autograd Functions, HIP-graph capture.  Inputs:
tests/polish_cases.py."""
import numpy as np
import pytest
import torch

import polish_cases as C
import polish_reference as R

pytestmark = pytest.mark.gpu

AUTO, DENSE, DIAG = C.AUTO, C.DENSE, C.DIAG
DIAG_ROWS, TEAM_ROWS, ANY_ROWS = C.DIAG_ROWS, C.TEAM_ROWS, C.ANY_ROWS
# the properties below at the diagonal sizes the first tables left out, the kinds rotating: (kind, N, B, layout, structure)
MORE_DIAG = [(k, N, C.ragged_b(N), DIAG, "diag") for k, N in zip(("qcqp", "box", "sbox"), C.DIAG_N_MORE)]


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()


def ops_polish(kind, P, q, ex, x, layout, max_steps=C.MAX_STEPS, **kw):
    """ops._polish on a batch given as flat numpy arrays (P (B,N,N), q, x (B,N), extras (B,.)); DIAG: P goes in as its compact
    diagonal.  -> numpy (x_out (B,N), resid, steps, status)"""
    from diffqcqp_amd import ops
    Pd = dev(C.compact(P) if layout == DIAG else P)
    out = ops._polish(R.KIND[kind], Pd, dev(q[:, :, None]), [dev(e[:, :, None]) for e in ex], dev(x[:, :, None]), max_steps, layout,
                      return_info=True, **kw)
    xo, resid, steps, status = (t.cpu().numpy() for t in out)
    return xo[:, :, 0], resid, steps, status


def assert_same(got, ref, what=""):
    for name, g, r in zip(("x_out", "resid", "steps", "status"), got, ref):
        assert g.dtype == r.dtype and C.same_bits(g, r), "%s %s: %s vs %s" % (what, name, g[:4], r[:4])


def check_against_host(kind, N, B, layout, structure):
    d, x = C.problem(kind, N, B, structure)
    P, q, ex = C.flat(d, kind)
    x = x[:, :, 0]
    ref = C.host_polish(kind, P, q, ex, x)
    got = ops_polish(kind, P, q, ex, x, layout)
    print("%s N=%d B=%d layout %d: accepted %d of %d, steps %s, worst r after %.2e" % (
        kind, N, B, layout, (ref[3] == 0).sum(), B, np.unique(ref[2]), ref[1][:, 1].max()))
    assert (ref[3] == 0).sum() >= B // 4           # (not a comparison of untouched points)
    assert_same(got, ref, "%s N=%d" % (kind, N))
    return P, q, ex, x, got


@pytest.mark.parametrize("kind,N,B", DIAG_ROWS)
def test_diagonal_kernel_is_the_host_core(oracle, kind, N, B):
    P, q, ex, x, got = check_against_host(kind, N, B, DIAG, "diag")
    # a batch slice that starts at an odd problem: every array a view into the full batch's memory
    from diffqcqp_amd import ops
    s = slice(3, B)
    full = [dev(C.compact(P)), dev(q[:, :, None])] + [dev(e[:, :, None]) for e in ex] + [dev(x[:, :, None])]
    views = [t[s] for t in full]
    assert all(v.is_contiguous() and v.data_ptr() != t.data_ptr() for v, t in zip(views, full))
    out = ops._polish(R.KIND[kind], views[0], views[1], views[2:-1], views[-1], C.MAX_STEPS, DIAG, return_info=True)
    xo, resid, steps, status = (t.cpu().numpy() for t in out)
    assert_same((xo[:, :, 0], resid, steps, status), tuple(g[s] for g in got), "slice")


@pytest.mark.parametrize("layout", C.TEAM_LAYOUTS)
@pytest.mark.parametrize("kind,N,B", TEAM_ROWS)
def test_team_kernel_is_the_host_core(oracle, kind, N, B, layout):
    check_against_host(kind, N, B, layout, "dense")


@pytest.mark.parametrize("kind,N,B", ANY_ROWS)
def test_global_memory_kernel_is_the_host_core(oracle, kind, N, B):
    from diffqcqp_amd import ops
    P, q, ex, x, got = check_against_host(kind, N, B, DENSE, "dense")
    ws = ops.polish_workspace(torch.device("cuda"), R.KIND[kind], N, B)       # the caller's scratch instead of the per-call one
    assert ws is not None and ops.polish_workspace(torch.device("cuda"), R.KIND[kind], 64, B) is None
    assert_same(ops_polish(kind, P, q, ex, x, DENSE, workspace=ws), got, "workspace=")


@pytest.mark.parametrize("kind,N,B,layout,structure", [(k, 8, 67, DIAG, "diag") for k in C.KINDS] + MORE_DIAG +
                         [(k, 8, 37, DENSE, "dense") for k in C.KINDS] + [("qp", 65, 5, DENSE, "dense")])
def test_nan_and_inf_problems_change_no_other_row(oracle, kind, N, B, layout, structure):
    d, x = C.problem(kind, N, B, structure)
    P, q, ex = C.flat(d, kind)
    x = x[:, :, 0]
    clean = ops_polish(kind, P, q, ex, x, layout)
    P2, x2 = np.array(P), np.array(x)
    m1, m2 = B // 2, B // 2 + 1
    x2[m1, N - 1] = np.nan
    P2[m2, 1, 1] = np.inf
    got = ops_polish(kind, P2, q, ex, x2, layout)
    assert_same(got, C.host_polish(kind, C.compact(P2) if layout == DIAG else P2, q, ex, x2, diag=layout == DIAG), "with bad rows")
    assert got[3][m1] == 2 and got[3][m2] == 2 and C.same_bits(got[0][[m1, m2]], x2[[m1, m2]]) and not got[2][[m1, m2]].any()
    keep = np.ones(B, dtype=bool)
    keep[[m1, m2]] = False
    assert_same(tuple(g[keep] for g in got), tuple(c[keep] for c in clean), "other rows")


@pytest.mark.parametrize("kind,N,B,layout,structure", [("qcqp", 8, 67, DIAG, "diag"), ("box", 20, 37, DENSE, "dense"),
                                                       ("qp", 65, 5, DENSE, "dense")] + MORE_DIAG)
def test_in_place_and_max_steps_zero(oracle, kind, N, B, layout, structure):
    from diffqcqp_amd import ops
    d, x = C.problem(kind, N, B, structure)
    P, q, ex = C.flat(d, kind)
    x = x[:, :, 0]
    ref = ops_polish(kind, P, q, ex, x, layout)
    xt = dev(x[:, :, None])
    args = (R.KIND[kind], dev(C.compact(P) if layout == DIAG else P), dev(q[:, :, None]), [dev(e[:, :, None]) for e in ex])
    out = ops._polish(*args, xt, C.MAX_STEPS, layout, out=xt, return_info=True)
    assert out[0] is xt
    assert_same(tuple(t.cpu().numpy().reshape(r.shape) for t, r in zip(out, ref)), ref, "in place")
    x0 = dev(x[:, :, None])
    out = ops._polish(*args, x0, 0, layout, return_info=True)
    assert C.same_bits(out[0].cpu().numpy()[:, :, 0], x) and not out[2].any().item() and (out[3] == 1).all().item()
    assert torch.equal(out[1][:, 0], out[1][:, 1]) and C.same_bits(out[1].cpu().numpy()[:, 0], ref[1][:, 0])


def diagonal_p_both_ways(kind, N, B):
    d, x = C.problem(kind, N, B, "diag")
    P, q, ex = C.flat(d, kind)
    a = ops_polish(kind, P, q, ex, x[:, :, 0], DENSE)
    b = ops_polish(kind, P, q, ex, x[:, :, 0], DIAG)
    assert (a[3] == 0).sum() > 16
    assert_same(a, b, kind)


@pytest.mark.parametrize("kind", C.KINDS)
def test_a_diagonal_p_through_the_general_kernel_gives_the_diagonal_kernels_bits(oracle, kind):
    diagonal_p_both_ways(kind, 8, 67)


@pytest.mark.parametrize("N", C.DIAG_N_MORE)
@pytest.mark.parametrize("kind", C.KINDS)
def test_a_diagonal_p_through_the_general_kernel_at_the_other_diagonal_sizes(oracle, kind, N):
    """N = 16 runs the general kernel on its teams of 16."""
    diagonal_p_both_ways(kind, N, C.ragged_b(N))


@pytest.mark.parametrize("kind,N,B,layout,structure", [(k, 8, 67, DIAG, "diag") for k in C.KINDS] +
                         [(k, 20, 37, DENSE, "dense") for k in C.KINDS] + [("qcqp", 66, 5, DENSE, "dense")])
def test_accepted_outputs_do_not_look_worse_to_the_solution_check(oracle, kind, N, B, layout, structure):
    """resid[0] of x_out <= resid[0] of x + N 2^-51 resid[3]: the check sums its rows in another order, so the term is the
    rounding of one row sum."""
    from diffqcqp_amd import ops
    d, x = C.problem(kind, N, B, structure)
    P, q, ex = C.flat(d, kind)
    Pd, qd, exd, xd = dev(C.compact(P) if layout == DIAG else P), dev(q[:, :, None]), [dev(e[:, :, None]) for e in ex], dev(x)
    xo, resid, steps, status = ops._polish(R.KIND[kind], Pd, qd, exd, xd, C.MAX_STEPS, layout, return_info=True)
    _, before, _ = ops.solution_check(R.KIND[kind], Pd, qd, exd, xd, layout=layout)
    st, after, _ = ops.solution_check(R.KIND[kind], Pd, qd, exd, xo, layout=layout)
    before, after = before.cpu().numpy(), after.cpu().numpy()
    print("%s N=%d: check's natural residual before max %.2e, after max %.2e" % (kind, N, before[:, 0].max(), after[:, 0].max()))
    assert (st == 0).all().item()
    assert (after[:, 0] <= before[:, 0] + N * 2.0 ** -51 * before[:, 3]).all()


@pytest.mark.parametrize("kind", ["qp", "qcqp"])
def test_set_default_polish_on_the_functions(oracle, kind):
    from diffqcqp_amd import ops, qcqp
    d, _ = C.problem(kind, 8, 67, "dense")
    t = {k: dev(v) for k, v in d.items()}
    ins = [t["P"], t["q"]] + [t[n] for n in C.EXTRAS[kind]]
    fn = qcqp.QPFn2 if kind == "qp" else qcqp.QCQPFn2
    eps, max_iter = 1e-4, 1000
    plain = fn.apply(*ins, None, eps, max_iter)
    leaves = [a.clone().requires_grad_(True) for a in ins]
    assert qcqp.set_default_polish(8) == 0
    try:
        x = fn.apply(*leaves, None, eps, max_iter)
        g = torch.randn(x.shape, generator=torch.Generator().manual_seed(1)).cuda()
        grads = torch.autograd.grad(x, leaves, g)
    finally:
        assert qcqp.set_default_polish(0) == 8
    fwd = ops._forward(R.KIND[kind], ins[0], ins[1], ins[2:], eps, max_iter)
    assert torch.equal(fwd, plain)                                     # steps = 0: the forward's bits as they were
    pol = ops._polish(R.KIND[kind], ins[0], ins[1], ins[2:], fwd, 8)
    assert torch.equal(x.detach(), pol) and not torch.equal(pol, fwd)
    ref = ops._backward(R.KIND[kind], ins[0], ins[1], ins[2:], pol, g, (True,) * len(ins), AUTO, False, None, 1e-10, None, None, None)
    for a, b in zip(grads, ref):
        assert torch.equal(a, b)
    assert torch.equal(fn.apply(*ins, None, eps, max_iter), plain)     # and switched off again


def test_forward_plus_polish_in_a_captured_graph(oracle):
    from diffqcqp_amd import ops
    for kind, N, B, structure in (("qcqp", 8, 67, "dense"), ("qp", 65, 5, "dense")):
        d, _ = C.problem(kind, N, B, structure)
        t = {k: dev(v) for k, v in d.items()}
        ex = [t[n] for n in C.EXTRAS[kind]]
        k = R.KIND[kind]
        eager = ops._polish(k, t["P"], t["q"], ex, ops._forward(k, t["P"], t["q"], ex, 1e-4, 1000), 8, return_info=True)
        ws = ops.make_workspace(torch.device("cuda"), B, k, 0, N)
        pws = ops.polish_workspace(torch.device("cuda"), k, N, B)
        x = torch.zeros((B, N, 1), dtype=torch.float64, device="cuda")
        xo = torch.zeros_like(x)
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())   # the eager calls and the buffers' fills above are on the current stream
        with torch.cuda.stream(stream):
            ops._forward(k, t["P"], t["q"], ex, 1e-4, 1000, out=x, workspace=ws)          # warm-up on the capture stream
            ops._polish(k, t["P"], t["q"], ex, x, 8, out=xo, workspace=pws)
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                ops._forward(k, t["P"], t["q"], ex, 1e-4, 1000, out=x, workspace=ws)
                ops._polish(k, t["P"], t["q"], ex, x, 8, out=xo, workspace=pws)
        torch.cuda.current_stream().wait_stream(stream)
        xo.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(xo, eager[0]) and (eager[3] == 0).sum().item() >= B // 4, kind


def test_every_public_front_is_ops_polish(oracle):
    """ops.qp_polish / qcqp_polish / boxqp_polish(v=), diagnostics.solve_*_polished (GPU tensors, and CPU tensors staged there
    and back) and diffqcqp.polishQP / polishQCQP / polishBoxQP against ops._polish and the forward they wrap, bit for bit."""
    from diffqcqp_amd import diagnostics, diffqcqp, ops
    eps, max_iter = 1e-4, 1000
    for kind in C.KINDS:
        d, x = C.problem(kind, 8, 37, "dense")
        k = R.KIND[kind]
        t = {n: dev(v) for n, v in d.items()}
        ex = [t[n] for n in C.EXTRAS[kind]]
        xd = dev(x)
        ref = ops._polish(k, t["P"], t["q"], ex, xd, 5, DENSE, return_info=True)
        front = {"qp": lambda **kw: ops.qp_polish(t["P"], t["q"], xd, **kw),
                 "qcqp": lambda **kw: ops.qcqp_polish(t["P"], t["q"], t.get("l_n"), t.get("mu"), xd, **kw),
                 "box": lambda **kw: ops.boxqp_polish(t["P"], t["q"], t.get("l_min"), t.get("l_max"), xd, **kw),
                 "sbox": lambda **kw: ops.boxqp_polish(t["P"], t["q"], t.get("l_min"), t.get("l_max"), xd, v=t.get("v"), **kw)}[kind]
        got = front(max_steps=5, layout=DENSE, return_info=True)
        assert all(torch.equal(a, b) for a, b in zip(got, ref)), kind
        out = torch.empty_like(xd)
        assert front(max_steps=5, layout=DENSE, out=out) is out and torch.equal(out, ref[0])
        assert torch.equal(front(), ops._polish(k, t["P"], t["q"], ex, xd))            # the defaults: 8 steps, DQQ_P_AUTO
        # forward + polish + check on one stream
        solve = {"qp": diagnostics.solve_qp_polished, "qcqp": diagnostics.solve_qcqp_polished,
                 "box": diagnostics.solve_boxqp_polished, "sbox": diagnostics.solve_signedboxqp_polished}[kind]
        fwd = ops._forward(k, t["P"], t["q"], ex, eps, max_iter, layout=DENSE)
        pol = ops._polish(k, t["P"], t["q"], ex, fwd, 8, DENSE, return_info=True)
        st, resid, _ = ops.solution_check(k, t["P"], t["q"], ex, pol[0], layout=DENSE)
        for home in ("cuda", "cpu"):
            args = [t["P"], t["q"]] + ex
            xs, info, pinfo = solve(*[a.to(home) for a in args], eps, max_iter, layout="dense")
            assert xs.device.type == home and info.natural.device.type == home and pinfo.steps.device.type == home
            assert torch.equal(xs.cuda(), pol[0]) and torch.equal(info.natural.cuda(), resid[:, 0]), (kind, home)
            assert torch.equal(pinfo.before.cuda(), pol[1][:, 0]) and torch.equal(pinfo.after.cuda(), pol[1][:, 1])
            assert torch.equal(pinfo.steps.cuda(), pol[2]) and torch.equal(pinfo.status.cuda(), pol[3])
        # one problem, numpy in and out
        b = 3
        one = {"qp": lambda: diffqcqp.polishQP(d["P"][b], d["q"][b], x[b], 5),
               "qcqp": lambda: diffqcqp.polishQCQP(d["P"][b], d["q"][b], d.get("l_n", x)[b], d.get("mu", x)[b], x[b], 5),
               "box": lambda: diffqcqp.polishBoxQP(d["P"][b], d["q"][b], d.get("l_min", x)[b], d.get("l_max", x)[b], x[b], 5),
               "sbox": lambda: diffqcqp.polishBoxQP(d["P"][b], d["q"][b], d.get("l_min", x)[b], d.get("l_max", x)[b], x[b], 5,
                                                    v=d.get("v", x)[b])}[kind]()
        ref1 = ops._polish(k, t["P"][b:b + 1], t["q"][b:b + 1], [e[b:b + 1] for e in ex], xd[b:b + 1], 5, return_info=True)
        assert C.same_bits(one[0], ref1[0].cpu().numpy().reshape(-1)) and one[0].shape == (8,)
        assert one[1] == tuple(ref1[1].cpu().numpy()[0]) and one[2] == int(ref1[2]) and one[3] == int(ref1[3])


def test_out_that_overlaps_x_is_in_place_or_refused(oracle):
    from diffqcqp_amd import ops
    d, x = C.problem("qp", 8, 37, "dense")
    P, q = dev(d["P"]), dev(d["q"])
    ref = ops._polish(0, P, q, (), dev(x), 8, DENSE)
    buf = torch.zeros(38 * 8, dtype=torch.float64, device="cuda")
    xa = buf[:37 * 8].view(37, 8, 1)
    xa.copy_(dev(x))
    alias = buf[:37 * 8].view(37, 8, 1)                      # another tensor over x's memory: in place
    assert alias is not xa and torch.equal(ops._polish(0, P, q, (), xa, 8, DENSE, out=alias), ref) and torch.equal(xa, ref)
    xa.copy_(dev(x))
    before = buf.clone()
    with pytest.raises(ValueError, match="overlaps"):
        ops._polish(0, P, q, (), xa, 8, DENSE, out=buf[8:].view(37, 8, 1))   # shifted by one problem
    torch.cuda.synchronize()
    assert torch.equal(buf, before)                          # refused before any launch
