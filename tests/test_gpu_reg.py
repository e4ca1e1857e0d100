"""The proximal weight of the Newton family on the device (-m gpu): dqq_polish_reg_f64, dqq_newton_bwd_reg_f64,
dqq_newton_jvp_reg_f64 and dqq_newton_jac_reg_f64 on every route family and kind against the host core
(tests/hostcore/reg_core_check.cpp, held bit-equal to the numpy restatement on the CPU) bit for bit -- every output, status, steps
and both residuals --, on batches whose free block is singular (tests/reg_cases.py); a diagonal P through the general kernels;
Jacobian columns against the JVP; reg = 0 against the parent entries; a NaN and a one-sided problem in the middle of the batch; a
batch slice that starts at an odd problem and the empty batch; the adjoint identity; and the Functions under
set_default_newton_reg against the ops, in both modes, and replayed from a captured graph."""
import numpy as np
import pytest
import torch

import jvp_cases as JC
import polish_reference as R
import reg_cases as C

pytestmark = pytest.mark.gpu

AUTO, DENSE, DIAG = 0, C.DENSE, C.DIAG
CASES = [(k,) + r for k in C.KINDS for r in C.ROWS]


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()


def col(a):
    return None if a is None else dev(a[:, :, None])


def host(t):
    return None if t is None else t.cpu().numpy().reshape(t.shape[0], -1) if t.dim() == 3 and t.shape[2] == 1 else t.cpu().numpy()


def problem(kind, N, B, mode, layout):
    """-> (P as the layout takes it, q, ex, x (B,N), x0 a start for the polish, tangents as the layout takes them, g)"""
    d = C.batch(kind, N, mode, B)
    P = d["pdiag"] if layout == DIAG else d["P"]
    tan, g = C.inputs(kind, N, B)
    if layout == DIAG:
        tan = (np.ascontiguousarray(np.einsum("bii->bi", tan[0])),) + tuple(tan[1:])
    x0 = np.stack([R.project(kind, d["x"][b] + 1e-3 * np.sin(np.arange(N) + b), tuple(e[b] for e in d["ex"]), N) for b in range(B)])
    return P, d["q"], d["ex"], d["x"], x0, tan, g


def gpu_all(kind, P, q, ex, x, x0, tan, g, layout, reg, **kw):
    """Every entry once -> dict of numpy outputs."""
    from diffqcqp_amd import ops
    k = R.KIND[kind]
    Pd, qd, exd = dev(P), col(q), [col(e) for e in ex]
    t = [dev(tan[0])] + [col(v) for v in tan[1:]] + [None] * (4 - len(tan))
    out = {}
    dx, st = ops._newton_jvp(k, Pd, qd, exd, col(x), t, layout, return_status=True, reg=reg, **kw)
    out["jvp"] = (host(dx), st.cpu().numpy())
    b = ops._newton_backward(k, Pd, qd, exd, col(x), col(g), (True,) * 4, layout, return_status=True, reg=reg, **kw)
    b = tuple(b) if kind != "qp" else (b[0], b[1], None, None, b[2])
    out["bwd"] = tuple(host(v) for v in b[:4]) + (b[4].cpu().numpy(),)
    j = ops._newton_jacobian(k, Pd, qd, exd, col(x), (True,) * 3, layout, return_status=True, reg=reg, **kw)
    j = tuple(j) if kind != "qp" else (j[0], None, None, j[1])
    out["jac"] = tuple(None if v is None else v.cpu().numpy() for v in j[:3]) + (j[3].cpu().numpy(),)
    p = ops._polish(k, Pd, qd, exd, col(x0), 8, layout, return_info=True, reg=reg, **kw)
    out["polish"] = (host(p[0]), p[1].cpu().numpy(), p[2].cpu().numpy(), p[3].cpu().numpy())
    torch.cuda.synchronize()
    return out


def host_all(kind, P, q, ex, x, x0, tan, g, layout, reg, inf_ok=False):
    diag = layout == DIAG
    return {"jvp": C.host_jvp(kind, P, q, ex, x, tan, reg, diag, inf_ok), "bwd": C.host_backward(kind, P, q, ex, x, g, reg, diag, inf_ok),
            "jac": C.host_jacobian(kind, P, q, ex, x, reg, diag, inf_ok), "polish": C.host_polish(kind, P, q, ex, x0, 8, reg, diag, inf_ok)}


def assert_same(got, want, where):
    for name in want:
        for i, (a, b) in enumerate(zip(got[name], want[name])):
            if b is not None and b.dtype == np.int32:
                assert np.array_equal(a, b), (where, name, i, a, b)
            else:
                assert C.same_bits(a, b), (where, name, i)


@pytest.mark.parametrize("kind,family,N,B,mode,layout", CASES, ids=lambda v: str(v))
def test_every_entry_is_the_host_core(kind, family, N, B, mode, layout):
    """On a singular free block: bit for bit at every weight; status 0 and finite numbers from 1e-7 on; and what reg = 0 does
    there -- the parents' status 1 or numbers beyond 1e8 -- bit for bit too."""
    args = problem(kind, N, B, mode, layout)
    for reg in C.REGS + (0.0,):
        got, want = gpu_all(kind, *args, layout, reg), host_all(kind, *args, layout, reg)
        assert_same(got, want, (kind, family, N, reg))
        if reg >= C.REG:
            assert not got["jvp"][1].any() and not got["bwd"][4].any() and not got["jac"][3].any()
            assert np.isfinite(got["jvp"][0]).all() and all(np.isfinite(a).all() for a in got["bwd"][:4] if a is not None)
            assert (got["polish"][1][:, 1] <= got["polish"][1][:, 0]).all()
        if reg == 0.0:
            dx, s = got["jvp"]
            assert ((s == 1) | ((s == 0) & (np.abs(np.nan_to_num(dx)).max(axis=1) > 1e8))).all()
        if reg == C.REG and N <= 20:
            grads = [got["bwd"][0], got["bwd"][1]] + ([got["bwd"][2], got["bwd"][3]] if kind != "qp" else [])
            assert JC.adjoint_gap(args[6], got["jvp"][0], grads, args[5]) <= 10 * C.ADJOINT_GAP_CPU[kind]   # (compact dP, grad_P pair up)


@pytest.mark.parametrize("kind", C.KINDS)
def test_diagonal_P_as_a_matrix_and_jacobian_columns(kind):
    """A diagonal P given as (B,N,N) gives DQQ_P_DIAG's bits; column j of the Jacobians is the JVP's dx for e_j."""
    from diffqcqp_amd import ops
    N, B, reg = 8, 37, C.REG
    d = C.batch(kind, N, "diagzero", B)
    full = problem(kind, N, B, "diagzero", DENSE)
    comp = problem(kind, N, B, "diagzero", DIAG)
    tan0 = (None,) + tuple(full[5][1:])
    a = gpu_all(kind, *full[:5], tan0, full[6], DENSE, reg)
    b = gpu_all(kind, *comp[:5], tan0, comp[6], DIAG, reg)
    assert C.same_bits(a["jvp"][0], b["jvp"][0]) and np.array_equal(a["jvp"][1], b["jvp"][1])
    assert C.same_bits(a["bwd"][1], b["bwd"][1]) and C.same_bits(np.einsum("bii->bi", a["bwd"][0]), b["bwd"][0])
    assert all(C.same_bits(u, v) for u, v in zip(a["polish"], b["polish"]))
    # columns, on the rank-deficient dense batch
    P, q, ex, x = (C.batch(kind, N, "lowrank", B)[n] for n in ("P", "q", "ex", "x"))
    k = R.KIND[kind]
    Pd, qd, exd, xd = dev(P), col(q), [col(e) for e in ex], col(x)
    J = ops._newton_jacobian(k, Pd, qd, exd, xd, (True,) * 3, DENSE, reg=reg)
    ne = C.ne_of(kind, N)
    for which, width in ((0, N),) + (((1, ne), (2, ne)) if ne else ()):
        for j in range(width):
            e = torch.zeros((B, width, 1), dtype=torch.float64, device="cuda")
            e[:, j] = 1.0
            t = [None, None, None, None]
            t[which + 1] = e
            dx = ops._newton_jvp(k, Pd, qd, exd, xd, t, DENSE, reg=reg)
            assert torch.equal(J[which][:, :, j], dx[:, :, 0]), (which, j)


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("N,layout,mode", [(8, DIAG, "diagzero"), (20, DENSE, "lowrank"), (72, DENSE, "lowrank")])
def test_reg_zero_is_the_parent_entry(kind, N, layout, mode):
    """The *_reg_f64 entries at reg = 0, called directly, against the parent entries on the same inputs."""
    from diffqcqp_amd import _capi
    lib = _capi.lib()
    B = 5 if N > 64 else 37
    P, q, ex, x, x0, tan, g = problem(kind, N, B, mode, layout)
    k = R.KIND[kind]
    Pd, qd, xd, x0d, gd = dev(P), dev(q), dev(x), dev(x0), dev(g)
    exd = [dev(e) for e in ex]
    exp = [e.data_ptr() for e in exd] + [None] * (3 - len(exd))
    td = [dev(v) for v in tan] + [None] * (4 - len(tan))
    tp = [None if v is None else v.data_ptr() for v in td]
    ne = C.ne_of(kind, N)
    stream = torch.cuda.current_stream().cuda_stream
    need = max(lib.dqq_polish_scratch_bytes(k, N, B), lib.dqq_newton_scratch_bytes(k, N, B), lib.dqq_newton_jac_scratch_bytes(k, N, B))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device="cuda")
    wsa = (ws.data_ptr() if need else None, need, stream)
    shapes = C.jac_shapes(kind, B, N, layout == DIAG)

    def run(regged):
        mid = (0.0,) if regged else ()
        sfx = "_reg_f64" if regged else "_f64"
        o = {n: torch.full(s, 7.0, dtype=torch.float64, device="cuda") for n, s in
             (("dx", (B, N)), ("gP", P.shape), ("gq", (B, N)), ("ga", (B, max(ne, 1))), ("gb", (B, max(ne, 1))), ("xo", (B, N)),
              ("rs", (B, 2)), ("Jq", shapes[0]), ("Ja", shapes[1] if ne else (1,)), ("Jb", shapes[2] if ne else (1,)))}
        st = torch.full((5, B), -1, dtype=torch.int32, device="cuda")
        opt = lambda n: o[n].data_ptr() if ne else None
        rcs = [getattr(lib, "dqq_newton_jvp" + sfx)(k, Pd.data_ptr(), qd.data_ptr(), *exp, xd.data_ptr(), *tp, o["dx"].data_ptr(), B, N,
                                                    layout, *mid, st[0].data_ptr(), *wsa),
               getattr(lib, "dqq_newton_bwd" + sfx)(k, Pd.data_ptr(), qd.data_ptr(), *exp, xd.data_ptr(), gd.data_ptr(), o["gP"].data_ptr(),
                                                    o["gq"].data_ptr(), opt("ga"), opt("gb"), B, N, layout, *mid, st[1].data_ptr(), *wsa),
               getattr(lib, "dqq_newton_jac" + sfx)(k, Pd.data_ptr(), qd.data_ptr(), *exp, xd.data_ptr(), o["Jq"].data_ptr(), opt("Ja"),
                                                    opt("Jb"), B, N, layout, *mid, st[2].data_ptr(), *wsa),
               getattr(lib, "dqq_polish" + sfx)(k, Pd.data_ptr(), qd.data_ptr(), *exp, x0d.data_ptr(), o["xo"].data_ptr(), B, N, 8, layout,
                                                *mid, o["rs"].data_ptr(), st[3].data_ptr(), st[4].data_ptr(), *wsa)]
        torch.cuda.synchronize()
        assert rcs == [0, 0, 0, 0]
        return {n: v.cpu().numpy() for n, v in o.items()}, st.cpu().numpy()

    (a, sa), (b, sb) = run(True), run(False)
    assert np.array_equal(sa, sb)
    for n in a:
        assert C.same_bits(a[n], b[n]), n


@pytest.mark.parametrize("kind", ("box", "sbox"))
@pytest.mark.parametrize("N,layout,mode", [(8, DIAG, "diagzero"), (20, DENSE, "lowrank"), (72, DENSE, "lowrank")])
def test_bad_and_one_sided_problems_touch_no_other_row(kind, N, layout, mode):
    """A NaN problem and an infinite-bound problem in the middle of the batch: status 2 for both without the flag, the one-sided
    box ordinary input with it; every other row as the host core has it."""
    B = 5 if N > 64 else 37
    P, q, ex, x, x0, tan, g = problem(kind, N, B, mode, layout)
    q, ex = q.copy(), [e.copy() for e in ex]
    nan_row, inf_row = B // 2, B // 2 + 1
    q[nan_row, N // 2] = np.nan
    free = np.nonzero(C.batch(kind, N, mode, B)["free"][inf_row])[0]
    ex[1][inf_row, free] = np.inf            # upper bounds of free coordinates: never sat on
    args = (P, q, tuple(ex), x, x0, tan, g)
    for flag in (False, True):
        got = gpu_all(kind, *args, layout, C.REG, infinite_bounds=flag)
        want = host_all(kind, *args, layout, C.REG, inf_ok=flag)
        assert_same(got, want, (kind, N, flag))
        assert got["jvp"][1][nan_row] == 2 and got["jvp"][1][inf_row] == (0 if flag else 2)
        others = np.ones(B, dtype=bool)
        others[[nan_row, inf_row]] = False
        assert (got["jvp"][1][others] == 0).all() and (got["polish"][3][others] < 2).all()


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("N,layout,mode", [(8, DIAG, "diagzero"), (8, DENSE, "lowrank"), (20, DENSE, "lowrank")])
def test_sliced_and_empty_batches(kind, N, layout, mode):
    """A batch that is a slice starting at an odd problem: its own rows bit for bit, the rows around it untouched; B = 0: nothing."""
    from diffqcqp_amd import ops
    B = 37
    P, q, ex, x, x0, tan, g = problem(kind, N, B, mode, layout)
    k = R.KIND[kind]
    lo, hi = 3, 32
    full = dict(P=dev(P), q=col(q), x=col(x), x0=col(x0), ex=[col(e) for e in ex])
    sl = lambda t: t[lo:hi]
    out = torch.full((B, N, 1), 7.0, dtype=torch.float64, device="cuda")
    ops._newton_jvp(k, sl(full["P"]), sl(full["q"]), [sl(e) for e in full["ex"]], sl(full["x"]), [None, sl(col(tan[1])), None, None], layout,
                    out=out[lo:hi], reg=C.REG)
    want = C.host_jvp(kind, P[lo:hi], q[lo:hi], tuple(e[lo:hi] for e in ex), x[lo:hi], (None, tan[1][lo:hi]), C.REG, layout == DIAG)[0]
    assert C.same_bits(host(out[lo:hi]), want)
    assert (out[:lo] == 7.0).all().item() and (out[hi:] == 7.0).all().item()
    out.fill_(7.0)
    ops._polish(k, sl(full["P"]), sl(full["q"]), [sl(e) for e in full["ex"]], sl(full["x0"]), 8, layout, out=out[lo:hi], reg=C.REG)
    want = C.host_polish(kind, P[lo:hi], q[lo:hi], tuple(e[lo:hi] for e in ex), x0[lo:hi], 8, C.REG, layout == DIAG)[0]
    assert C.same_bits(host(out[lo:hi]), want)
    assert (out[:lo] == 7.0).all().item() and (out[hi:] == 7.0).all().item()
    e0 = lambda t: t[:0]
    r = ops._newton_jvp(k, e0(full["P"]), e0(full["q"]), [e0(e) for e in full["ex"]], e0(full["x"]), [None] * 4, layout, reg=C.REG)
    assert r.shape == (0, N, 1)
    r = ops._polish(k, e0(full["P"]), e0(full["q"]), [e0(e) for e in full["ex"]], e0(full["x0"]), 8, layout, reg=C.REG)
    assert r.shape == (0, N, 1)


def _functions(kind):
    from diffqcqp_amd import qcqp
    return {"qp": qcqp.QPFn2, "qcqp": qcqp.QCQPFn2, "box": qcqp.BoxQPFn2, "sbox": qcqp.SignedBoxQPDiffFn2}[kind]


@pytest.mark.parametrize("kind", C.KINDS)
def test_functions_under_the_default_reg(kind):
    """set_default_derivative("newton"), set_default_newton_reg(1e-7), set_default_polish(8) on a rank-deficient batch: finite
    gradients equal to the ops calls at the saved x, torch.func.jvp equal to the op and adjoint to the backward; the Function's
    apply and autograd.grad replayed from a captured graph: the same bits."""
    from diffqcqp_amd import ops, qcqp
    N, B = 8, 37
    k = R.KIND[kind]
    d = C.batch(kind, N, "lowrank", B)
    ins = [dev(d["P"]), col(d["q"])] + [col(e) for e in d["ex"]]
    nd = 2 + min(len(ins) - 2, 2)
    fn = _functions(kind)
    g = col(C.inputs(kind, N, B)[1])
    eps, max_iter = 1e-4, 1000
    assert qcqp.get_default_newton_reg() == 0.0
    with pytest.raises(ValueError):
        qcqp.set_default_newton_reg(-1.0)
    with pytest.raises(ValueError):
        qcqp.set_default_newton_reg(float("nan"))

    def run(leaves):
        x = fn.apply(*leaves, *ins[nd:], None, eps, max_iter)
        return x.detach(), torch.autograd.grad(x, leaves, g)

    prev = (qcqp.set_default_polish(8), qcqp.set_default_derivative("newton"), qcqp.set_default_newton_reg(C.REG))
    try:
        assert qcqp.get_default_newton_reg() == C.REG
        leaves = [a.clone().requires_grad_(True) for a in ins[:nd]]
        x, grads = run(leaves)
        assert all(torch.isfinite(a).all().item() for a in grads)
        x_fwd = ops._forward(k, ins[0], ins[1], ins[2:], eps, max_iter, 1e-7, True, AUTO)
        assert torch.equal(x, ops._polish(k, ins[0], ins[1], ins[2:], x_fwd, 8, reg=C.REG))
        out = ops._newton_backward(k, ins[0], ins[1], ins[2:], x, g, (True,) * 4, reg=C.REG, return_status=True)
        assert not out[-1].any().item()
        for a, b in zip(grads, out[:-1]):
            assert torch.equal(a, b)
        # forward mode through the Function: _jvp_leaf reads the default weight; equal to the op, adjoint to the backward
        tan = C.inputs(kind, N, B)[0]
        tans = [dev(tan[0])] + [col(v) for v in tan[1:]]
        f = lambda *a: fn.apply(*a, *ins[nd:], None, eps, max_iter)   # noqa: E731
        xj, dxj = torch.func.jvp(f, tuple(ins[:nd]), tuple(tans[:nd]))
        assert torch.equal(xj, x)
        assert torch.equal(dxj, ops._newton_jvp(k, ins[0], ins[1], ins[2:], x, tans + [None] * (4 - len(tans)), reg=C.REG))
        gh = [host(a) if a.dim() == 3 and a.shape[2] == 1 else a.cpu().numpy() for a in grads]
        assert JC.adjoint_gap(host(g), host(dxj), gh, tan) <= 10 * C.ADJOINT_GAP_CPU[kind]
        # the Function itself -- apply and autograd.grad, which read the defaults -- captured and replayed
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            run(leaves)                                          # warm-up on the capture stream
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                xg, gg = run(leaves)
        torch.cuda.current_stream().wait_stream(stream)
        xg.zero_()
        for o in gg:
            o.zero_()
        qcqp.set_default_newton_reg(0.0)     # the replay carries the weight it was captured with: a launch argument
        graph.replay()
        torch.cuda.synchronize()
        qcqp.set_default_newton_reg(C.REG)
        assert torch.equal(xg, x)
        for a, b in zip(gg, grads):
            assert torch.equal(a, b)
    finally:
        qcqp.set_default_polish(prev[0])
        qcqp.set_default_derivative(prev[1])
        qcqp.set_default_newton_reg(prev[2])
    assert qcqp.get_default_newton_reg() == 0.0
