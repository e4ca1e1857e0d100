"""dqq_polish_smooth_f64, dqq_newton_bwd_smooth_f64 and dqq_newton_jvp_smooth_f64 on the device (-m gpu): every route family and
kind against the host core (tests/hostcore/smooth_core_check.cpp, held bit-equal to the numpy restatement on the CPU) bit for bit
on every output -- x_out, both residuals, steps, status, halvings; all gradients; dx --, at kappa in {1e-4, 1e-2}; then the
properties of the entry points: a batch slice from an odd problem, in place, a NaN and an Inf problem in the middle of a tile,
max_steps = 0, reg > 0, kappa = 0 against the parents' entries, a diagonal P given as (B,N,N) against DQQ_P_DIAG, the Python
fronts and what they are for: gradients of inactive bounds that are not zero.  Inputs: tests/smooth_cases.py."""
import numpy as np
import pytest
import torch

import polish_reference as R
import smooth_cases as SC

pytestmark = pytest.mark.gpu

AUTO, DENSE, DIAG = SC.C.PC.AUTO, SC.C.PC.DENSE, SC.C.PC.DIAG
H = 8
DIAG_ROWS, TEAM_ROWS, ANY_ROWS = SC.DIAG_ROWS, SC.TEAM_ROWS, SC.ANY_ROWS
POLISH = ("x_out", "resid", "steps", "status", "halvings")
BWD = ("grad_P", "grad_q", "grad_a", "grad_b", "status")
JVP = ("dx", "status")


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()


def _ws(group, k, N, n):
    from diffqcqp_amd import ops
    ws = (ops.polish_workspace if group == "polish" else ops.newton_workspace)(torch.device("cuda"), k, N, n)
    return (None, 0) if ws is None else (ws, ws.numel() * 4)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def polish(kind, P, q, ex, x, layout, kappa, max_steps=SC.MAX_STEPS, h=H, reg=0.0, in_place=False, first=0, parent=False):
    """dqq_polish_smooth_f64 itself (parent: dqq_polish_ls_f64) on flat numpy arrays, the problems from `first` on as views into
    the full batch's memory.  -> numpy (x_out, resid, steps, status, halvings)"""
    from diffqcqp_amd import _capi
    lib = _capi.lib()
    B, N = x.shape
    k = R.KIND[kind]
    full = [dev(SC.compact(P) if (layout & 0xff) == DIAG else P), dev(q)] + [dev(e) for e in ex] + [dev(x)]
    t = [a[first:] for a in full]
    assert all(a.is_contiguous() for a in t)
    n = B - first
    xo = t[-1] if in_place else torch.full((n, N), 7.0, dtype=torch.float64, device="cuda")
    resid = torch.empty((n, 2), dtype=torch.float64, device="cuda")
    steps, status, halv = (torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(3))
    ws, wb = _ws("polish", k, N, n)
    exp = [a.data_ptr() for a in t[2:-1]] + [None] * (3 - len(ex))
    head = (k, t[0].data_ptr(), t[1].data_ptr(), *exp, t[-1].data_ptr(), xo.data_ptr(), n, N, max_steps, layout, reg)
    tail = (h, resid.data_ptr(), steps.data_ptr(), status.data_ptr(), halv.data_ptr(), None if ws is None else ws.data_ptr(), wb, _stream())
    rc = lib.dqq_polish_ls_f64(*head, *tail) if parent else lib.dqq_polish_smooth_f64(*head, kappa, *tail)
    assert rc == 0
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in (xo, resid, steps, status, halv))


def backward(kind, P, q, ex, x, gx, layout, kappa, reg=0.0, first=0, parent=False):
    """dqq_newton_bwd_smooth_f64 (parent: dqq_newton_bwd_reg_f64) -> numpy (grad_P, grad_q, grad_a, grad_b, status)"""
    from diffqcqp_amd import _capi
    lib = _capi.lib()
    B, N = x.shape
    k, diag = R.KIND[kind], (layout & 0xff) == DIAG
    t = [a[first:] for a in [dev(SC.compact(P) if diag else P), dev(q)] + [dev(e) for e in ex] + [dev(x), dev(gx)]]
    n = B - first
    gP = torch.full((n, N) if diag else (n, N, N), 7.0, dtype=torch.float64, device="cuda")
    gq = torch.full((n, N), 7.0, dtype=torch.float64, device="cuda")
    ne = 0 if kind == "qp" else (N // 2 if kind == "qcqp" else N)
    ga, gb = ((torch.full((n, ne), 7.0, dtype=torch.float64, device="cuda") for _ in range(2)) if ne else (None, None))
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ws, wb = _ws("newton", k, N, n)
    exp = [a.data_ptr() for a in t[2:-2]] + [None] * (3 - len(ex))
    head = (k, t[0].data_ptr(), t[1].data_ptr(), *exp, t[-2].data_ptr(), t[-1].data_ptr(), gP.data_ptr(), gq.data_ptr(),
            None if ga is None else ga.data_ptr(), None if gb is None else gb.data_ptr(), n, N, layout, reg)
    tail = (status.data_ptr(), None if ws is None else ws.data_ptr(), wb, _stream())
    rc = lib.dqq_newton_bwd_reg_f64(*head, *tail) if parent else lib.dqq_newton_bwd_smooth_f64(*head, kappa, *tail)
    assert rc == 0
    torch.cuda.synchronize()
    return tuple(None if a is None else a.cpu().numpy() for a in (gP, gq, ga, gb, status))


def jvp(kind, P, q, ex, x, tang, layout, kappa, reg=0.0, first=0, parent=False):
    """dqq_newton_jvp_smooth_f64 (parent: dqq_newton_jvp_reg_f64); tang = (dP, dq, da, db), None = NULL -> numpy (dx, status)"""
    from diffqcqp_amd import _capi
    lib = _capi.lib()
    B, N = x.shape
    k, diag = R.KIND[kind], (layout & 0xff) == DIAG
    t = [a[first:] for a in [dev(SC.compact(P) if diag else P), dev(q)] + [dev(e) for e in ex] + [dev(x)]]
    tg = [None if a is None else dev(SC.compact(a) if (diag and i == 0) else a)[first:] for i, a in enumerate(tang)]
    n = B - first
    dx = torch.full((n, N), 7.0, dtype=torch.float64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ws, wb = _ws("newton", k, N, n)
    exp = [a.data_ptr() for a in t[2:-1]] + [None] * (3 - len(ex))
    head = (k, t[0].data_ptr(), t[1].data_ptr(), *exp, t[-1].data_ptr(), *[None if a is None else a.data_ptr() for a in tg], dx.data_ptr(),
            n, N, layout, reg)
    tail = (status.data_ptr(), None if ws is None else ws.data_ptr(), wb, _stream())
    rc = lib.dqq_newton_jvp_reg_f64(*head, *tail) if parent else lib.dqq_newton_jvp_smooth_f64(*head, kappa, *tail)
    assert rc == 0
    torch.cuda.synchronize()
    return dx.cpu().numpy(), status.cpu().numpy()


def assert_same(names, got, ref, what=""):
    for name, g, r in zip(names, got, ref):
        if g is None and r is None:
            continue
        assert g.dtype == r.dtype and SC.same_bits(g, r), "%s %s: %s vs %s" % (what, name, g.reshape(-1)[:4], r.reshape(-1)[:4])


def _pc(P, layout):
    return SC.compact(P) if (layout & 0xff) == DIAG else P


def hosts(kind, P, q, ex, x, layout, kappa, structure, max_steps=SC.MAX_STEPS, h=H, reg=0.0):
    """The host core's polish from x, and its two derivatives at the polished point.  -> (polish, xs, backward, jvp, tangents)"""
    diag = (layout & 0xff) == DIAG
    B, N = x.shape
    dP, dq, da, db, gx = SC.tangents(kind, N, B, structure)
    pol = SC.host_polish(kind, _pc(P, layout), q, ex, x, max_steps, h, reg, kappa, diag=diag)
    xs = pol[0]
    bwd = SC.host_backward(kind, _pc(P, layout), q, ex, xs, gx, reg, kappa, diag=diag)
    jv = SC.host_jvp(kind, _pc(P, layout), q, ex, xs, _pc(dP, layout), dq, da, db, reg, kappa, diag=diag)
    return pol, xs, bwd, jv, (dP, dq, da, db, gx)


def family_checks(kind, N, Bs, layout, structure):
    """The bit equality of all three entries on every B of the family at both kappa, and on the middle B the properties of the
    entry points."""
    for kappa in SC.KAPPAS:
        for B in Bs:
            P, q, ex, x = SC.problem(kind, N, B, structure)
            pol, xs, bwd, jv, (dP, dq, da, db, gx) = hosts(kind, P, q, ex, x, layout, kappa, structure)
            what = "%s N=%d B=%d kappa=%g" % (kind, N, B, kappa)
            print("%s layout %d: status 0 on %d, steps up to %d, halvings up to %d, worst r_kappa after %.2e" % (
                what, layout, (pol[3] == 0).sum(), pol[2].max(), pol[4].max(), pol[1][:, 1].max()))
            assert_same(POLISH, polish(kind, P, q, ex, x, layout, kappa), pol, what)
            assert_same(BWD, backward(kind, P, q, ex, xs, gx, layout, kappa), bwd, what)
            assert_same(JVP, jvp(kind, P, q, ex, xs, (dP, dq, da, db), layout, kappa), jv, what)
            assert (pol[3] == 0).sum() >= (B + 1) // 2 and not bwd[4].any() and not jv[1].any()
    kappa = SC.KAPPAS[1]
    B = Bs[1]
    P, q, ex, x = SC.problem(kind, N, B, structure)
    pol, xs, bwd, jv, (dP, dq, da, db, gx) = hosts(kind, P, q, ex, x, layout, kappa, structure)
    cut = lambda ref, f=3: tuple(None if r is None else r[f:] for r in ref)
    assert_same(POLISH, polish(kind, P, q, ex, x, layout, kappa, first=3), cut(pol), "a slice from an odd problem")
    assert_same(BWD, backward(kind, P, q, ex, xs, gx, layout, kappa, first=3), cut(bwd), "a slice from an odd problem")
    assert_same(JVP, jvp(kind, P, q, ex, xs, (dP, dq, da, db), layout, kappa, first=3), cut(jv), "a slice from an odd problem")
    assert_same(POLISH, polish(kind, P, q, ex, x, layout, kappa, in_place=True), pol, "in place")
    zero = polish(kind, P, q, ex, x, layout, kappa, 0)
    assert SC.same_bits(zero[0], x) and not zero[2].any() and not zero[4].any() and (zero[3] == 1).all()
    assert SC.same_bits(zero[1][:, 0], pol[1][:, 0]) and SC.same_bits(zero[1][:, 1], pol[1][:, 0])
    # the proximal weight, fewer halvings, absent tangents
    pr, xr, br, jr, _ = hosts(kind, P, q, ex, x, layout, kappa, structure, 5, 1, 1e-3)
    assert_same(POLISH, polish(kind, P, q, ex, x, layout, kappa, 5, 1, 1e-3), pr, "reg")
    assert_same(BWD, backward(kind, P, q, ex, xr, gx, layout, kappa, 1e-3), br, "reg")
    assert_same(JVP, jvp(kind, P, q, ex, xr, (dP, dq, da, db), layout, kappa, 1e-3), jr, "reg")
    diag = (layout & 0xff) == DIAG
    assert_same(JVP, jvp(kind, P, q, ex, xs, (None, dq, None, db), layout, kappa),
                SC.host_jvp(kind, _pc(P, layout), q, ex, xs, None, dq, None, db, 0.0, kappa, diag=diag), "NULL tangents")
    # a NaN problem and an Inf problem in the middle of a tile: status 2, x kept, NaN derivatives, no other row changes
    P2, x2, xs2 = np.array(P), np.array(x), np.array(xs)
    m1, m2 = B // 2, B // 2 + 1
    x2[m1, N - 1] = xs2[m1, N - 1] = np.nan
    P2[m2, 1, 1] = np.inf
    keep = np.ones(B, dtype=bool)
    keep[[m1, m2]] = False
    bad = polish(kind, P2, q, ex, x2, layout, kappa)
    assert_same(POLISH, bad, SC.host_polish(kind, _pc(P2, layout), q, ex, x2, SC.MAX_STEPS, H, 0.0, kappa, diag=diag), "with bad rows")
    assert bad[3][m1] == 2 and bad[3][m2] == 2 and SC.same_bits(bad[0][[m1, m2]], x2[[m1, m2]]) and not bad[2][[m1, m2]].any()
    assert_same(POLISH, tuple(g[keep] for g in bad), tuple(r[keep] for r in pol), "other rows")
    badb = backward(kind, P2, q, ex, xs2, gx, layout, kappa)
    assert_same(BWD, badb, SC.host_backward(kind, _pc(P2, layout), q, ex, xs2, gx, 0.0, kappa, diag=diag), "with bad rows")
    assert list(badb[4][[m1, m2]]) == [2, 2] and np.isnan(badb[1][[m1, m2]]).all()
    assert_same(BWD, cut(tuple(None if g is None else g[keep] for g in badb), 0), tuple(None if r is None else r[keep] for r in bwd), "other rows")
    badj = jvp(kind, P2, q, ex, xs2, (dP, dq, da, db), layout, kappa)
    assert list(badj[1][[m1, m2]]) == [2, 2] and np.isnan(badj[0][[m1, m2]]).all()
    assert_same(JVP, tuple(g[keep] for g in badj), tuple(r[keep] for r in jv), "other rows")


@pytest.mark.parametrize("kind,N", DIAG_ROWS)
def test_diagonal_kernels_are_the_host_core(kind, N):
    family_checks(kind, N, SC.diag_bs(N), DIAG, "diag")


@pytest.mark.parametrize("kind,N", TEAM_ROWS)
def test_team_kernels_are_the_host_core(kind, N):
    family_checks(kind, N, SC.TEAM_BS, SC.team_layout(N), "dense")


@pytest.mark.parametrize("kind,N", ANY_ROWS)
def test_global_memory_kernels_are_the_host_core(kind, N):
    P, q, ex, x = SC.problem(kind, N, 3, "dense")
    cut = lambda ref: tuple(None if r is None else r[1:] for r in ref)
    for kappa in SC.KAPPAS:
        pol, xs, bwd, jv, (dP, dq, da, db, gx) = hosts(kind, P, q, ex, x, DENSE, kappa, "dense")
        assert_same(POLISH, polish(kind, P, q, ex, x, DENSE, kappa), pol, kind)
        assert_same(BWD, backward(kind, P, q, ex, xs, gx, DENSE, kappa), bwd, kind)
        assert_same(JVP, jvp(kind, P, q, ex, xs, (dP, dq, da, db), DENSE, kappa), jv, kind)
        assert (pol[3] == 0).all() and not bwd[4].any() and not jv[1].any()
        assert_same(POLISH, polish(kind, P, q, ex, x, DENSE, kappa, first=1), cut(pol), "a slice from an odd problem")
        assert_same(BWD, backward(kind, P, q, ex, xs, gx, DENSE, kappa, first=1), cut(bwd), "a slice from an odd problem")
        assert_same(JVP, jvp(kind, P, q, ex, xs, (dP, dq, da, db), DENSE, kappa, first=1), cut(jv), "a slice from an odd problem")
        assert_same(POLISH, polish(kind, P, q, ex, x, DENSE, kappa, in_place=True), pol, "in place")
        zero = polish(kind, P, q, ex, x, DENSE, kappa, 0)
        assert SC.same_bits(zero[0], x) and (zero[3] == 1).all() and not zero[4].any()
        pr, xr, br, jr, _ = hosts(kind, P, q, ex, x, DENSE, kappa, "dense", 5, 1, 1e-3)
        assert_same(POLISH, polish(kind, P, q, ex, x, DENSE, kappa, 5, 1, 1e-3), pr, "reg")
        assert_same(BWD, backward(kind, P, q, ex, xr, gx, DENSE, kappa, 1e-3), br, "reg")
        assert_same(JVP, jvp(kind, P, q, ex, xr, (dP, dq, da, db), DENSE, kappa, 1e-3), jr, "reg")
        # a NaN problem and an Inf problem: status 2, x kept, NaN derivatives, the third problem keeps its bits
        x2, xs2, P2 = np.array(x), np.array(xs), np.array(P)
        x2[1, N - 1] = xs2[1, N - 1] = np.nan
        P2[0, 1, 1] = np.inf
        bad = polish(kind, P2, q, ex, x2, DENSE, kappa)
        assert list(bad[3][:2]) == [2, 2] and SC.same_bits(bad[0][:2], x2[:2]) and all(SC.same_bits(g[2:], r[2:]) for g, r in zip(bad, pol))
        badb = backward(kind, P2, q, ex, xs2, gx, DENSE, kappa)
        badj = jvp(kind, P2, q, ex, xs2, (dP, dq, da, db), DENSE, kappa)
        assert list(badb[4][:2]) == [2, 2] and np.isnan(badb[1][:2]).all() and list(badj[1][:2]) == [2, 2] and np.isnan(badj[0][:2]).all()
        assert_same(BWD, cut(cut(badb)), cut(cut(bwd)), "beside the bad rows")
        assert_same(JVP, cut(cut(badj)), cut(cut(jv)), "beside the bad rows")


@pytest.mark.parametrize("kind,N,B,layout,structure", [(k, 8, 37, DIAG, "diag") for k in SC.KINDS] + [(k, 8, 9, DENSE, "dense") for k in SC.KINDS] +
                         [("box", 20, 9, AUTO, "dense"), ("qp", 65, 3, DENSE, "dense")])
def test_kappa_zero_is_the_parents_bit_for_bit(kind, N, B, layout, structure):
    P, q, ex, x = SC.problem(kind, N, B, structure)
    dP, dq, da, db, gx = SC.tangents(kind, N, B, structure)
    for reg in (0.0, 1e-3):
        for h in (0, H):
            got = polish(kind, P, q, ex, x, layout, 0.0, h=h, reg=reg)
            assert_same(POLISH, got, polish(kind, P, q, ex, x, layout, 0.0, h=h, reg=reg, parent=True), "polish reg=%g h=%d" % (reg, h))
        xs = got[0]
        assert_same(BWD, backward(kind, P, q, ex, xs, gx, layout, 0.0, reg), backward(kind, P, q, ex, xs, gx, layout, 0.0, reg, parent=True), "backward")
        assert_same(JVP, jvp(kind, P, q, ex, xs, (dP, dq, da, db), layout, 0.0, reg),
                    jvp(kind, P, q, ex, xs, (dP, dq, da, db), layout, 0.0, reg, parent=True), "jvp")
    assert (got[3] == 0).any()
    assert_same(POLISH, got, SC.host_polish(kind, _pc(P, layout), q, ex, x, SC.MAX_STEPS, H, 1e-3, 0.0, diag=layout == DIAG), "host core at kappa = 0")


@pytest.mark.parametrize("kind", SC.KINDS)
@pytest.mark.parametrize("N", SC.DIAG_MATRIX_N)
def test_a_diagonal_P_given_as_a_matrix_gives_the_compact_bits(kind, N):
    """smooth_core.h guarantees it: an entry of M is an exact zero wherever P's is, and the elimination skips exact zeros."""
    kappa = 1e-2
    B = SC.diag_bs(N)[1]
    P, q, ex, x = SC.problem(kind, N, B, "diag")
    dP, dq, da, db, gx = SC.tangents(kind, N, B, "diag")
    pol = polish(kind, P, q, ex, x, DIAG, kappa)
    assert_same(POLISH, polish(kind, P, q, ex, x, AUTO, kappa), pol)
    c = backward(kind, P, q, ex, pol[0], gx, DIAG, kappa)
    d = backward(kind, P, q, ex, pol[0], gx, DENSE, kappa)
    assert SC.same_bits(SC.compact(d[0]), c[0])
    assert_same(BWD[1:], d[1:], c[1:])
    assert_same(JVP, jvp(kind, P, q, ex, pol[0], (dP, dq, da, db), DENSE, kappa), jvp(kind, P, q, ex, pol[0], (dP, dq, da, db), DIAG, kappa))


def test_inactive_bounds_get_gradients_through_the_public_ops():
    """What the feature is for, and the test that fails without it: at the hard solution the gradient of a bound that is not
    active is exactly +0.0; on the central path it is finite and not zero, and dx_i/dl_min_i > 0.  Also: the fronts' argument
    checks, and a captured graph of smoothed polish + smoothed backward replays the eager bits."""
    from diffqcqp_amd import ops
    kappa = 1e-2
    P, q, ex, x, xh, tang = SC.frozen("box")       # frozen with its hard solution: the same inputs on every host
    gx = tang[4]
    t = [dev(P), dev(q[:, :, None]), dev(ex[0][:, :, None]), dev(ex[1][:, :, None])]
    hard = dev(xh[:, :, None])
    gh = ops.boxqp_newton_backward(*t, hard, dev(gx[:, :, None]))
    xs, resid, steps, status = ops.boxqp_polish(*t, hard, max_steps=40, max_halvings=H, kappa=kappa, return_info=True)
    conv = resid[:, 1] <= SC.CONVERGED              # from a solution the smoothed polish converges on every problem
    assert (status.cpu().numpy() == 0).all() and conv.all().item()
    gs = ops.boxqp_newton_backward(*t, xs, dev(gx[:, :, None]), kappa=kappa)
    ref = SC.host_backward("box", P, q, ex, xs.cpu().numpy()[:, :, 0], gx, 0.0, kappa)
    assert_same(BWD[:4], tuple(g.cpu().numpy().reshape(r.shape) for g, r in zip(gs, ref[:4])), ref[:4])
    for hard_g, smooth_g in zip(gh[2:], gs[2:]):
        hz = (hard_g == 0.0).cpu().numpy()
        assert hz.any() and not np.signbit(hard_g.cpu().numpy()[hz]).any()
        sg = smooth_g.cpu().numpy()
        assert np.isfinite(sg).all() and (sg[hz] != 0.0).all()
    free = (gh[2] == 0.0) & (gh[3] == 0.0) & conv[:, None, None]             # inactive on both sides at the hard solution
    e = torch.zeros_like(xs)
    i = int(free[:, :, 0].sum(0).argmax())
    e[:, i] = 1.0
    dx = ops.boxqp_newton_jvp(*t, xs, dl_min=e, kappa=kappa)
    assert free[:, i].any().item() and (dx[:, i][free[:, i]] > 0.0).all()
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.boxqp_polish(*t, hard, kappa=bad)
    with pytest.raises(ValueError):
        ops.boxqp_newton_backward(*t, xs, dev(gx[:, :, None]), kappa=kappa, infinite_bounds=True)
    # captured
    xo, g = torch.zeros_like(xs), [torch.zeros_like(a) for a in gs]
    gxd = dev(gx[:, :, None])
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.boxqp_polish(*t, hard, max_steps=40, max_halvings=H, kappa=kappa, out=xo)
        ops.boxqp_newton_backward(*t, xo, gxd, kappa=kappa, out=g)
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            ops.boxqp_polish(*t, hard, max_steps=40, max_halvings=H, kappa=kappa, out=xo)
            ops.boxqp_newton_backward(*t, xo, gxd, kappa=kappa, out=g)
    torch.cuda.current_stream().wait_stream(stream)
    xo.zero_()
    for a in g:
        a.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(xo, xs) and all(torch.equal(a, b) for a, b in zip(g, gs))
