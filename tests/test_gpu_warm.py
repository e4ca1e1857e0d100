"""-m gpu: the warm-started forward (dqq_fwd_warm_f64, ops.*_forward_warm, the *WarmFn2 classes) on the device.

One row per forward family and kind: the rows of tests/param_cases.py (the smallest batch that reaches each family and lane
layout, every B with a ragged last tile), well-conditioned inputs (tests/warm_cases.py), each row also as a `t[1:]` slice.
Against tests/warm_reference.py -- the numpy restatement that tests/test_warm_reference.py pins to the oracle --:
  * x within 1e-6 of the problem's scale; iteration counts equal on >= 0.999 of the problems for N <= 16, >= 0.99 for the
    matrix-core kernel and for the reference-order kernels beyond N = 16 (their cold parity bars, tests/test_gpu_parity.py);
    with x0 = the solution of the 1 % perturbed problem, the problem's own solution, zero, and an infeasible point;
  * the device's total warm iterations are strictly below its total cold iterations on the same batch;
  * max_iter = 0 returns x0 bit for bit; a NaN x0 in one problem leaves every other problem's bits unchanged;
  * the same bits on every lane layout of the diagonal kernel, with and without DQQ_F_EXPECT_DENSE, fused against drained;
  * a captured warm forward + backward replays bit-equal to eager; QPWarmFn2's gradients are QPFn2's backward at the same x;
    x0 is read only and exactly sized (the guarded arena of tests/footprint_arena.py)."""
import numpy as np
import pytest
import torch

from footprint_arena import Arena, call_specs
from param_cases import DIAG, KIND, tile
from test_gpu_parity import npy
from warm_cases import EPS, EXTRAS, FWD, MAX_ITER, VARIANTS, reference, row_id

pytestmark = pytest.mark.gpu
XD = 0x200


@pytest.fixture(scope="module")
def ops():
    """The shipped library, the hint feedback off: the route of a call is then a function of its arguments alone."""
    assert torch.cuda.is_available(), "these tests need the GPU"
    from diffqcqp_amd import build, ops as _ops, _capi
    build.build()
    _capi.lib()
    was_on = _capi._feedback is not None
    _capi.enable_feedback(False)
    yield _ops
    _capi.enable_feedback(was_on)


def _dev(d, layout):
    g = {k: v.cuda() for k, v in d.items()}
    if (layout & 0xff) == DIAG:
        g["P"] = torch.diagonal(g["P"], dim1=1, dim2=2).contiguous()
    return g


def _fwd(ops, kind, g, layout, x0=None, max_iter=MAX_ITER):
    kw = dict(layout=layout, return_iters=True)
    if x0 is None:
        if kind == "qp":
            return ops.qp_forward(g["P"], g["q"], EPS, max_iter, **kw)
        if kind == "qcqp":
            return ops.qcqp_forward(g["P"], g["q"], g["l_n"], g["mu"], EPS, max_iter, **kw)
        return ops.boxqp_forward(g["P"], g["q"], g["l_min"], g["l_max"], EPS, max_iter, v=g.get("v"), **kw)
    if kind == "qp":
        return ops.qp_forward_warm(g["P"], g["q"], x0, EPS, max_iter, **kw)
    if kind == "qcqp":
        return ops.qcqp_forward_warm(g["P"], g["q"], g["l_n"], g["mu"], x0, EPS, max_iter, **kw)
    return ops.boxqp_forward_warm(g["P"], g["q"], g["l_min"], g["l_max"], x0, EPS, max_iter, v=g.get("v"), **kw)


def _tiled(base, B):
    """The base batch repeated to B problems (problem b is problem b mod base)."""
    reps = -(-B // base["q"].shape[0])
    return {k: v.repeat((reps,) + (1,) * (v.dim() - 1))[:B].contiguous() for k, v in base.items()}


def _min_match(N, route):
    return 0.999 if N <= 16 else 0.99


def _check(xh, ith, xr, itr, min_match, what):
    xh, ith = npy(xh), npy(ith)
    scale = np.maximum(1.0, np.abs(xr).max(axis=(1, 2), keepdims=True))
    err = (np.abs(xh - xr) / scale).max()
    match = (ith == itr).mean()
    print("%s: max |dx| / scale %.3g, equal iteration counts on %.4f" % (what, err, match))
    assert np.isfinite(xh).all(), what
    assert err <= 1e-6, "%s: |x - reference| / scale = %g" % (what, err)
    assert match >= min_match, "%s: iteration counts differ on %.3f%% of the problems" % (what, 100 * (1 - match))


@pytest.mark.parametrize("row", FWD, ids=row_id)
def test_warm_forward_against_the_restatement(ops, row):
    _, kind, N, B, layout, _, route = row
    base, full, cold, ref = reference(row)
    g = _dev(full, layout)
    xc, itc = _fwd(ops, kind, g, layout)
    for name in VARIANTS:
        x0, xr, itr = ref[name]
        x0d = torch.from_numpy(tile(x0, B)).cuda()
        xh, ith = _fwd(ops, kind, g, layout, x0d)
        _check(xh, ith, tile(xr, B), tile(itr, B), _min_match(N, route), "%s x0 = %s" % (row_id(row), name))
        if name == "perturbed":
            warm_total, cold_total = int(npy(ith).astype(np.int64).sum()), int(npy(itc).astype(np.int64).sum())
            print("%s: device iterations cold %d, warm %d (%.3f)" % (row_id(row), cold_total, warm_total, warm_total / cold_total))
            assert warm_total < cold_total
            # the batch slice t[1:] of every argument (8-byte aligned for odd N, a multiple of 16 otherwise)
            gs = {k: v[1:] for k, v in g.items()}
            xs, its = _fwd(ops, kind, gs, layout, x0d[1:])
            _check(xs, its, tile(xr, B)[1:], tile(itr, B)[1:], _min_match(N, route), "%s t[1:]" % row_id(row))
    # max_iter = 0: x0 comes back bit for bit, no iteration is counted
    x0d = torch.from_numpy(tile(ref["infeasible"][0], B)).cuda()
    xh, ith = _fwd(ops, kind, g, layout, x0d, max_iter=0)
    assert torch.equal(xh.view(torch.int64), x0d.view(torch.int64)) and not bool(ith.any())
    # a NaN start in two problems (a diagonal and, in the mixed batches, a general one): NaN there, the same bits elsewhere
    x0d = torch.from_numpy(tile(ref["perturbed"][0], B)).cuda()
    xa, ita = _fwd(ops, kind, g, layout, x0d, max_iter=50)
    poisoned = x0d.clone()
    hit = [b for b in (3, 4) if b < B]
    for b in hit:
        poisoned[b, b % N, 0] = float("nan")
    xb, itb = _fwd(ops, kind, g, layout, poisoned, max_iter=50)
    torch.cuda.synchronize()
    keep = torch.ones(B, dtype=torch.bool, device="cuda")
    keep[hit] = False
    assert torch.equal(xa[keep].view(torch.int64), xb[keep].view(torch.int64)) and torch.equal(ita[keep], itb[keep])
    assert bool(torch.isnan(xb[hit]).all())


@pytest.mark.parametrize("kind", ("qp", "qcqp", "box", "sbox"))
def test_same_bits_on_every_lane_layout(ops, kind):
    """N = 8: four, two and (DQQ_F_EXPECT_DENSE, QP / QCQP) one lane per problem, reached through B, all fused.  N = 4: two
    lanes fused against one lane with the general tiles drained by the lane kernel -- there the problems of diagonal tiles."""
    row = next(r for r in FWD if r[1] == kind and r[2] == 8 and r[3] == 2051 and r[4] == 0)
    base, _, _, ref = reference(row)
    nb = base["q"].shape[0]
    runs = [(2051, 0), (57344, 0)] + ([(57344, XD)] if kind in ("qp", "qcqp") else [])
    out = []
    for B, flags in runs:
        g = _dev(_tiled(base, B), 0)
        x0 = torch.from_numpy(tile(ref["perturbed"][0], B)).cuda()
        x, it = _fwd(ops, kind, g, flags, x0)
        out.append((x[:nb].clone(), it[:nb].clone()))
    for x, it in out[1:]:
        assert torch.equal(x.view(torch.int64), out[0][0].view(torch.int64)) and torch.equal(it, out[0][1])
    # N = 4.  The work-list form queues WHOLE tiles (a tile with one general problem goes to the lane kernel, its diagonal
    # problems with it -- as in the cold forward), so the batch keeps its general problems in the first 128 and is diagonal
    # from there on: those tiles stay on the diagonal arithmetic in both forms, while the drain still has tiles 0 and 1 to solve.
    row4 = next(r for r in FWD if r[1] == kind and r[2] == 4)
    base, _, _, ref = reference(row4)
    out = []
    for B in (600, 131073):
        full = _tiled(base, B)
        full["P"][128:] = torch.diag_embed(torch.diagonal(full["P"][128:], dim1=1, dim2=2))
        g = _dev(full, 0)
        x0 = torch.from_numpy(tile(ref["perturbed"][0], B)).cuda()
        x, it = _fwd(ops, kind, g, 0, x0)
        out.append((x[128:600].clone(), it[128:600].clone()))
    assert torch.equal(out[0][0].view(torch.int64), out[1][0].view(torch.int64)) and torch.equal(out[0][1], out[1][1])


def test_graph_capture_replays_bit_equal(ops):
    """The warm forward and the backward of its x, captured on a side stream (warmed up first: tests/test_gpu_graph_capture.py)
    into preallocated outputs; the replay must give the eager run's bits."""
    row = next(r for r in FWD if r[1] == "qp" and r[2] == 8 and r[3] == 2051 and r[4] == 0)
    _, full, _, ref = reference(row)
    B = row[3]
    g = _dev(full, 0)
    x0 = torch.from_numpy(tile(ref["perturbed"][0], B)).cuda()
    x = torch.empty(B, 8, 1, dtype=torch.float64, device="cuda")
    gP, gq = torch.empty(B, 8, 8, dtype=torch.float64, device="cuda"), torch.empty(B, 8, 1, dtype=torch.float64, device="cuda")

    def step():
        ops.qp_forward_warm(g["P"], g["q"], x0, EPS, MAX_ITER, out=x)
        ops.qp_backward(g["P"], g["q"], x, g["grad_x"], out=(gP, gq))
    step()
    torch.cuda.synchronize()
    eager = [t.clone() for t in (x, gP, gq)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()   # warms the capture stream's workspace up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    for t in (x, gP, gq):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, (x, gP, gq)):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_autograd_is_the_base_class_backward(ops):
    from diffqcqp_amd import qcqp
    cases = (("qp", qcqp.QPWarmFn2, ops.qp_backward), ("qcqp", qcqp.QCQPWarmFn2, ops.qcqp_backward),
             ("box", qcqp.BoxQPWarmFn2, ops.boxqp_backward), ("sbox", qcqp.SignedBoxQPWarmFn2, ops.boxqp_backward))
    for kind, fn, bwd in cases:
        row = next(r for r in FWD if r[1] == kind and r[2] == 8 and r[3] == 2051 and r[4] == 0)
        _, full, _, ref = reference(row)
        g = _dev(full, 0)
        x0 = torch.from_numpy(tile(ref["perturbed"][0], row[3])).cuda().requires_grad_(True)
        names = ("P", "q") + EXTRAS[kind]
        ins = [g[n].clone().requires_grad_(n != "v") for n in names]
        x = fn.apply(*ins, x0, EPS, MAX_ITER)
        xw = _fwd(ops, kind, g, 0, x0.detach())[0]
        assert torch.equal(x.detach().view(torch.int64), xw.view(torch.int64))
        x.backward(torch.ones_like(x))
        assert x0.grad is None                                     # warm_start gets no gradient
        aux = [g[n] for n in EXTRAS[kind][:2]]
        kw = {"v": g["v"]} if kind == "sbox" else {}
        want = bwd(g["P"], g["q"], *aux, x.detach(), torch.ones_like(x), **kw)
        for t, w in zip(ins, want):
            assert torch.equal(t.grad.view(torch.int64), w.view(torch.int64))


@pytest.mark.parametrize("kind,N,B,layout", [("qp", 8, 65, 0), ("qcqp", 8, 129, 2), ("box", 6, 63, 0), ("sbox", 12, 33, 0),
                                             ("qp", 24, 17, 0), ("qcqp", 18, 9, 0x100), ("qp", 70, 3, 0)])
@pytest.mark.parametrize("sliced", (True, False))
def test_x0_is_read_only_and_exactly_sized(kind, N, B, layout, sliced):
    """Every buffer of the call in the guarded arena (tests/footprint_arena.py), x0 an input of exactly (B,N,1) doubles between
    poisoned guards: a read past it brings NaN into x, a write to it or around it is seen."""
    from conftest import make_problem
    from diffqcqp_amd import build, _capi
    from warm_cases import well_conditioned
    build.build()
    lib = _capi.lib()
    d = make_problem(kind, B, N, 555 + N, "mixed" if N <= 16 else "dense")
    d["P"] = well_conditioned(d["P"])
    if layout == 2:
        d["P"] = torch.diag_embed(torch.diagonal(d["P"], dim1=1, dim2=2))
    x0 = 0.5 * torch.randn(B, N, 1, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    dd = dict(d, P=torch.diagonal(d["P"], dim1=1, dim2=2).contiguous()) if layout == 2 else d
    worklist = lib.dqq_workspace_bytes(B)
    scratch = lib.dqq_scratch_bytes(KIND[kind], 0, N, B, layout)
    piece = lib.dqq_scratch_bytes(KIND[kind], 0, N, 1, layout) if scratch else 0
    specs = call_specs(0, kind, N, B, layout, dd, worklist + scratch, worklist, piece)
    specs.insert(len(specs) - 1, ("x0", "in", torch.float64, (B, N, 1), x0))
    a = Arena(specs, 256, "cuda", sliced=sliced)
    p = a.ptr
    ex = [p(n) for n in EXTRAS[kind]] + [None] * (3 - len(EXTRAS[kind]))
    rc = lib.dqq_fwd_warm_f64(KIND[kind], p("P"), p("q"), ex[0], ex[1], ex[2], p("x0"), p("x"), B, N, EPS, 1e-7, MAX_ITER, 1,
                              layout, p("iters"), p("pdiag_out"), p("diag_flags_out"), p("ws"), a.bufs["ws"]["nbytes"],
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    a.check_guards()
    a.check_inputs()
    for name in ("x", "iters", "diag_flags_out"):
        a.check_written(name)
    assert bool(torch.isfinite(a.view("x")).all()) and bool((a.view("iters") < MAX_ITER).all())
