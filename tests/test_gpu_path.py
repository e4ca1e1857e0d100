"""dqq_polish_path_f64 on the device (-m gpu): every kind on every route family, bit for bit on every output -- x_out, resid,
steps, status, halvings, stage_resid, stage_steps -- against (a) the plain host core (tests/hostcore/path_core_check.cpp, held
bit-equal to the numpy restatement on the CPU) and (b) the chain of dqq_polish_smooth_f64 launches on the device that the entry is
defined to be; then the properties of the entry: in place, a batch slice, a NaN and an Inf problem next to good ones, a single
stage against both parents, budgets of zero, reg > 0, the longest schedule, each optional output NULL in turn, a diagonal P given as
(B,N,N) against DQQ_P_DIAG, the Python fronts, and capture into a graph.  Shapes: the smallest that reach each code path -- a ragged
last tile on the compact diagonal; on (B,N,N) a team size that does not divide N, the LDS limit N = 64, and N = 66 on scratch.
Inputs: tests/path_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

import path_cases as PC
import polish_reference as R
import smooth_cases as SC

pytestmark = pytest.mark.gpu

AUTO, DENSE, DIAG = 0, PC.DENSE, PC.DIAG
H = 8
DEFAULT = (PC.KAPPAS, PC.STEPS)
NAMES = ("x_out", "resid", "steps", "status", "halvings", "stage_resid", "stage_steps")
ROWS = PC.ROWS


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()


def _ws(k, N, n):
    from diffqcqp_amd import ops
    ws = ops.polish_workspace(torch.device("cuda"), k, N, n)
    return (None, 0) if ws is None else (ws, ws.numel() * 4)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _inputs(kind, P, q, ex, x, layout, first):
    full = [dev(PC.compact(P) if (layout & 0xff) == DIAG else P), dev(q)] + [dev(e) for e in ex] + [dev(x)]
    t = [a[first:] for a in full]
    assert all(a.is_contiguous() for a in t)
    return t, [a.data_ptr() for a in t[2:-1]] + [None] * (3 - len(ex))


def path(kind, P, q, ex, x, layout, schedule=DEFAULT, h=H, reg=0.0, in_place=False, first=0, null=()):
    """dqq_polish_path_f64 itself on flat numpy arrays, the problems from `first` on as views into the full batch's memory.  null:
    the names of the optional outputs passed as NULL.  -> numpy, NAMES' order (None for a NULL output)"""
    from diffqcqp_amd import _capi
    lib = _capi.lib()
    B, N = x.shape
    k, S = R.KIND[kind], len(schedule[0])
    t, exp = _inputs(kind, P, q, ex, x, layout, first)
    n = B - first
    xo = t[-1] if in_place else torch.full((n, N), 7.0, dtype=torch.float64, device="cuda")
    f64 = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device="cuda")      # noqa: E731
    i32 = lambda *s: torch.full(s, -1, dtype=torch.int32, device="cuda")         # noqa: E731
    outs = [xo, f64(n, 2), i32(n), i32(n), i32(n), f64(n, S, 2), i32(n, S)]
    ptr = [None if name in null else o.data_ptr() for name, o in zip(NAMES, outs)]
    ks, ns = (ctypes.c_double * S)(*schedule[0]), (ctypes.c_int * S)(*schedule[1])
    ws, wb = _ws(k, N, n)
    rc = lib.dqq_polish_path_f64(k, t[0].data_ptr(), t[1].data_ptr(), *exp, t[-1].data_ptr(), ptr[0], n, N, layout, reg,
                                 ctypes.addressof(ks), ctypes.addressof(ns), S, h, *ptr[1:], None if ws is None else ws.data_ptr(), wb,
                                 _stream())
    assert rc == 0
    torch.cuda.synchronize()
    for name, o in zip(NAMES, outs):         # a NULL output's buffer is not reached by another pointer
        if name in null:
            assert (o == (7.0 if o.dtype is torch.float64 else -1)).all()
    return tuple(None if name in null else o.cpu().numpy() for name, o in zip(NAMES, outs))


def device_chain(kind, P, q, ex, x, layout, schedule=DEFAULT, h=H, reg=0.0, parent=False):
    """The chain the entry is defined to be: one dqq_polish_smooth_f64 launch per stage on the device, each from the last one's
    x_out (parent: dqq_polish_ls_f64 for the stages with kappa = 0).  -> numpy, NAMES' order"""
    from diffqcqp_amd import _capi
    lib = _capi.lib()
    B, N = x.shape
    k = R.KIND[kind]
    t, exp = _inputs(kind, P, q, ex, x, layout, 0)
    ws, wb = _ws(k, N, B)
    cur = t[-1]

    def call(cur_np, kappa, n):
        nonlocal cur
        xo = torch.full((B, N), 7.0, dtype=torch.float64, device="cuda")
        resid = torch.empty((B, 2), dtype=torch.float64, device="cuda")
        steps, status, halv = (torch.full((B,), -1, dtype=torch.int32, device="cuda") for _ in range(3))
        head = (k, t[0].data_ptr(), t[1].data_ptr(), *exp, cur.data_ptr(), xo.data_ptr(), B, N, n, layout, reg)
        tail = (h, resid.data_ptr(), steps.data_ptr(), status.data_ptr(), halv.data_ptr(), None if ws is None else ws.data_ptr(), wb, _stream())
        rc = lib.dqq_polish_ls_f64(*head, *tail) if (parent and kappa == 0.0) else lib.dqq_polish_smooth_f64(*head, kappa, *tail)
        assert rc == 0
        cur = xo
        torch.cuda.synchronize()
        return tuple(a.cpu().numpy() for a in (xo, resid, steps, status, halv))

    return PC.chain(call, x, *schedule)


def host(kind, P, q, ex, x, layout, schedule=DEFAULT, h=H, reg=0.0):
    diag = (layout & 0xff) == DIAG
    return PC.host_path(kind, PC.compact(P) if diag else P, q, ex, x, schedule[0], schedule[1], h, reg, diag=diag)


def assert_same(got, ref, what="", skip=()):
    for name, g, r in zip(NAMES, got, ref):
        if name in skip:
            continue
        assert g.dtype == r.dtype and g.shape == r.shape and PC.same_bits(g, r), "%s %s: %s vs %s" % (what, name, g.reshape(-1)[:4], r.reshape(-1)[:4])


@pytest.mark.parametrize("kind,N,layout,structure,B", ROWS)
def test_family_is_the_host_core_and_the_device_chain_bit_for_bit(kind, N, layout, structure, B):
    P, q, ex, x = PC.problem(kind, N, B, structure)
    ref = host(kind, P, q, ex, x, layout)
    what = "%s N=%d layout %d" % (kind, N, layout)
    print("%s: status 0 on %d of %d, steps up to %d over %s, worst r after %.2e" % (what, (ref[3] == 0).sum(), B, ref[2].max(),
                                                                                    ref[6].max(axis=0), ref[1][:, 1].max()))
    got = path(kind, P, q, ex, x, layout)
    assert_same(got, ref, what + " vs the host core")
    assert_same(got, device_chain(kind, P, q, ex, x, layout), what + " vs the device chain")
    assert (ref[3] == 0).sum() >= (B + 1) // 2
    # in place, and a batch slice from an odd problem
    assert_same(path(kind, P, q, ex, x, layout, in_place=True), ref, "in place")
    assert_same(path(kind, P, q, ex, x, layout, first=3), tuple(r[3:] for r in ref), "a slice from an odd problem")
    # a schedule that is not monotone, with a stage without budget and the hard stage in the middle; reg > 0 and one halving
    assert_same(path(kind, P, q, ex, x, layout, PC.SHORT, 1, 1e-3), host(kind, P, q, ex, x, layout, PC.SHORT, 1, 1e-3), "reg")
    assert_same(path(kind, P, q, ex, x, layout, PC.SHORT, 1, 1e-3), device_chain(kind, P, q, ex, x, layout, PC.SHORT, 1, 1e-3), "reg, chain")
    # the longest schedule
    assert_same(path(kind, P, q, ex, x, layout, PC.LONG), host(kind, P, q, ex, x, layout, PC.LONG), "eight stages")
    # one stage: both parents' bits
    for one in (((1e-2,), (6,)), ((0.0,), (6,))):
        single = path(kind, P, q, ex, x, layout, one)
        assert_same(single, device_chain(kind, P, q, ex, x, layout, one, parent=True), "one stage against its parent")
        assert PC.same_bits(single[5][:, 0], single[1]) and PC.same_bits(single[6][:, 0], single[2])
    # budgets of zero: x is copied, every stage records its r before twice
    zero = path(kind, P, q, ex, x, layout, (PC.SHORT[0], (0,) * 4))
    assert_same(zero, host(kind, P, q, ex, x, layout, (PC.SHORT[0], (0,) * 4)), "no budget")
    assert PC.same_bits(zero[0], x) and not zero[2].any() and not zero[4].any() and not zero[6].any() and (zero[3] == 1).all()
    assert PC.same_bits(zero[5][:, :, 0], zero[5][:, :, 1])
    # a NaN problem and an Inf problem next to good ones: status 2, x kept, no other row changes
    P2, x2 = np.array(P), np.array(x)
    m1, m2 = B // 2, B // 2 + 1
    x2[m1, N - 1] = np.nan
    P2[m2, 1, 1] = np.inf
    bad = path(kind, P2, q, ex, x2, layout, PC.SHORT)
    assert_same(bad, host(kind, P2, q, ex, x2, layout, PC.SHORT), "with bad rows")
    assert_same(bad, device_chain(kind, P2, q, ex, x2, layout, PC.SHORT), "with bad rows, chain")
    keep = np.ones(B, dtype=bool)
    keep[[m1, m2]] = False
    good = path(kind, P, q, ex, x, layout, PC.SHORT)
    assert list(bad[3][[m1, m2]]) == [2, 2] and PC.same_bits(bad[0][[m1, m2]], x2[[m1, m2]]) and not bad[2][[m1, m2]].any()
    for g, b in zip(good, bad):
        assert PC.same_bits(g[keep], b[keep])
    # each optional output NULL in turn: the others' bits do not change
    for name in NAMES[1:]:
        assert_same(path(kind, P, q, ex, x, layout, PC.SHORT, null=(name,)), good, "without " + name, skip=(name,))
    assert_same(path(kind, P, q, ex, x, layout, PC.SHORT, null=NAMES[1:]), good, "x_out alone", skip=NAMES[1:])


@pytest.mark.parametrize("kind", PC.KINDS)
@pytest.mark.parametrize("N", PC.DIAG_MATRIX_N)
def test_a_diagonal_P_given_dense_gives_the_compact_routes_bits(kind, N):
    P, q, ex, x = PC.problem(kind, N, PC.diag_bs(N)[1], "diag")
    for schedule in (DEFAULT, PC.SHORT):
        assert_same(path(kind, P, q, ex, x, DENSE, schedule), path(kind, P, q, ex, x, DIAG, schedule), "%s N=%d" % (kind, N))


def _t(a, tail=1):
    return None if a is None else dev(a).reshape(a.shape + (1,) * tail)


@pytest.mark.parametrize("kind,structure", SC.ROWS)
def test_ops_and_the_cold_start_solver_on_the_frozen_rows(kind, structure):
    """The public ops give the entry's bits, and diagnostics.solve_*_newton -- cold start, path, check: no ADMM -- ends converged on
    every problem of every frozen row."""
    from diffqcqp_amd import diagnostics as D, ops
    P, q, ex, x, _, _ = SC.frozen(kind, structure)
    ref = host(kind, P, q, ex, x, DENSE)
    assert (ref[1][:, 1] <= SC.CONVERGED).all()
    Pt, qt, ext, xt = dev(P), _t(q), [_t(e) for e in ex], _t(x)
    op = {"qp": ops.qp_polish_path, "qcqp": ops.qcqp_polish_path, "box": ops.boxqp_polish_path, "sbox": ops.boxqp_polish_path}[kind]
    kw = dict(v=ext[2]) if kind == "sbox" else {}
    out = op(Pt, qt, *ext[:2], xt, return_info=True, **kw)
    assert_same(tuple(o.cpu().numpy().reshape(r.shape) for o, r in zip(out, ref)), ref, "ops")
    assert PC.same_bits(op(Pt, qt, *ext[:2], xt, **kw).cpu().numpy().reshape(x.shape), ref[0])
    short = op(Pt, qt, *ext[:2], xt, kappas=PC.SHORT[0], stage_steps=PC.SHORT[1], max_halvings=1, reg=1e-3, return_info=True, **kw)
    href = host(kind, P, q, ex, x, DENSE, PC.SHORT, 1, 1e-3)
    assert_same(tuple(o.cpu().numpy().reshape(r.shape) for o, r in zip(short, href)), href, "ops, another schedule")
    # scaling="pow2" composes as the polish's does: equilibrate, the path on the scaled problem, unscale
    scaled = op(Pt, qt, *ext[:2], xt, return_info=True, scaling="pow2", **kw)
    k = R.KIND[kind]
    Ps, qs, exs, x0s, e = ops.equilibrate(k, Pt, qt, ext, xt, AUTO)
    by_hand = ops._polish_path(k, Ps, qs, exs, x0s, return_info=True)
    assert torch.equal(scaled[0], ops.unscale(by_hand[0], e)) and all(torch.equal(a, b) for a, b in zip(scaled[1:], by_hand[1:]))
    if structure == "diag":
        got = op(dev(PC.compact(P)), qt, *ext[:2], xt, layout=DIAG, return_info=True, **kw)
        assert_same(tuple(o.cpu().numpy().reshape(r.shape) for o, r in zip(got, ref)), ref, "ops, compact diagonal")
    solve = {"qp": D.solve_qp_newton, "qcqp": D.solve_qcqp_newton, "box": D.solve_boxqp_newton, "sbox": D.solve_signedboxqp_newton}[kind]
    xs, info, pinfo = solve(Pt, qt, *ext, layout="dense")
    assert PC.same_bits(xs.cpu().numpy().reshape(x.shape), ref[0])           # the cold start made by torch ops is the frozen one
    assert (info.status == 0).all() and int(info.counts[0]) == SC.B and (pinfo.status == 0).all()
    assert PC.same_bits(pinfo.after.cpu().numpy(), ref[1][:, 1]) and (pinfo.after <= SC.CONVERGED).all()
    assert PC.same_bits(pinfo.stage_steps.cpu().numpy(), ref[6]) and PC.same_bits(pinfo.steps.cpu().numpy(), ref[2])
    print("%s %s: natural residual of the check up to %.2e" % (kind, structure, float(info.natural.max())))


@pytest.mark.parametrize("kind,N,layout,structure,B", [("qcqp", 8, DIAG, "diag", 70), ("sbox", 20, DENSE, "dense", 37), ("qp", 66, DENSE, "dense", 5)])
def test_capture_and_two_replays_give_the_eager_bits(kind, N, layout, structure, B):
    """The schedule travels in the launch: the host arrays are gone when the graph replays."""
    from diffqcqp_amd import ops
    P, q, ex, x = PC.problem(kind, N, B, structure)
    Pt, qt, ext, xt = dev(PC.compact(P) if layout == DIAG else P), _t(q), [_t(e) for e in ex], _t(x)
    k = R.KIND[kind]
    call = lambda out, info=True: ops._polish_path(k, Pt, qt, ext, xt, PC.SHORT[0], PC.SHORT[1], 2, 1e-3, layout, out=out,   # noqa: E731
                                                   return_info=info, workspace=ws)
    ws = ops.polish_workspace(torch.device("cuda"), k, N, B)
    eager = call(torch.empty_like(xt))
    torch.cuda.synchronize()
    out = torch.empty_like(xt)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call(torch.empty_like(xt), False)      # warm the stream up
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = call(out)
    for _ in range(2):
        for r in res:
            r.fill_(-3)
        g.replay()
        torch.cuda.synchronize()
        for r, e in zip(res, eager):
            assert PC.same_bits(r.cpu().numpy(), e.cpu().numpy())
    assert_same(tuple(r.cpu().numpy().reshape(h.shape) for r, h in zip(res, host(kind, P, q, ex, x, layout, PC.SHORT, 2, 1e-3))),
                host(kind, P, q, ex, x, layout, PC.SHORT, 2, 1e-3), "replay vs the host core")
