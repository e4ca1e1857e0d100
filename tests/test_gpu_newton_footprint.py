"""The memory footprint of dqq_newton_bwd_f64 / dqq_newton_jvp_f64 (-m gpu): one guarded-arena case per kernel family and mode,
ragged, one-problem and empty, with the arena of tests/footprint_arena.py -- every buffer of the call carved out of one poisoned
allocation, each payload one problem past a 512-byte boundary (a batch slice that starts at an odd problem).  No byte outside a
payload changes, no input changes, every output is written for every problem and equals the host core's bits, and the scratch
NewtonAny is given is exactly dqq_newton_scratch_bytes."""
import numpy as np
import pytest
import torch

import newton_cases as C
import polish_cases as PC
import polish_reference as R
from footprint_arena import F64, I32, U8, Arena
from test_gpu_footprint import _tiled, capi   # noqa: F401  (capi: the fixture)

pytestmark = pytest.mark.gpu
AUTO, DENSE, DIAG = 0, 1, 2
# (family, kind, N, B, layout, structure, problems per workgroup): NewtonDiag 4 waves of 128/N problems; NewtonTeam 4 waves of
# 64/T teams (N = 20: T = 32); NewtonAny a problem per workgroup
CASES = [("diag", "qcqp", 8, 67, DIAG, "diag", 64), ("diag", "sbox", 64, 5, DIAG, "diag", 8),
         ("team", "box", 20, 37, DENSE, "dense", 8), ("team", "qp", 3, 37, AUTO, "dense", 32),
         ("team", "qcqp", 8, 37, DENSE, "dense", 32), ("any", "qcqp", 66, 5, DENSE, "dense", 1),
         ("any", "sbox", 66, 5, DENSE, "dense", 1)]
OUTS = {"bwd": ("grad_P", "grad_q", "grad_a", "grad_b"), "jvp": ("dx",)}


def _specs(mode, kind, N, B, layout, d, ws_bytes, slice_bytes):
    pshape = (B, N) if layout == DIAG else (B, N, N)
    eshape = (B, N // 2, 1) if kind == "qcqp" else (B, N, 1)
    specs = [("P", "in", F64, pshape, d["P"]), ("q", "in", F64, (B, N, 1), d["q"])]
    specs += [(n, "in", F64, eshape, d[n]) for n in PC.EXTRAS[kind]]
    specs += [("x", "in", F64, (B, N, 1), d["x"])]
    if mode == "bwd":
        specs += [("grad_x", "in", F64, (B, N, 1), d["grad_x"]), ("grad_P", "out", F64, pshape, None),
                  ("grad_q", "out", F64, (B, N, 1), None)]
        if kind != "qp":
            specs += [("grad_a", "out", F64, eshape, None), ("grad_b", "out", F64, eshape, None)]
    else:
        specs += [("dP", "in", F64, pshape, d["dP"]), ("dq", "in", F64, (B, N, 1), d["dq"])]
        if kind != "qp":
            specs += [("da", "in", F64, eshape, d["da"]), ("db", "in", F64, eshape, d["db"])]
        specs += [("dx", "out", F64, (B, N, 1), None)]
    specs += [("status", "out", I32, (B,), None)]
    return specs + [("ws", "ws", U8, (ws_bytes, 0), slice_bytes)]


def _call(capi, mode, kind, N, B, layout, d, g):   # noqa: F811
    lib = capi.lib()
    k = R.KIND[kind]
    need = lib.dqq_newton_scratch_bytes(k, N, B) if layout != DIAG else 0
    piece = lib.dqq_newton_scratch_bytes(k, N, 1) if need else 0
    a = Arena(_specs(mode, kind, N, B, layout, d, need, piece), g, "cuda", sliced=True)
    p = a.ptr
    opt = lambda n: p(n) if n in a.bufs else None   # noqa: E731
    ex = [p(n) for n in PC.EXTRAS[kind]] + [None] * (3 - len(PC.EXTRAS[kind]))
    tail = (B, N, layout, p("status"), p("ws") if need else None, need, torch.cuda.current_stream().cuda_stream)
    try:
        if mode == "bwd":
            rc = lib.dqq_newton_bwd_f64(k, p("P"), p("q"), *ex, p("x"), p("grad_x"), p("grad_P"), p("grad_q"), opt("grad_a"),
                                        opt("grad_b"), *tail)
        else:
            rc = lib.dqq_newton_jvp_f64(k, p("P"), p("q"), *ex, p("x"), p("dP"), p("dq"), opt("da"), opt("db"), p("dx"), *tail)
        torch.cuda.synchronize()
    except RuntimeError as e:   # a device fault: nothing more is started on this GPU
        pytest.exit("newton footprint %s %s N=%d: %s" % (mode, kind, N, e), returncode=3)
    return a, rc, need


def _inputs(kind, N, B, layout, structure):
    """-> (d: CPU tensors of every input of both modes, the host core's outputs by buffer name)"""
    from diffqcqp_amd import ops
    dn, x0 = PC.problem(kind, N, B, structure)
    P, q, ex = PC.flat(dn, kind)
    cu = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()   # noqa: E731
    x = ops._polish(R.KIND[kind], cu(P), cu(q[:, :, None]), [cu(e[:, :, None]) for e in ex], cu(x0), PC.MAX_STEPS, DENSE).cpu().numpy()
    tan, g = C.inputs(kind, N, B, structure)
    diag = layout == DIAG
    Pa = PC.compact(P) if diag else P
    ta = ((PC.compact(tan[0]) if diag else tan[0]),) + tan[1:]
    t = lambda a: torch.from_numpy(np.array(a, order="C"))   # noqa: E731
    d = {k: t(v) for k, v in dn.items()}
    d.update(P=t(Pa), x=t(x), grad_x=t(g[:, :, None]), dP=t(ta[0]), dq=t(ta[1][:, :, None]))
    if kind != "qp":
        d.update(da=t(ta[2][:, :, None]), db=t(ta[3][:, :, None]))
    hj = C.host_jvp(kind, Pa, q, ex, x[:, :, 0], ta, diag=diag)
    hb = C.host_backward(kind, Pa, q, ex, x[:, :, 0], g, diag=diag)
    ref = {"jvp": {"dx": hj[0], "status": hj[1]},
           "bwd": {"grad_P": hb[0], "grad_q": hb[1], "grad_a": hb[2], "grad_b": hb[3], "status": hb[4]}}
    return d, ref


def _same(a, ref, names, rows=slice(None)):
    for n in names:
        if ref[n] is None:
            assert n not in a.bufs
            continue
        got = a.view(n).cpu().numpy()
        assert C.same_bits(got.reshape(ref[n][rows].shape), ref[n][rows]), n


@pytest.mark.parametrize("mode", ["bwd", "jvp"])
@pytest.mark.parametrize("family,kind,N,B,layout,structure,g", CASES, ids=lambda v: str(v))
def test_newton_footprint(oracle, capi, mode, family, kind, N, B, layout, structure, g):   # noqa: F811
    d, ref = _inputs(kind, N, B, layout, structure)
    need_any = capi.lib().dqq_newton_scratch_bytes(R.KIND[kind], N, B)
    assert (need_any > 0) == (family == "any")
    a, rc, need = _call(capi, mode, kind, N, B, layout, d, g)
    assert rc == 0 and need == need_any
    a.check_guards()
    a.check_inputs()
    names = tuple(n for n in OUTS[mode] + ("status",) if n in a.bufs)
    for name in names:
        a.check_written(name)
    _same(a, ref[mode], OUTS[mode] + ("status",))
    assert not ref[mode]["status"].any()
    if need:   # one byte less of scratch is refused, and nothing is touched
        lib, p = capi.lib(), a.ptr
        a2 = Arena(_specs(mode, kind, N, B, layout, d, need, need // min(B, 512)), g, "cuda", sliced=True)
        p = a2.ptr
        ex = [p(n) for n in PC.EXTRAS[kind]] + [None] * (3 - len(PC.EXTRAS[kind]))
        if mode == "bwd":
            rc = lib.dqq_newton_bwd_f64(R.KIND[kind], p("P"), p("q"), *ex, p("x"), p("grad_x"), p("grad_P"), p("grad_q"), None, None,
                                        B, N, layout, None, p("ws"), need - 1, None)
        else:
            rc = lib.dqq_newton_jvp_f64(R.KIND[kind], p("P"), p("q"), *ex, p("x"), None, p("dq"), None, None, p("dx"), B, N, layout,
                                        None, p("ws"), need - 1, None)
        torch.cuda.synchronize()
        assert rc == -5
        a2.check_untouched()
    # a batch that ends on one problem, and the empty batch: nothing outside, nothing at all
    one = _tiled(d, 1)
    a, rc, _ = _call(capi, mode, kind, N, 1, layout, one, g)
    assert rc == 0
    a.check_guards()
    a.check_inputs()
    for name in names:
        a.check_written(name)
    _same(a, ref[mode], OUTS[mode] + ("status",), slice(0, 1))
    empty = {k: v[:0] for k, v in d.items()}
    a, rc, _ = _call(capi, mode, kind, N, 0, layout, empty, g)
    assert rc == 0
    a.check_untouched()
