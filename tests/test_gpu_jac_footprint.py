"""The memory footprint of dqq_newton_jac_f64 (-m gpu): guarded-arena cases per kernel family, ragged, one-problem and empty, with
the arena of tests/footprint_arena.py -- every buffer of the call carved out of one poisoned allocation, each payload one problem
past a 512-byte boundary (a batch slice that starts at an odd problem).  No byte outside a payload changes, no input changes,
every output is written for every problem and equals the host core's bits, an output that is not requested stays untouched, and
the scratch NewtonJacAny is given is exactly dqq_newton_jac_scratch_bytes."""
import numpy as np
import pytest
import torch

import jac_cases as C
import polish_cases as PC
import polish_reference as R
from footprint_arena import F64, I32, U8, Arena
from test_gpu_footprint import _tiled, capi   # noqa: F401  (capi: the fixture)

pytestmark = pytest.mark.gpu
AUTO, DENSE, DIAG = 0, 1, 2
# (family, kind, N, B, layout, structure, problems per workgroup, at most): NewtonJacDiag 4 waves of 128/N problems; NewtonJacTeam
# up to 4 waves of 64/T teams (N = 20: T = 32; fewer waves where the slices fill 64 KiB); NewtonJacAny a problem per workgroup
CASES = [("diag", "qcqp", 8, 67, DIAG, "diag", 64), ("diag", "sbox", 64, 5, DIAG, "diag", 8), ("diag", "qp", 2, 259, DIAG, "diag", 256),
         ("team", "box", 20, 37, DENSE, "dense", 8), ("team", "qp", 3, 37, AUTO, "dense", 32),
         ("team", "qcqp", 8, 37, DENSE, "dense", 32), ("team", "sbox", 64, 3, DENSE, "dense", 1),
         ("any", "qcqp", 66, 5, DENSE, "dense", 1), ("any", "sbox", 66, 5, DENSE, "dense", 1)]
OUTS = ("Jq", "Ja", "Jb")


def _specs(kind, N, B, layout, d, ws_bytes, slice_bytes, need=(True, True, True)):
    pshape = (B, N) if layout == DIAG else (B, N, N)
    eshape = (B, N // 2, 1) if kind == "qcqp" else (B, N, 1)
    specs = [("P", "in", F64, pshape, d["P"]), ("q", "in", F64, (B, N, 1), d["q"])]
    specs += [(n, "in", F64, eshape, d[n]) for n in PC.EXTRAS[kind]]
    specs += [("x", "in", F64, (B, N, 1), d["x"])]
    shapes = C.out_shapes(kind, B, N, layout == DIAG)
    specs += [(n, "out", F64, s, None) for n, s, nd in zip(OUTS, shapes, need) if s is not None and nd]
    specs += [("status", "out", I32, (B,), None)]
    return specs + [("ws", "ws", U8, (ws_bytes, 0), slice_bytes)]


def _call(capi, kind, N, B, layout, d, g, need=(True, True, True), short=0):   # noqa: F811
    lib = capi.lib()
    k = R.KIND[kind]
    ws_need = lib.dqq_newton_jac_scratch_bytes(k, N, B) if layout != DIAG else 0
    piece = lib.dqq_newton_jac_scratch_bytes(k, N, 1) if ws_need else 0
    a = Arena(_specs(kind, N, B, layout, d, ws_need, piece, need), g, "cuda", sliced=True)
    p = a.ptr
    opt = lambda n: p(n) if n in a.bufs else None   # noqa: E731
    ex = [p(n) for n in PC.EXTRAS[kind]] + [None] * (3 - len(PC.EXTRAS[kind]))
    try:
        rc = lib.dqq_newton_jac_f64(k, p("P"), p("q"), *ex, p("x"), opt("Jq"), opt("Ja"), opt("Jb"), B, N, layout, p("status"),
                                    p("ws") if ws_need else None, ws_need - short, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    except RuntimeError as e:   # a device fault: nothing more is started on this GPU
        pytest.exit("newton jac footprint %s N=%d: %s" % (kind, N, e), returncode=3)
    return a, rc, ws_need


def _inputs(kind, N, B, layout, structure):
    """-> (d: CPU tensors of every input, the host core's outputs by buffer name)"""
    from diffqcqp_amd import ops
    dn, x0 = PC.problem(kind, N, B, structure)
    P, q, ex = PC.flat(dn, kind)
    cu = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()   # noqa: E731
    x = ops._polish(R.KIND[kind], cu(P), cu(q[:, :, None]), [cu(e[:, :, None]) for e in ex], cu(x0), PC.MAX_STEPS, DENSE).cpu().numpy()
    diag = layout == DIAG
    Pa = PC.compact(P) if diag else P
    t = lambda a: torch.from_numpy(np.array(a, order="C"))   # noqa: E731
    d = {k: t(v) for k, v in dn.items()}
    d.update(P=t(Pa), x=t(x))
    h = C.host_jac(kind, Pa, q, ex, x[:, :, 0], diag=diag)
    return d, {"Jq": h[0], "Ja": h[1], "Jb": h[2], "status": h[3]}


def _same(a, ref, names, rows=slice(None)):
    for n in names:
        if ref[n] is None:
            assert n not in a.bufs
            continue
        got = a.view(n).cpu().numpy()
        assert C.same_bits(got.reshape(ref[n][rows].shape), ref[n][rows]), n


@pytest.mark.parametrize("family,kind,N,B,layout,structure,g", CASES, ids=lambda v: str(v))
def test_newton_jac_footprint(oracle, capi, family, kind, N, B, layout, structure, g):   # noqa: F811
    d, ref = _inputs(kind, N, B, layout, structure)
    need_any = capi.lib().dqq_newton_jac_scratch_bytes(R.KIND[kind], N, B)
    assert (need_any > 0) == (family == "any")
    a, rc, ws_need = _call(capi, kind, N, B, layout, d, g)
    assert rc == 0 and ws_need == need_any
    a.check_guards()
    a.check_inputs()
    names = tuple(n for n in OUTS + ("status",) if n in a.bufs)
    for name in names:
        a.check_written(name)
    _same(a, ref, OUTS + ("status",))
    assert not ref["status"].any()
    if kind != "qp":   # one output alone: the others' pointers are NULL, nothing but that output and the status is written
        a1, rc, _ = _call(capi, kind, N, B, layout, d, g, need=(False, True, False))
        assert rc == 0 and "Jq" not in a1.bufs and "Jb" not in a1.bufs
        a1.check_guards()
        a1.check_inputs()
        a1.check_written("Ja")
        _same(a1, ref, ("Ja", "status"))
    if ws_need:   # one byte less of scratch is refused, and nothing is touched
        a2, rc, _ = _call(capi, kind, N, B, layout, d, g, short=1)
        assert rc == -5
        a2.check_untouched()
    # a batch that ends on one problem, and the empty batch: nothing outside, nothing at all
    one = _tiled(d, 1)
    a, rc, _ = _call(capi, kind, N, 1, layout, one, g)
    assert rc == 0
    a.check_guards()
    a.check_inputs()
    for name in names:
        a.check_written(name)
    _same(a, ref, OUTS + ("status",), slice(0, 1))
    empty = {k: v[:0] for k, v in d.items()}
    a, rc, _ = _call(capi, kind, N, 0, layout, empty, g)
    assert rc == 0
    a.check_untouched()
