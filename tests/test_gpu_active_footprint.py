"""The memory footprint of dqq_newton_active_f64 (-m gpu): guarded-arena cases per kernel family, ragged, one-problem and empty,
with the arena of tests/footprint_arena.py -- every buffer of the call carved out of one poisoned allocation, each payload one
problem past a 512-byte boundary (a batch slice that starts at an odd problem).  No byte outside a payload changes, no input
changes, every output is written for every problem and equals the host core's bits, and an output that is not requested stays
untouched.  The entry has no workspace: the arena holds none."""
import numpy as np
import pytest
import torch

import active_cases as C
import polish_cases as PC
import polish_reference as R
from footprint_arena import F64, I32, Arena
from test_gpu_footprint import _tiled, capi   # noqa: F401  (capi: the fixture)

pytestmark = pytest.mark.gpu
AUTO, DENSE, DIAG = 0, 1, 2
# (family, kind, N, B, layout, structure, problems per workgroup, at most): ActiveDiag 4 waves of 128/N problems; ActiveTeam up to
# 4 waves of 64/T teams (N = 20: T = 32; N = 64: one wave, the slice fills half of 64 KiB); ActiveAny a problem per workgroup
CASES = [("diag", "qcqp", 8, 67, DIAG, "diag", 64), ("diag", "sbox", 64, 5, DIAG, "diag", 8), ("diag", "qp", 2, 259, DIAG, "diag", 256),
         ("team", "box", 20, 37, DENSE, "dense", 8), ("team", "qp", 3, 37, AUTO, "dense", 32),
         ("team", "qcqp", 8, 37, DENSE, "dense", 32), ("team", "sbox", 64, 3, DENSE, "dense", 1),
         ("any", "qcqp", 66, 5, DENSE, "dense", 1), ("any", "sbox", 258, 3, DENSE, "dense", 1)]
OUTS = C.NAMES
DTYPE = {"state": I32, "mult": F64, "margin": F64, "where": I32, "status": I32}


def _specs(kind, N, B, layout, d, need):
    pshape = (B, N) if layout == DIAG else (B, N, N)
    eshape = (B, N // 2, 1) if kind == "qcqp" else (B, N, 1)
    ne = C.elements(kind, N)
    shapes = {"state": (B, ne), "mult": (B, ne), "margin": (B,), "where": (B,), "status": (B,)}
    specs = [("P", "in", F64, pshape, d["P"]), ("q", "in", F64, (B, N, 1), d["q"])]
    specs += [(n, "in", F64, eshape, d[n]) for n in PC.EXTRAS[kind]]
    specs += [("x", "in", F64, (B, N, 1), d["x"])]
    return specs + [(n, "out", DTYPE[n], shapes[n], None) for n, nd in zip(OUTS, need) if nd]


def _call(capi, kind, N, B, layout, d, g, need=(True,) * 5):   # noqa: F811
    lib = capi.lib()
    a = Arena(_specs(kind, N, B, layout, d, need), g, "cuda", sliced=True)
    p = a.ptr
    opt = lambda n: p(n) if n in a.bufs else None   # noqa: E731
    ex = [p(n) for n in PC.EXTRAS[kind]] + [None] * (3 - len(PC.EXTRAS[kind]))
    try:
        rc = lib.dqq_newton_active_f64(R.KIND[kind], p("P"), p("q"), *ex, p("x"), *[opt(n) for n in OUTS], B, N, layout,
                                       torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    except RuntimeError as e:   # a device fault: nothing more is started on this GPU
        pytest.exit("newton active footprint %s N=%d: %s" % (kind, N, e), returncode=3)
    return a, rc


def _inputs(kind, N, B, layout, structure):
    """-> (d: CPU tensors of every input, the host core's outputs by buffer name)"""
    P, q, ex, x = C.random_problem(kind, B, N, structure)
    Pa = PC.compact(P) if layout == DIAG else P
    t = lambda a: torch.from_numpy(np.array(a, order="C"))   # noqa: E731
    d = {"P": t(Pa), "q": t(q[:, :, None]), "x": t(x[:, :, None])}
    d.update({n: t(e[:, :, None]) for n, e in zip(PC.EXTRAS[kind], ex)})
    return d, dict(zip(OUTS, C.host_active(kind, Pa, q, ex, x, diag=layout == DIAG)))


def _same(a, ref, names, rows=slice(None)):
    for n in names:
        got = a.view(n).cpu().numpy()
        assert got.dtype == ref[n].dtype and C.same_outputs([got], [ref[n][rows]]) is None, n


@pytest.mark.parametrize("family,kind,N,B,layout,structure,g", CASES, ids=lambda v: str(v))
def test_newton_active_footprint(capi, family, kind, N, B, layout, structure, g):   # noqa: F811
    d, ref = _inputs(kind, N, B, layout, structure)
    a, rc = _call(capi, kind, N, B, layout, d, g)
    assert rc == 0
    a.check_guards()
    a.check_inputs()
    for name in OUTS:
        a.check_written(name)
    _same(a, ref, OUTS)
    assert not ref["status"].any()
    for alone in ("mult", "where"):   # one output alone: the others' pointers are NULL, nothing but that output is written
        a1, rc = _call(capi, kind, N, B, layout, d, g, need=tuple(n == alone for n in OUTS))
        assert rc == 0 and set(a1.bufs) & set(OUTS) == {alone}
        a1.check_guards()
        a1.check_inputs()
        a1.check_written(alone)
        _same(a1, ref, (alone,))
    # a batch that ends on one problem, and the empty batch: nothing outside, nothing at all
    one = _tiled(d, 1)
    a, rc = _call(capi, kind, N, 1, layout, one, g)
    assert rc == 0
    a.check_guards()
    a.check_inputs()
    for name in OUTS:
        a.check_written(name)
    _same(a, ref, OUTS, slice(0, 1))
    empty = {k: v[:0] for k, v in d.items()}
    a, rc = _call(capi, kind, N, 0, layout, empty, g)
    assert rc == 0
    a.check_untouched()
