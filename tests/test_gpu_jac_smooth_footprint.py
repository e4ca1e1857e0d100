"""The memory footprint of dqq_newton_jac_smooth_f64 at kappa > 0 (-m gpu): a guarded arena per new kernel family, ragged, sliced,
one-problem and empty batches and every subset of outputs, with the arena of tests/footprint_arena.py -- every buffer of the call
carved out of one poisoned allocation, each payload one problem past a 512-byte boundary (a batch slice that starts at an odd
problem).  No byte outside a payload changes, no input changes, every requested output is written for every problem and equals the
host core's bits, an output that is not requested does not exist, and the scratch NewtonJacSmoothAny is given is exactly
dqq_newton_jac_scratch_bytes."""
import numpy as np
import pytest
import torch

import jac_smooth_cases as C
import polish_cases as PC
import polish_reference as R
from footprint_arena import Arena
from test_gpu_footprint import _tiled, capi   # noqa: F401  (capi: the fixture)
from test_gpu_jac_footprint import OUTS, _same, _specs

pytestmark = pytest.mark.gpu
AUTO, DENSE, DIAG = 0, 1, 2
KAPPA = C.KAPPA
# (family, kind, N, B, layout, structure, problems per workgroup, at most): the hard Jacobian kernels' geometry
CASES = [("diag", "qcqp", 8, 67, DIAG, "diag", 64), ("diag", "sbox", 64, 5, DIAG, "diag", 8), ("diag", "qp", 2, 259, DIAG, "diag", 256),
         ("team", "box", 20, 37, DENSE, "dense", 8), ("team", "qp", 3, 37, AUTO, "dense", 32),
         ("team", "qcqp", 8, 37, DENSE, "dense", 32), ("team", "sbox", 64, 3, DENSE, "dense", 1),
         ("any", "qcqp", 66, 5, DENSE, "dense", 1), ("any", "sbox", 66, 5, DENSE, "dense", 1)]


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
        rc = lib.dqq_newton_jac_smooth_f64(k, p("P"), p("q"), *ex, p("x"), opt("Jq"), opt("Ja"), opt("Jb"), B, N, layout, 0.0, KAPPA,
                                           p("status"), p("ws") if ws_need else None, ws_need - short,
                                           torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    except RuntimeError as e:   # a device fault: nothing more is started on this GPU
        pytest.exit("smoothed newton jac footprint %s N=%d: %s" % (kind, N, e), returncode=3)
    return a, rc, ws_need


def _inputs(kind, N, B, layout, structure):
    """-> (d: CPU tensors of every input by buffer name, the host core's outputs by buffer name)"""
    P, q, ex, x = C.problem(kind, N, B, structure)
    diag = layout == DIAG
    Pa = C.compact(P) if diag else P
    t = lambda a: torch.from_numpy(np.array(a, order="C"))   # noqa: E731
    d = {"P": t(Pa), "q": t(q[:, :, None]), "x": t(x[:, :, None])}
    d.update({n: t(e[:, :, None]) for n, e in zip(PC.EXTRAS[kind], ex)})
    h = C.host_jac(kind, Pa, q, ex, x, diag=diag, kappa=KAPPA)
    return d, {"Jq": h[0], "Ja": h[1], "Jb": h[2], "status": h[3]}


@pytest.mark.parametrize("family,kind,N,B,layout,structure,g", CASES, ids=lambda v: str(v))
def test_smoothed_newton_jac_footprint(capi, family, kind, N, B, layout, structure, g):   # noqa: F811
    d, ref = _inputs(kind, N, B, layout, structure)
    need_any = capi.lib().dqq_newton_jac_scratch_bytes(R.KIND[kind], N, B)
    assert (need_any > 0) == (family == "any") and C.cell(kind, N, B, layout)[1] == family
    assert not ref["status"].any()
    for need in C.subsets(kind):        # every subset of outputs: only what is requested exists, and it is the host core's bits
        a, rc, ws_need = _call(capi, kind, N, B, layout, d, g, need)
        assert rc == 0 and ws_need == need_any
        a.check_guards()
        a.check_inputs()
        names = tuple(n for n, nd in zip(OUTS, need) if nd and ref[n] is not None) + ("status",)
        assert {n for n in OUTS if n in a.bufs} == set(names[:-1])
        for name in names:
            a.check_written(name)
        _same(a, ref, names)
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
    names = tuple(n for n in OUTS + ("status",) if n in a.bufs)
    for name in names:
        a.check_written(name)
    _same(a, ref, OUTS + ("status",), slice(0, 1))
    empty = {k: v[:0] for k, v in d.items()}
    a, rc, _ = _call(capi, kind, N, 0, layout, empty, g)
    assert rc == 0
    a.check_untouched()
