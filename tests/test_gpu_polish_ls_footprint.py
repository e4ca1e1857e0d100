"""The memory footprint of dqq_polish_ls_f64 (-m gpu): one guarded-arena case per kernel family, ragged and empty, with the
arena and the helpers of tests/test_gpu_footprint.py -- every buffer of the call carved out of one poisoned allocation, each
payload one problem past a 512-byte boundary (a batch slice).  No byte outside a payload changes, no input changes, every
output (`halvings` included) is written for every problem, and the scratch PolishLsAny is given is exactly
dqq_polish_scratch_bytes."""
import pytest
import torch

import polish_ls_cases as C
import polish_reference as R
from footprint_arena import F64, I32, U8, Arena
from test_gpu_footprint import _tiled, capi   # noqa: F401  (capi: the fixture)

pytestmark = pytest.mark.gpu
AUTO, DENSE, DIAG = 0, 1, 2
EXTRAS = {"qp": (), "qcqp": ("l_n", "mu"), "box": ("l_min", "l_max"), "sbox": ("l_min", "l_max", "v")}
MAX_HALVINGS = 8
# (family, kind, N, B, layout, structure, problems per workgroup): PolishLsDiag 4 waves of 128/N problems; PolishLsTeam 4 waves
# of 64/T teams (N = 20: T = 32); PolishLsAny a problem per workgroup
CASES = [("diag", "box", 8, 67, DIAG, "diag", 64), ("team", "sbox", 20, 37, DENSE, "dense", 8), ("any", "qcqp", 66, 3, DENSE, "dense", 1)]


def _specs(kind, N, B, layout, d, ws_bytes, slice_bytes):
    pshape = (B, N) if layout == DIAG else (B, N, N)
    eshape = (B, N // 2, 1) if kind == "qcqp" else (B, N, 1)
    specs = [("P", "in", F64, pshape, d["P"]), ("q", "in", F64, (B, N, 1), d["q"])]
    specs += [(n, "in", F64, eshape, d[n]) for n in EXTRAS[kind]]
    specs += [("x", "in", F64, (B, N, 1), d["x"]), ("x_out", "out", F64, (B, N, 1), None), ("resid", "out", F64, (B, 2), None),
              ("steps", "out", I32, (B,), None), ("status", "out", I32, (B,), None), ("halvings", "out", I32, (B,), None)]
    return specs + [("ws", "ws", U8, (ws_bytes, 0), slice_bytes)]


def _call(capi, kind, N, B, layout, d, g):
    lib = capi.lib()
    k = R.KIND[kind]
    need = lib.dqq_polish_scratch_bytes(k, N, B)
    piece = lib.dqq_polish_scratch_bytes(k, N, 1) if need else 0
    a = Arena(_specs(kind, N, B, layout, d, need, piece), g, "cuda", sliced=True)
    p = a.ptr
    ex = [p(n) for n in EXTRAS[kind]] + [None] * (3 - len(EXTRAS[kind]))
    try:
        rc = lib.dqq_polish_ls_f64(k, p("P"), p("q"), *ex, p("x"), p("x_out"), B, N, C.MAX_STEPS, layout, 0.0, MAX_HALVINGS,
                                   p("resid"), p("steps"), p("status"), p("halvings"), p("ws") if need else None, need,
                                   torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    except RuntimeError as e:   # a device fault: nothing more is started on this GPU
        pytest.exit("damped polish footprint %s N=%d: %s" % (kind, N, e), returncode=3)
    return a, rc, need


@pytest.mark.parametrize("family,kind,N,B,layout,structure,g", CASES, ids=lambda v: str(v))
def test_damped_polish_footprint(capi, family, kind, N, B, layout, structure, g):   # noqa: F811
    P, q, ex, x = C.problem(kind, N, B, structure)
    d = {"P": torch.from_numpy((C.compact(P) if layout == DIAG else P).copy()), "q": torch.from_numpy(q.copy())[:, :, None],
         "x": torch.from_numpy(x.copy())[:, :, None]}
    d.update({n: torch.from_numpy(e.copy())[:, :, None] for n, e in zip(EXTRAS[kind], ex)})
    d = {k: v.contiguous() for k, v in d.items()}
    assert (capi.lib().dqq_polish_scratch_bytes(R.KIND[kind], N, B) > 0) == (family == "any")
    a, rc, need = _call(capi, kind, N, B, layout, d, g)
    assert rc == 0
    a.check_guards()
    a.check_inputs()
    for name in ("x_out", "resid", "steps", "status", "halvings"):
        a.check_written(name)
    ref = C.host_polish_ls(kind, C.compact(P) if layout == DIAG else P, q, ex, x, C.MAX_STEPS, MAX_HALVINGS, diag=layout == DIAG)
    assert ref[4].any()
    assert C.same_bits(a.view("x_out").cpu().numpy()[:, :, 0], ref[0]) and C.same_bits(a.view("resid").cpu().numpy(), ref[1])
    assert (a.view("halvings").cpu().numpy() == ref[4]).all()
    # a batch that ends inside the first tile / team / on one problem, and the empty batch: nothing outside, nothing at all
    one = _tiled(d, 1)
    a, rc, _ = _call(capi, kind, N, 1, layout, one, g)
    assert rc == 0
    a.check_guards()
    a.check_inputs()
    assert C.same_bits(a.view("x_out").cpu().numpy()[:, :, 0], ref[0][:1])
    empty = {k: v[:0] for k, v in d.items()}
    a, rc, _ = _call(capi, kind, N, 0, layout, empty, g)
    assert rc == 0
    a.check_untouched()
