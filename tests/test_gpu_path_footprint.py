"""The memory footprint of dqq_polish_path_f64 (-m gpu): one guarded-arena case per new kernel family, ragged, sliced and empty,
with the arena of tests/footprint_arena.py and the helpers of tests/test_gpu_footprint.py -- every buffer of the call carved out of
one poisoned allocation, each payload one problem past a 512-byte boundary (a batch slice).  No byte outside a payload changes, no
input changes, every output is written for every problem -- the per-stage outputs to their full extents (B,S,2) and (B,S), for
S = 1 and S = 8 --, and the scratch the any-N form is given is exactly dqq_polish_scratch_bytes."""
import ctypes

import pytest
import torch

import path_cases as PC
import polish_reference as R
from footprint_arena import F64, I32, U8, Arena
from test_gpu_footprint import _tiled, capi   # noqa: F401  (capi: the fixture)

pytestmark = pytest.mark.gpu
AUTO, DENSE, DIAG = 0, 1, 2
EXTRAS = {"qp": (), "qcqp": ("l_n", "mu"), "box": ("l_min", "l_max"), "sbox": ("l_min", "l_max", "v")}
OUTPUTS = ("x_out", "resid", "steps", "status", "halvings", "stage_resid", "stage_steps")
H = 8
ONE = ((1e-2,), (6,))
# (family, kind, N, B, layout, structure, problems per workgroup): the diagonal tiles 4 waves of 128/N problems, ragged last tile;
# the LDS teams 4 waves of 64/T teams (N = 20: T = 32); the any-N form a problem per workgroup
CASES = [("PolishPathDiag", "box", 8, 67, DIAG, "diag", 64), ("PolishPathDiag", "qcqp", 2, 259, DIAG, "diag", 256),
         ("PolishPathTeam", "sbox", 20, 37, DENSE, "dense", 8), ("PolishPathTeam", "qp", 8, 37, AUTO, "dense", 32),
         ("PolishPathAny", "qcqp", 66, 3, DENSE, "dense", 1)]


def _specs(kind, N, B, S, layout, d, ws_bytes, slice_bytes):
    pshape = (B, N) if layout == DIAG else (B, N, N)
    eshape = (B, N // 2, 1) if kind == "qcqp" else (B, N, 1)
    vec = (B, N, 1)
    specs = [("P", "in", F64, pshape, d["P"]), ("q", "in", F64, vec, d["q"])]
    specs += [(n, "in", F64, eshape, d[n]) for n in EXTRAS[kind]]
    specs += [("x", "in", F64, vec, d["x"]), ("x_out", "out", F64, vec, None), ("resid", "out", F64, (B, 2), None),
              ("steps", "out", I32, (B,), None), ("status", "out", I32, (B,), None), ("halvings", "out", I32, (B,), None),
              ("stage_resid", "out", F64, (B, S, 2), None), ("stage_steps", "out", I32, (B, S), None)]
    return specs + [("ws", "ws", U8, (ws_bytes, 0), slice_bytes)]


def _call(capi, kind, N, B, layout, schedule, d, g):
    lib = capi.lib()
    k, S = R.KIND[kind], len(schedule[0])
    need = lib.dqq_polish_scratch_bytes(k, N, B)
    piece = lib.dqq_polish_scratch_bytes(k, N, 1) if need else 0
    a = Arena(_specs(kind, N, B, S, layout, d, need, piece), g, "cuda", sliced=True)
    p = a.ptr
    ex = [p(n) for n in EXTRAS[kind]] + [None] * (3 - len(EXTRAS[kind]))
    ks, ns = (ctypes.c_double * S)(*schedule[0]), (ctypes.c_int * S)(*schedule[1])
    try:
        rc = lib.dqq_polish_path_f64(k, p("P"), p("q"), *ex, p("x"), p("x_out"), B, N, layout, 0.0, ctypes.addressof(ks),
                                     ctypes.addressof(ns), S, H, p("resid"), p("steps"), p("status"), p("halvings"), p("stage_resid"),
                                     p("stage_steps"), p("ws") if need else None, need, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    except RuntimeError as e:   # a device fault: nothing more is started on this GPU
        pytest.exit("path footprint %s N=%d: %s" % (kind, N, e), returncode=3)
    return a, rc


@pytest.mark.parametrize("schedule", (ONE, PC.LONG), ids=("S1", "S8"))
@pytest.mark.parametrize("family,kind,N,B,layout,structure,g", CASES, ids=lambda v: str(v))
def test_path_family_footprint(capi, family, kind, N, B, layout, structure, g, schedule):   # noqa: F811
    P, q, ex, x = PC.problem(kind, N, B, structure)
    diag = layout == DIAG
    pc = lambda M: PC.compact(M) if diag else M      # noqa: E731
    col = lambda v: torch.from_numpy(v.copy())[:, :, None]      # noqa: E731
    d = {"P": torch.from_numpy(pc(P).copy()), "q": col(q), "x": col(x)}
    d.update({n: col(e) for n, e in zip(EXTRAS[kind], ex)})
    d = {k: v.contiguous() for k, v in d.items()}
    assert (capi.lib().dqq_polish_scratch_bytes(R.KIND[kind], N, B) > 0) == family.endswith("Any")
    a, rc = _call(capi, kind, N, B, layout, schedule, d, g)
    assert rc == 0
    a.check_guards()
    a.check_inputs()
    for name in OUTPUTS:
        a.check_written(name)
    ref = PC.host_path(kind, pc(P), q, ex, x, schedule[0], schedule[1], H, 0.0, diag=diag)
    for name, r in zip(OUTPUTS, ref):
        assert PC.same_bits(a.view(name).cpu().numpy().reshape(r.shape), r), name
    # a batch that ends inside the first tile / team / on one problem, and the empty batch: nothing outside, nothing at all
    a, rc = _call(capi, kind, N, 1, layout, schedule, _tiled(d, 1), g)
    assert rc == 0
    a.check_guards()
    a.check_inputs()
    for name, r in zip(OUTPUTS, ref):
        assert PC.same_bits(a.view(name).cpu().numpy().reshape((1,) + r.shape[1:]), r[:1]), name
    a, rc = _call(capi, kind, N, 0, layout, schedule, {k: v[:0] for k, v in d.items()}, g)
    assert rc == 0
    a.check_untouched()
