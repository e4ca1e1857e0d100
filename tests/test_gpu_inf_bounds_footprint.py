"""The memory footprint of the Newton family's calls with DQQ_F_INFINITE_BOUNDS (-m gpu): guarded-arena cases, one kernel family
per entry point, ragged, one-problem and empty, with the arena of tests/footprint_arena.py as tests/test_gpu_jac_footprint.py uses
it -- every buffer of the call carved out of one poisoned allocation, each payload one problem past a 512-byte boundary.  No byte
outside a payload changes, no input changes (infinite bounds included), every output is written for every problem and equals the
flagged host core's bits."""
import numpy as np
import pytest
import torch

import inf_bounds_cases as C
import polish_reference as R
from footprint_arena import F64, I32, U8, Arena
from test_gpu_footprint import _tiled, capi   # noqa: F401  (capi: the fixture)

pytestmark = pytest.mark.gpu
AUTO, DENSE, DIAG = 0, 1, 2
# (entry, kind, N, B, layout, structure, problems per workgroup, at most)
CASES = [("polish", "box", 8, 67, DIAG, "diag", 64), ("bwd", "sbox", 20, 37, DENSE, "dense", 8),
         ("jvp", "box", 66, 5, DENSE, "dense", 1), ("jac", "sbox", 3, 37, AUTO, "dense", 32)]
OUTS = {"polish": ("x_out", "resid", "steps", "st_polish"), "bwd": ("gP", "gq", "ga", "gb", "st_bwd"), "jvp": ("dx", "st_jvp"),
        "jac": ("Jq", "Ja", "Jb", "st_jac")}
EXTRAS = {"box": ("l_min", "l_max"), "sbox": ("l_min", "l_max", "v")}


def _scratch(lib, entry, k, N, B, layout):
    if layout == DIAG:
        return 0
    return {"polish": lib.dqq_polish_scratch_bytes, "jac": lib.dqq_newton_jac_scratch_bytes}.get(entry, lib.dqq_newton_scratch_bytes)(k, N, B)


def _call(capi, entry, kind, N, B, layout, d, ref, g):   # noqa: F811
    lib = capi.lib()
    k = R.KIND[kind]
    ws_need, piece = _scratch(lib, entry, k, N, B, layout), _scratch(lib, entry, k, N, 1, layout)
    pshape = (B, N) if layout == DIAG else (B, N, N)
    ins = ["P", "q"] + list(EXTRAS[kind]) + ["x"] + {"bwd": ["gx"], "jvp": ["dP", "dq", "da", "db"]}.get(entry, [])
    specs = [(n, "in", F64, (pshape if n in ("P", "dP") else (B, N, 1)), d[n]) for n in ins]
    specs += [(n, "out", I32 if ref[n].dtype == np.int32 else F64, (B,) + ref[n].shape[1:], None) for n in OUTS[entry]]
    a = Arena(specs + [("ws", "ws", U8, (ws_need, 0), piece)], g, "cuda", sliced=True)
    p = a.ptr
    ex = [p(n) for n in EXTRAS[kind]] + [None] * (3 - len(EXTRAS[kind]))
    fl = layout | C.F_INFINITE_BOUNDS
    tail = (p("ws") if ws_need else None, ws_need, torch.cuda.current_stream().cuda_stream)
    try:
        if entry == "polish":
            rc = lib.dqq_polish_f64(k, p("P"), p("q"), *ex, p("x"), p("x_out"), B, N, C.MAX_STEPS, fl, p("resid"), p("steps"),
                                    p("st_polish"), *tail)
        elif entry == "bwd":
            rc = lib.dqq_newton_bwd_f64(k, p("P"), p("q"), *ex, p("x"), p("gx"), p("gP"), p("gq"), p("ga"), p("gb"), B, N, fl,
                                        p("st_bwd"), *tail)
        elif entry == "jvp":
            rc = lib.dqq_newton_jvp_f64(k, p("P"), p("q"), *ex, p("x"), p("dP"), p("dq"), p("da"), p("db"), p("dx"), B, N, fl,
                                        p("st_jvp"), *tail)
        else:
            rc = lib.dqq_newton_jac_f64(k, p("P"), p("q"), *ex, p("x"), p("Jq"), p("Ja"), p("Jb"), B, N, fl, p("st_jac"), *tail)
        torch.cuda.synchronize()
    except RuntimeError as e:   # a device fault: nothing more is started on this GPU
        pytest.exit("infinite-bounds footprint %s %s N=%d: %s" % (entry, kind, N, e), returncode=3)
    return a, rc


def _check(a, entry, ref, rows=slice(None)):
    a.check_guards()
    a.check_inputs()
    for n in OUTS[entry]:
        a.check_written(n)
        got = a.view(n).cpu().numpy()
        assert C.same_bits(got.reshape(ref[n][rows].shape), ref[n][rows]), n


@pytest.mark.parametrize("entry,kind,N,B,layout,structure,g", CASES, ids=lambda v: str(v))
def test_flagged_calls_footprint(capi, entry, kind, N, B, layout, structure, g):   # noqa: F811
    P, q, ex, x, gx, tan = C.problem(kind, B, N, structure, bad_row=B // 2)
    diag = layout == DIAG
    Pa, dPa = (C.compact(P), C.compact(tan[0])) if diag else (P, tan[0])
    ref = C.host_all(kind, Pa, q, ex, x, gx, (dPa,) + tan[1:], diag=diag, flag=True)
    assert ref["st_" + entry][B // 2] == 2
    t = lambda v: torch.from_numpy(np.array(v, order="C"))   # noqa: E731
    d = {"P": t(Pa), "dP": t(dPa)}
    d.update({n: t(v[:, :, None]) for n, v in zip(("q", "x", "gx", "dq", "da", "db") + EXTRAS[kind], (q, x, gx) + tan[1:] + ex)})
    assert torch.isinf(d["l_min"]).any() and torch.isinf(d["l_max"]).any()
    a, rc = _call(capi, entry, kind, N, B, layout, d, ref, g)
    assert rc == 0
    _check(a, entry, ref)
    one = _tiled(d, 1)
    a, rc = _call(capi, entry, kind, N, 1, layout, one, ref, g)
    assert rc == 0
    _check(a, entry, ref, slice(0, 1))
    a, rc = _call(capi, entry, kind, N, 0, layout, {n: v[:0] for n, v in d.items()}, ref, g)
    assert rc == 0
    a.check_untouched()
