"""The memory footprint of dqq_polish_reg_f64, dqq_newton_bwd_reg_f64, dqq_newton_jvp_reg_f64 and dqq_newton_jac_reg_f64 with
reg != 0 (-m gpu): a guarded-arena case per kernel family and entry, with the arena of tests/footprint_arena.py -- every buffer of
the call carved out of one poisoned allocation, each payload one problem past a 512-byte boundary (a batch slice that starts at an
odd problem) --, and the empty batch.  No byte outside a payload changes, no input changes, every output is written for every
problem and equals the host core's bits (tests/hostcore/reg_core_check.cpp), and the scratch the any-N form is given is exactly
the parent's query.  Inputs: the singular batches of tests/reg_cases.py."""
import numpy as np
import pytest
import torch

import polish_reference as R
import reg_cases as C
from footprint_arena import F64, I32, U8, Arena
from test_gpu_footprint import capi   # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
AUTO, DENSE, DIAG = 0, 1, 2
EXTRAS = {"qp": (), "qcqp": ("a", "b"), "box": ("a", "b"), "sbox": ("a", "b", "c")}
# (family, kind, N, B, layout, mode, problems per workgroup): the diagonal form 4 waves of 128/N problems; teams 4 waves of 64/T
# (N = 20: T = 32; N = 8: T = 8); the any-N form a problem per workgroup
CASES = [("diag", "qcqp", 8, 37, DIAG, "diagzero", 64), ("diag", "box", 2, 37, DIAG, "diagzero", 256),
         ("team", "sbox", 20, 37, DENSE, "lowrank", 8), ("team", "qp", 8, 37, AUTO, "duprow", 32),
         ("team", "qcqp", 8, 37, DENSE, "lowrank", 32), ("any", "box", 72, 5, DENSE, "lowrank", 1),
         ("any", "qcqp", 72, 5, DENSE, "lowrank", 1)]
ENTRIES = ("polish", "bwd", "jvp", "jac")
SCRATCH = {"polish": "dqq_polish_scratch_bytes", "bwd": "dqq_newton_scratch_bytes", "jvp": "dqq_newton_scratch_bytes",
           "jac": "dqq_newton_jac_scratch_bytes"}


def _outs(entry, kind):
    if entry == "polish":
        return ("x_out", "resid", "steps", "status")
    if entry == "jvp":
        return ("dx", "status")
    if entry == "bwd":
        return ("grad_P", "grad_q") + (("grad_a", "grad_b") if kind != "qp" else ()) + ("status",)
    return ("Jq",) + (("Ja", "Jb") if kind != "qp" else ()) + ("status",)


def _specs(entry, kind, N, B, layout, d, ws_bytes, slice_bytes):
    diag = layout == DIAG
    pshape = (B, N) if diag else (B, N, N)
    eshape = (B, N // 2, 1) if kind == "qcqp" else (B, N, 1)
    sq, sa, sb = C.jac_shapes(kind, B, N, diag)
    specs = [("P", "in", F64, pshape, d["P"]), ("q", "in", F64, (B, N, 1), d["q"])]
    specs += [(n, "in", F64, eshape, d[n]) for n in EXTRAS[kind]]
    if entry == "polish":
        specs += [("x", "in", F64, (B, N, 1), d["x0"]), ("x_out", "out", F64, (B, N, 1), None), ("resid", "out", F64, (B, 2), None),
                  ("steps", "out", I32, (B,), None)]
    else:
        specs += [("x", "in", F64, (B, N, 1), d["x"])]
    if entry == "bwd":
        specs += [("grad_x", "in", F64, (B, N, 1), d["grad_x"]), ("grad_P", "out", F64, pshape, None),
                  ("grad_q", "out", F64, (B, N, 1), None)]
        if kind != "qp":
            specs += [("grad_a", "out", F64, eshape, None), ("grad_b", "out", F64, eshape, None)]
    if entry == "jvp":
        specs += [("dP", "in", F64, pshape, d["dP"]), ("dq", "in", F64, (B, N, 1), d["dq"])]
        if kind != "qp":
            specs += [("da", "in", F64, eshape, d["da"]), ("db", "in", F64, eshape, d["db"])]
        specs += [("dx", "out", F64, (B, N, 1), None)]
    if entry == "jac":
        specs += [("Jq", "out", F64, sq, None)]
        if kind != "qp":
            specs += [("Ja", "out", F64, sa, None), ("Jb", "out", F64, sb, None)]
    specs += [("status", "out", I32, (B,), None)]
    return specs + [("ws", "ws", U8, (ws_bytes, 0), slice_bytes)]


def _call(capi, entry, kind, N, B, layout, d, g, reg):   # noqa: F811
    lib = capi.lib()
    k = R.KIND[kind]
    need = getattr(lib, SCRATCH[entry])(k, N, B) if layout != DIAG else 0
    piece = getattr(lib, SCRATCH[entry])(k, N, 1) if need else 0
    a = Arena(_specs(entry, kind, N, B, layout, d, need, piece), g, "cuda", sliced=True)
    p = a.ptr
    opt = lambda n: p(n) if n in a.bufs else None   # noqa: E731
    ex = [p(n) for n in EXTRAS[kind]] + [None] * (3 - len(EXTRAS[kind]))
    ws = (p("ws") if need else None, need, torch.cuda.current_stream().cuda_stream)
    try:
        if entry == "polish":
            rc = lib.dqq_polish_reg_f64(k, p("P"), p("q"), *ex, p("x"), p("x_out"), B, N, 8, layout, reg, p("resid"), p("steps"),
                                        p("status"), *ws)
        elif entry == "bwd":
            rc = lib.dqq_newton_bwd_reg_f64(k, p("P"), p("q"), *ex, p("x"), p("grad_x"), p("grad_P"), p("grad_q"), opt("grad_a"),
                                            opt("grad_b"), B, N, layout, reg, p("status"), *ws)
        elif entry == "jvp":
            rc = lib.dqq_newton_jvp_reg_f64(k, p("P"), p("q"), *ex, p("x"), p("dP"), p("dq"), opt("da"), opt("db"), p("dx"), B, N,
                                            layout, reg, p("status"), *ws)
        else:
            rc = lib.dqq_newton_jac_reg_f64(k, p("P"), p("q"), *ex, p("x"), p("Jq"), opt("Ja"), opt("Jb"), B, N, layout, reg,
                                            p("status"), *ws)
        torch.cuda.synchronize()
    except RuntimeError as e:   # a device fault: nothing more is started on this GPU
        pytest.exit("reg footprint %s %s N=%d: %s" % (entry, kind, N, e), returncode=3)
    return a, rc, need


def _inputs(kind, N, B, layout, mode, reg):
    """-> (d: CPU tensors of every input of every entry, the host core's outputs by entry and buffer name)"""
    b = C.batch(kind, N, mode, B)
    diag = layout == DIAG
    P, q, ex, x = (b["pdiag"] if diag else b["P"]), b["q"], b["ex"], b["x"]
    tan, g = C.inputs(kind, N, B)
    if diag:
        tan = (np.ascontiguousarray(np.einsum("bii->bi", tan[0])),) + tuple(tan[1:])
    x0 = np.stack([R.project(kind, x[i] + 1e-3 * np.sin(np.arange(N) + i), tuple(e[i] for e in ex), N) for i in range(B)])
    t = lambda a: torch.from_numpy(np.array(a, order="C"))   # noqa: E731
    d = dict(P=t(P), q=t(q[:, :, None]), x=t(x[:, :, None]), x0=t(x0[:, :, None]), grad_x=t(g[:, :, None]), dP=t(tan[0]),
             dq=t(tan[1][:, :, None]))
    d.update({n: t(e[:, :, None]) for n, e in zip(EXTRAS[kind], ex)})
    if kind != "qp":
        d.update(da=t(tan[2][:, :, None]), db=t(tan[3][:, :, None]))
    hp = C.host_polish(kind, P, q, ex, x0, 8, reg, diag)
    hj = C.host_jvp(kind, P, q, ex, x, tan, reg, diag)
    hb = C.host_backward(kind, P, q, ex, x, g, reg, diag)
    hc = C.host_jacobian(kind, P, q, ex, x, reg, diag)
    ref = {"polish": {"x_out": hp[0], "resid": hp[1], "steps": hp[2], "status": hp[3]}, "jvp": {"dx": hj[0], "status": hj[1]},
           "bwd": {"grad_P": hb[0], "grad_q": hb[1], "grad_a": hb[2], "grad_b": hb[3], "status": hb[4]},
           "jac": {"Jq": hc[0], "Ja": hc[1], "Jb": hc[2], "status": hc[3]}}
    return d, ref


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("family,kind,N,B,layout,mode,g", CASES, ids=lambda v: str(v))
def test_reg_footprint(capi, entry, family, kind, N, B, layout, mode, g):   # noqa: F811
    reg = C.REG
    d, ref = _inputs(kind, N, B, layout, mode, reg)
    lib = capi.lib()
    need_any = getattr(lib, SCRATCH[entry])(R.KIND[kind], N, B) if layout != DIAG else 0
    assert (need_any > 0) == (family == "any")
    a, rc, need = _call(capi, entry, kind, N, B, layout, d, g, reg)
    assert rc == 0 and need == need_any
    a.check_guards()
    a.check_inputs()
    for name in _outs(entry, kind):
        a.check_written(name)
        got = a.view(name).cpu().numpy()
        want = ref[entry][name]
        assert C.same_bits(got.reshape(want.shape), want) if want.dtype != np.int32 else np.array_equal(got, want), name
    assert not ref[entry]["status"].any() or entry == "polish"     # the weight's point: no status 1 on a singular free block
    # the empty batch: nothing at all
    empty = {k: v[:0] for k, v in d.items()}
    a, rc, _ = _call(capi, entry, kind, N, 0, layout, empty, g, reg)
    assert rc == 0
    a.check_untouched()
