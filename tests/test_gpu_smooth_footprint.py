"""The memory footprint of dqq_polish_smooth_f64, dqq_newton_bwd_smooth_f64 and dqq_newton_jvp_smooth_f64 at kappa > 0 (-m gpu):
one guarded-arena case per new kernel family, ragged and empty, with the arena of tests/footprint_arena.py and the helpers of
tests/test_gpu_footprint.py -- every buffer of the call carved out of one poisoned allocation, each payload one problem past a
512-byte boundary (a batch slice).  No byte outside a payload changes, no input changes, every output is written for every
problem (the optional ones too), and the scratch the any-N forms are given is exactly the parents' dqq_*_scratch_bytes."""
import pytest
import torch

import polish_reference as R
import smooth_cases as SC
from footprint_arena import F64, I32, U8, Arena
from test_gpu_footprint import _tiled, capi   # noqa: F401  (capi: the fixture)

pytestmark = pytest.mark.gpu
AUTO, DENSE, DIAG = 0, 1, 2
KAPPA = 1e-2
EXTRAS = {"qp": (), "qcqp": ("l_n", "mu"), "box": ("l_min", "l_max"), "sbox": ("l_min", "l_max", "v")}
TANGENTS = ("dP", "dq", "da", "db")
H = 8
# (family, entry, kind, N, B, layout, structure, problems per workgroup): the diagonal tiles 4 waves of 128/N problems, ragged last
# tile; the LDS teams 4 waves of 64/T teams (N = 20: T = 32); the any-N forms a problem per workgroup
CASES = [("PolishSmoothDiag", "polish", "box", 8, 67, DIAG, "diag", 64), ("PolishSmoothTeam", "polish", "sbox", 20, 37, DENSE, "dense", 8),
         ("PolishSmoothAny", "polish", "qcqp", 66, 3, DENSE, "dense", 1),
         ("NewtonSmoothDiag", "bwd", "qcqp", 8, 67, DIAG, "diag", 64), ("NewtonSmoothDiag", "jvp", "sbox", 2, 259, DIAG, "diag", 256),
         ("NewtonSmoothTeam", "bwd", "box", 20, 37, AUTO, "dense", 8), ("NewtonSmoothTeam", "jvp", "qcqp", 8, 37, DENSE, "dense", 32),
         ("NewtonSmoothAny", "bwd", "sbox", 65, 3, DENSE, "dense", 1), ("NewtonSmoothAny", "jvp", "qp", 65, 3, DENSE, "dense", 1)]


def _outputs(entry, kind):
    if entry == "polish":
        return ("x_out", "resid", "steps", "status", "halvings")
    if entry == "jvp":
        return ("dx", "status")
    return ("grad_P", "grad_q", "status") + (("grad_a", "grad_b") if kind != "qp" else ())


def _specs(entry, kind, N, B, layout, d, ws_bytes, slice_bytes):
    pshape = (B, N) if layout == DIAG else (B, N, N)
    eshape = (B, N // 2, 1) if kind == "qcqp" else (B, N, 1)
    vec = (B, N, 1)
    specs = [("P", "in", F64, pshape, d["P"]), ("q", "in", F64, vec, d["q"])]
    specs += [(n, "in", F64, eshape, d[n]) for n in EXTRAS[kind]]
    specs += [("x", "in", F64, vec, d["x"])]
    if entry == "polish":
        specs += [("x_out", "out", F64, vec, None), ("resid", "out", F64, (B, 2), None), ("steps", "out", I32, (B,), None),
                  ("halvings", "out", I32, (B,), None)]
    elif entry == "bwd":
        specs += [("gx", "in", F64, vec, d["gx"]), ("grad_P", "out", F64, pshape, None), ("grad_q", "out", F64, vec, None)]
        if kind != "qp":
            specs += [("grad_a", "out", F64, eshape, None), ("grad_b", "out", F64, eshape, None)]
    else:
        specs += [("dP", "in", F64, pshape, d["dP"]), ("dq", "in", F64, vec, d["dq"])]
        if kind != "qp":
            specs += [("da", "in", F64, eshape, d["da"]), ("db", "in", F64, eshape, d["db"])]
        specs += [("dx", "out", F64, vec, None)]
    return specs + [("status", "out", I32, (B,), None), ("ws", "ws", U8, (ws_bytes, 0), slice_bytes)]


def _call(capi, entry, kind, N, B, layout, d, g):
    lib = capi.lib()
    k = R.KIND[kind]
    query = lib.dqq_polish_scratch_bytes if entry == "polish" else lib.dqq_newton_scratch_bytes
    need = query(k, N, B)
    piece = query(k, N, 1) if need else 0
    a = Arena(_specs(entry, kind, N, B, layout, d, need, piece), g, "cuda", sliced=True)
    p = a.ptr
    opt = lambda n: p(n) if kind != "qp" else None      # noqa: E731
    ex = [p(n) for n in EXTRAS[kind]] + [None] * (3 - len(EXTRAS[kind]))
    tail = (p("ws") if need else None, need, torch.cuda.current_stream().cuda_stream)
    try:
        if entry == "polish":
            rc = lib.dqq_polish_smooth_f64(k, p("P"), p("q"), *ex, p("x"), p("x_out"), B, N, SC.MAX_STEPS, layout, 0.0, KAPPA, H,
                                           p("resid"), p("steps"), p("status"), p("halvings"), *tail)
        elif entry == "bwd":
            rc = lib.dqq_newton_bwd_smooth_f64(k, p("P"), p("q"), *ex, p("x"), p("gx"), p("grad_P"), p("grad_q"), opt("grad_a"),
                                               opt("grad_b"), B, N, layout, 0.0, KAPPA, p("status"), *tail)
        else:
            rc = lib.dqq_newton_jvp_smooth_f64(k, p("P"), p("q"), *ex, p("x"), p("dP"), p("dq"), opt("da"), opt("db"), p("dx"), B, N,
                                               layout, 0.0, KAPPA, p("status"), *tail)
        torch.cuda.synchronize()
    except RuntimeError as e:   # a device fault: nothing more is started on this GPU
        pytest.exit("smoothed footprint %s %s N=%d: %s" % (entry, kind, N, e), returncode=3)
    return a, rc, need


@pytest.mark.parametrize("family,entry,kind,N,B,layout,structure,g", CASES, ids=lambda v: str(v))
def test_smoothed_family_footprint(capi, family, entry, kind, N, B, layout, structure, g):   # noqa: F811
    P, q, ex, x = SC.problem(kind, N, B, structure)
    dP, dq, da, db, gx = SC.tangents(kind, N, B, structure)
    diag = layout == DIAG
    pc = lambda M: SC.compact(M) if diag else M      # noqa: E731
    if entry != "polish":
        x = SC.host_polish(kind, pc(P), q, ex, x, SC.MAX_STEPS, H, 0.0, KAPPA, diag=diag)[0]
    col = lambda v: torch.from_numpy(v.copy())[:, :, None]      # noqa: E731
    d = {"P": torch.from_numpy(pc(P).copy()), "q": col(q), "x": col(x), "gx": col(gx), "dP": torch.from_numpy(pc(dP).copy()), "dq": col(dq)}
    d.update({n: col(e) for n, e in zip(EXTRAS[kind], ex)})
    if da is not None:
        d.update(da=col(da), db=col(db))
    d = {k: v.contiguous() for k, v in d.items()}
    query = capi.lib().dqq_polish_scratch_bytes if entry == "polish" else capi.lib().dqq_newton_scratch_bytes
    assert (query(R.KIND[kind], N, B) > 0) == family.endswith("Any")
    a, rc, need = _call(capi, entry, kind, N, B, layout, d, g)
    assert rc == 0
    a.check_guards()
    a.check_inputs()
    for name in _outputs(entry, kind):
        a.check_written(name)
    if entry == "polish":
        ref = SC.host_polish(kind, pc(P), q, ex, x, SC.MAX_STEPS, H, 0.0, KAPPA, diag=diag)
        main, first = "x_out", ref[0]
        assert SC.same_bits(a.view("resid").cpu().numpy(), ref[1]) and (a.view("halvings").cpu().numpy() == ref[4]).all()
    elif entry == "bwd":
        ref = SC.host_backward(kind, pc(P), q, ex, x, gx, 0.0, KAPPA, diag=diag)
        main, first = "grad_q", ref[1]
        assert SC.same_bits(a.view("grad_P").cpu().numpy().reshape(ref[0].shape), ref[0])
    else:
        ref = SC.host_jvp(kind, pc(P), q, ex, x, pc(dP), dq, da, db, 0.0, KAPPA, diag=diag)
        main, first = "dx", ref[0]
    assert SC.same_bits(a.view(main).cpu().numpy()[:, :, 0], first)
    # a batch that ends inside the first tile / team / on one problem, and the empty batch: nothing outside, nothing at all
    a, rc, _ = _call(capi, entry, kind, N, 1, layout, _tiled(d, 1), g)
    assert rc == 0
    a.check_guards()
    a.check_inputs()
    assert SC.same_bits(a.view(main).cpu().numpy()[:, :, 0], first[:1])
    a, rc, _ = _call(capi, entry, kind, N, 0, layout, {k: v[:0] for k, v in d.items()}, g)
    assert rc == 0
    a.check_untouched()
