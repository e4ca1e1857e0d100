"""The memory footprint of dqq_jvp_f64 (-m gpu): one guarded-arena case per kernel family and addressing pattern, ragged, with
ir_steps = NULL, with NULL tangents, on one problem and empty, with the arena and the helpers of tests/test_gpu_footprint.py --
every buffer of the call carved out of one poisoned allocation, each payload one problem past a 512-byte boundary (a batch
slice: 8-byte aligned only for odd N).  No byte outside a payload changes, no input changes (every tangent is an input), dx
and ir_steps are written for every problem and hold the host core's bits, an output that was not handed over stays as it
was.  JvpAny is given exactly dqq_workspace_bytes + the backward's reference-order dqq_scratch_bytes: the work-list in front of
the scratch is not touched, and one byte less is DQQ_E_WORKSPACE without a launch."""
import numpy as np
import pytest
import torch

import jvp_cases as C
import jvp_reference as R
from footprint_arena import Arena, jvp_call_specs, run_jvp
from test_gpu_footprint import _tiled, capi   # noqa: F401  (capi: the fixture)

pytestmark = pytest.mark.gpu
AUTO, DENSE, DIAG = 0, 1, 2
REF = 0x100
E_WORKSPACE = -5
# (family, kind, N, B, layout, structure, problems per workgroup).  JvpDiag (jvp_diag.hip launch_one): 4 waves of 128 / N
# problems.  JvpTeam (jvp_dense.hip launch_jvp_team, the geometry of the backward's team kernel, footprint_cases.launch_g
# "bteam"): teams of T = 8 / 16 / 32 / 64 lanes for bwd_system_rows <= T, as many waves (<= 4) as 64 KiB of LDS hold -- box
# N = 21: 63 rows, T = 64, 98 400 bytes per wave, one wave, g = 1; QP N = 3: T = 8, 8 teams a wave, 4 waves, g = 32.  JvpAny
# (jvp_any.hip): a problem per workgroup.  tests/test_footprint_cases.py holds the g column against launch_g.
CASES = [("diag", "qcqp", 8, 67, DIAG, "diag", 64), ("diag", "sbox", 64, 5, DIAG, "diag", 8),
         ("team", "box", 21, 37, DENSE, "dense", 1), ("team", "qp", 3, 37, AUTO, "dense", 32),
         ("any", "box", 22, 5, DENSE, "dense", 1), ("any", "qcqp", 44, 5, DENSE, "dense", 1)]


def inputs(kind, N, B, layout, structure):
    """-> (d: the call's inputs as CPU tensors, tangents and x among them; the numpy batch, x and flat tangents host_jvp takes)"""
    dn, x = C.problem(kind, N, B, structure)
    tan = R.random_tangents(kind, B, N, 43 + N, diag=layout == DIAG)
    t = lambda a: torch.from_numpy(np.array(a, order="C"))   # noqa: E731
    d = {k: t(v) for k, v in dn.items() if k in ("P", "q") + C.EXTRAS[kind]}
    d.update(x=t(x), dP=t(tan[0]), dq=t(tan[1][:, :, None]))
    if kind != "qp":
        d.update(da=t(tan[2][:, :, None]), db=t(tan[3][:, :, None]))
    if layout == DIAG:
        d["P"] = torch.diagonal(d["P"], dim1=1, dim2=2).contiguous()
        d["dP"] = torch.diagonal(d["dP"], dim1=1, dim2=2).contiguous()
    return d, dn, x, tan


def workspace(lib, kind, N, B, layout):
    """(bytes of the workspace, of the work-list in front, of one workgroup's scratch slice): all 0 but for JvpAny.  (The
    backward's query knows nothing of the compact layout's N limit: DQQ_P_DIAG is JvpDiag, which looks at no workspace.)"""
    k = min(R.KIND[kind], 2)
    scratch = lib.dqq_scratch_bytes(k, 1, N, B, layout | REF) if (B and layout != DIAG) else 0
    if not scratch:
        return 0, 0, 0
    head = lib.dqq_workspace_bytes(B)
    return head + scratch, head, lib.dqq_scratch_bytes(k, 1, N, 1, layout | REF)


def call(capi, kind, N, B, layout, d, g, **kw):   # noqa: F811
    lib = capi.lib()
    a = Arena(jvp_call_specs(kind, N, B, layout, d, *workspace(lib, kind, N, B, layout)), g, "cuda", sliced=True)
    try:
        rc = run_jvp(lib, a, kind, N, B, layout, torch.cuda.current_stream().cuda_stream, C.EPSILON, **kw)
        torch.cuda.synchronize()
    except RuntimeError as e:   # a device fault: nothing more is started on this GPU
        pytest.exit("jvp footprint %s N=%d: %s" % (kind, N, e), returncode=3)
    return a, rc


def bits(t):
    return t.cpu().numpy().view(np.int64)


def check(a, rc, ref, ref_steps, steps=True):
    assert rc == 0
    a.check_guards()
    a.check_inputs()
    a.check_written("dx")
    assert np.array_equal(bits(a.view("dx"))[:, :, 0], ref.view(np.int64)), "dx is not the host core's"
    if steps:
        a.check_written("ir_steps")
        assert np.array_equal(a.view("ir_steps").cpu().numpy().reshape(ref_steps.shape), ref_steps)
    else:
        a.check_pristine("ir_steps")
    if "ws" in a.bufs:   # include/diffqcqp_hip.h: "the work-list itself is not touched"
        a.check_pristine("ws", a.bufs["ws"]["shape"][1])


@pytest.mark.parametrize("family,kind,N,B,layout,structure,g", CASES, ids=lambda v: str(v))
def test_jvp_footprint(oracle, capi, family, kind, N, B, layout, structure, g):   # noqa: F811
    d, dn, x, tan = inputs(kind, N, B, layout, structure)
    assert (workspace(capi.lib(), kind, N, B, layout)[0] > 0) == (family == "any")
    ref, ref_steps = C.host_jvp(kind, dn, x, tan)
    a, rc = call(capi, kind, N, B, layout, d, g)
    check(a, rc, ref, ref_steps)
    # (a) ir_steps = NULL: dx as before, the buffer that was not handed over as it was
    a, rc = call(capi, kind, N, B, layout, d, g, steps=False)
    check(a, rc, ref, ref_steps, steps=False)
    # (b) every tangent but dq NULL: the others are not read (they stay in the arena, poisoned reads would show in dx)
    only, only_steps = C.host_jvp(kind, dn, x, (None, tan[1], None, None)[:len(tan)])
    a, rc = call(capi, kind, N, B, layout, d, g, only_dq=True)
    check(a, rc, only, only_steps)
    # (c) a batch that ends inside the first tile / team, on one problem; (d) the empty batch: nothing at all
    a, rc = call(capi, kind, N, 1, layout, _tiled(d, 1), g)
    check(a, rc, ref[:1], ref_steps[:1])
    a, rc = call(capi, kind, N, 0, layout, {k: v[:0] for k, v in d.items()}, g)
    assert rc == 0
    a.check_untouched()
    if family == "any":   # one byte less of workspace: refused before any launch
        a, rc = call(capi, kind, N, B, layout, d, g, ws_short=1)
        assert rc == E_WORKSPACE
        a.check_untouched()
