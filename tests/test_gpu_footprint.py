"""The memory footprint of every kernel route on ragged, sliced and empty batches (run with -m gpu on an MI355X).

Each case of tests/footprint_cases.py is one call straight through the C ABI, every optional output requested, with every
buffer carved out of a guarded, poisoned arena (tests/footprint_arena.py) and the workspace exactly dqq_workspace_bytes +
dqq_scratch_bytes long.  After one synchronisation: rc == 0; every guard byte still holds its sentinel; every input is
unchanged bit for bit; no sentinel is left in [0, B) of x, iters, every gradient, ir_steps, gamma / dgamma and
diag_flags_out (pdiag_out: the problems flagged 1, which must hold the diagonal of P); the work-list header is zero again
and dqq_workspace_status reports clean; the values meet the bars the project already has (forward: x within X_TOL of the
oracle; backward on the oracle's x: _check_rows of tests/test_gpu_parameters.py -- bit-exact for bdiag, 1e-9 for the
reference-order kernels, REASSOC_TOL for the matrix-core kernels with min_same = 0: at 1 to 130 problems a share of equal
refinement exits is noise, and a problem whose exit differs is still held against the oracle forced to the kernel's step
count).  Then the same call with every payload on a 512-byte boundary of a fresh arena: bit-identical outputs.
B = 0: rc == 0 and the whole arena untouched.

Alignment, established from the sources before the first run.  The payloads sit where `t[1:]` of a torch tensor would: one
problem past a 512-byte boundary, i.e. 8 N bytes for q / x / grad_x / bounds / grad_q, 8 N N for P / grad_P, 4 N for the
QCQP's l_n / mu / grad_l_n / grad_mu / gamma / dgamma, 4 (8 for the box backward) for iters / ir_steps, 1 for diag_flags_out.
  * 16-byte vector accesses (double2) to caller pointers exist in fwd_diag.hip (q, box bounds, v, P as DQQ_P_DIAG, x,
    pdiag_out), stream_tile.h / group_dense.h (P, q, x), fwd_lane_dense.hip (P, q, box bounds, v, x), fwd_small.hip (P),
    bwd_diag.hip (P as DQQ_P_DIAG, pdiag, q, x, grad_x, box bounds, grad_q, grad_P's diagonal, box gradients and duals) and
    bwd_lane_dense.hip (P, q, x, grad_x).  Each is at an even element offset from its (B,N,..) buffer's base, so what they
    assume is a 16-byte aligned base.
  * Every one of these kernels is instantiated for even N only (fdiag / bdiag: 2, 4, ..., 64; flane / blane: 2, 4, 6, 8;
    fsmall: 10 .. 16 even): 8 N and 8 N N are multiples of 16, a one-problem offset keeps the alignment.  The box duals
    (B, 2 N) likewise.
  * The (B, N/2) buffers of the QCQP -- 8 bytes off for N = 2, 6, 10, 14 -- the int and byte buffers, and every buffer of
    the kernels that take odd N (dense.hip, dense_wave64.hip, bwd_wave_qcqp*.hip, general_any.hip) are touched element by
    element only.  The work-list header is read in 8-byte words (report.h worklist_feedback, bwd_lane_dense.hip
    report_nondiagonal): the workspace is not a batch slice and stays on a 512-byte boundary.
So no route needs more alignment than a batch slice gives."""
import numpy as np
import pytest
import torch

from conftest import make_problem
from footprint_arena import Arena, call_specs, run_call
from footprint_cases import CASES, case_g, case_id, case_seed
from param_cases import DIAG, KIND, F, base_size, tile
from test_gpu_parameters import _check_rows, _families, _obwd, _ofwd
from test_gpu_parity import X_TOL, npy, oracle_fwd
from test_gpu_worklist_guard import ENTRIES

pytestmark = pytest.mark.gpu
OUTPUTS = {0: ("x", "iters", "diag_flags_out"),
           1: {"qp": ("grad_P", "grad_q", "ir_steps"),
               "qcqp": ("grad_P", "grad_q", "grad_l_n", "grad_mu", "gamma", "dgamma", "ir_steps"),
               "box": ("grad_P", "grad_q", "grad_l_min", "grad_l_max", "gamma", "dgamma", "ir_steps")}}


@pytest.fixture(scope="module")
def capi():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from diffqcqp_amd import build, _capi
    build.build()
    _capi.lib()
    return _capi


# the oracle's answers on a group's base batch: computed once, shared by the group's cases (problem b is problem b mod base)
_BASE_B = {}
for _c in CASES:
    _BASE_B[_c[:3] + _c[4:6]] = max(_BASE_B.get(_c[:3] + _c[4:6], 1), _c[3])
_ref = {}


def _reference(oracle, case):
    pas, kind, N, B, layout, structure, _ = case
    key = case[:3] + case[4:6]
    if key not in _ref:
        _ref.clear()
        base = make_problem(kind, base_size(N, _BASE_B[key]), N, case_seed(case), structure)
        xo = _ofwd(oracle, kind, base, 1e-7, 1000)[0]
        _ref[key] = (base, xo, _obwd(oracle, kind, base, xo, 1e-10) if pas != F else None)
    return _ref[key]


def _tiled(base, B):
    nb = base["q"].shape[0]
    reps = -(-B // nb)
    return {k: v.repeat((reps,) + (1,) * (v.dim() - 1))[:B].contiguous() for k, v in base.items()}


def _call(capi, case, full, x, sliced):
    """One guarded call -> (arena, rc), synchronised."""
    pas, kind, N, B, layout, _, _ = case
    lib = capi.lib()
    d = dict(full)
    if (layout & 0xff) == DIAG:
        d["P"] = torch.diagonal(d["P"], dim1=1, dim2=2).contiguous()
    if pas != F:
        d["x"] = torch.from_numpy(np.ascontiguousarray(x))
    worklist = lib.dqq_workspace_bytes(B)
    scratch = lib.dqq_scratch_bytes(KIND[kind], pas, N, B, layout)
    # one workgroup's scratch slice: what a one-problem call (a grid of one, general_any.hip any_grid) asks for
    piece = lib.dqq_scratch_bytes(KIND[kind], pas, N, 1, layout) if scratch else 0
    g, gd = case_g(case)
    a = Arena(call_specs(pas, kind, N, B, layout, d, worklist + scratch, worklist, piece), max(g, gd or 1), "cuda", sliced=sliced)
    try:
        rc = run_call(lib, a, pas, kind, N, B, layout, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    except RuntimeError as e:   # a device fault: nothing more is started on this GPU
        pytest.exit("%s: %s" % (case_id(case), e), returncode=3)
    return a, rc


def _footprint(capi, a, case, full):
    pas, kind, N, B, layout, _, _ = case
    a.check_guards()
    a.check_inputs()
    for name in (OUTPUTS[0] if pas == F else OUTPUTS[1][kind]):
        a.check_written(name)
    if pas == F:
        flags = a.view("diag_flags_out")
        assert bool((flags <= 2).all())
        a.check_written("pdiag_out", rows=flags == 1)
        kept = (flags == 1).cpu()
        diag = torch.diagonal(full["P"], dim1=1, dim2=2)
        assert torch.equal(a.view("pdiag_out").cpu()[kept], diag[kept]), "pdiag_out is not the diagonal of P"
        if not ((layout & 0xff) == 0 and N in (2, 4, 8, 16, 32, 64)):
            assert not bool(flags.any()), "flags of a call that does not examine P"
    ws = a.view("ws")
    head = ws[: 4 * ENTRIES].view(torch.int32)
    assert not bool(head.any()), "work-list header not zero again: word %d" % int(head.nonzero()[0, 0])
    assert not capi.workspace_status(ws)


def _outputs(a, case):
    pas, kind = case[0], case[1]
    names = OUTPUTS[0] if pas == F else OUTPUTS[1][kind]
    out = {n: a.view(n).clone() for n in names}
    if pas == F:
        pd = a.view("pdiag_out").clone()
        pd[a.view("diag_flags_out") != 1] = 0.0
        out["pdiag_out"] = pd
    return out


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_footprint(oracle, capi, case):
    pas, kind, N, B, layout, structure, route = case
    if B == 0:
        for sliced in (True, False):
            empty = {k: v[:0] for k, v in make_problem(kind, 1, N, 1, structure).items()}
            a, rc = _call(capi, case, empty, np.zeros((0, N, 1)), sliced)
            assert rc == 0
            a.check_untouched()
        return
    base, xo, rb = _reference(oracle, case)
    full, x = _tiled(base, B), tile(xo, B)
    a, rc = _call(capi, case, full, x, True)
    assert rc == 0
    _footprint(capi, a, case, full)
    got = _outputs(a, case)
    if pas == F:
        xh = npy(got["x"])
        err = np.abs(xh - x).max()
        print("%s: max |x - oracle| = %.3g" % (case_id(case), err))
        assert np.isfinite(xh).all() and err <= X_TOL
        it = npy(got["iters"])
        assert (it >= 0).all() and (it <= 1000).all()
    else:
        nout = 2 if kind == "qp" else 4
        names = OUTPUTS[1][kind]
        grads = [npy(got[n]) for n in names[:nout]]
        duals = None if kind == "qp" else (npy(got["gamma"]), npy(got["dgamma"]))
        steps = npy(got["ir_steps"])
        ref = ([tile(r, B) for r in rb[0]], tile(rb[1], B), None if rb[2] is None else tuple(tile(r, B) for r in rb[2]))
        if (layout & 0xff) == DIAG:
            ref = ([np.ascontiguousarray(np.diagonal(ref[0][0], axis1=1, axis2=2))] + ref[0][1:],) + ref[1:]
        Pb = base["P"].numpy()
        diag = tile((Pb == Pb * np.eye(N)).all(axis=(1, 2)), B)
        fam_diag, fam_other = _families(route)
        _check_rows(oracle, kind, full, x, grads, steps, duals, ref, fam_diag, diag, 1e-10, min_same=0.0)
        _check_rows(oracle, kind, full, x, grads, steps, duals, ref, fam_other, ~diag, 1e-10, min_same=0.0)
    # the same call on unsliced payloads: results are a function of the arguments, not of where the buffers lie
    b, rc = _call(capi, case, full, x, False)
    assert rc == 0
    _footprint(capi, b, case, full)
    for name, t in _outputs(b, case).items():
        same = torch.equal(t.view(torch.int64) if t.dtype == torch.float64 else t,
                           got[name].view(torch.int64) if t.dtype == torch.float64 else got[name])
        assert same, "'%s' differs between the sliced and the unsliced call" % name


@pytest.mark.parametrize("kind", ["qp", "qcqp"])
@pytest.mark.parametrize("B", [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 255, 257])
def test_forward_guard_band_through_the_python_layer(oracle, kind, B):
    """The guard-band lines of tests/test_gpu_parity.py:test_ragged_and_empty_batches, taken over as they are."""
    from diffqcqp_amd import ops
    N = 8
    d = make_problem(kind, B, N, 300 + B)
    g = {k: v.cuda() for k, v in d.items()}
    # guard bands: the kernels must not write past the batch
    xbuf = torch.full((B + 4, N, 1), 7.0, dtype=torch.float64, device="cuda")
    xo, ito = oracle_fwd(oracle, kind, d)
    if kind == "qp":
        ops.qp_forward(g["P"], g["q"], 1e-7, 1000, out=xbuf[:B])
    else:
        ops.qcqp_forward(g["P"], g["q"], g["l_n"], g["mu"], 1e-7, 1000, out=xbuf[:B])
    assert (xbuf[B:] == 7.0).all()
    assert np.abs(npy(xbuf[:B]) - xo).max() <= X_TOL
