"""-m gpu: every launch family's addressing past 2^32 bytes and 2^31 (forwards: 2^32) elements of P and grad_P -- dP on the JVP's
rows; on the compact-layout rows past 2^32 bytes of every (B,N) buffer of the call -- (rows: tests/offset_cases.py, held to
account on the CPU by tests/test_offset_cases.py).

Per row the base batch -- make_problem's data, 61 or 37 problems -- is solved by the oracle on the CPU and tiled on the device to
the row's B (one index_select per tensor).  ONE call of the op under test, every output it can write pre-filled with a
sentinel.  Then:
  1. the reference problems -- the first nb of the batch; behind a work-list also the first occurrence of each base problem in
     the other kernel of the route (offset_cases.replica_keys) -- meet the bar of the test named beside the row: forward
     check_forward (X_TOL, equal iteration counts on _min_match), warm forward tests/test_gpu_warm.py's _check against the numpy
     restatement, backward _check_rows at min_same = 0 as tests/test_gpu_footprint.py holds its small batches, the solution
     check, the JVP (tangents tiled like the inputs) and the polish (polish_cases' own base and start, tiled) bit for bit
     against their host-compiled cores, step counts and status words included;
  2. every problem of the batch is bit-equal to its reference problem in every output (a problem's result does not depend on
     its neighbours or its position: tests/test_gpu_parity.py, tests/test_gpu_trips.py) -- compared on the device in chunks;
  3. no sentinel is left in the last whole replica and the ragged tail of any pre-filled output.
An address that wraps reads another problem's P or leaves a gradient above the mark unwritten: (2) or (3) names the problem.
A row skips only when the card has less free memory than the row needs; the reason states both numbers."""
import time

import numpy as np
import pytest
import torch

import check_ref as R
import jvp_cases as JC
import jvp_reference as JR
import polish_cases as PC
import warm_reference as WR
from conftest import make_problem
from offset_cases import (ROWS, C, J, Pl, W, compact, count_equal_bits, first_unequal_replica, mark_name, per_problem, replica_keys,
                          row_id, row_seed)
from param_cases import KIND, F, Bw
from test_gpu_parameters import REASSOCIATING, _check_rows, _families, _min_match
from test_gpu_parity import check_forward, npy
from test_gpu_warm import _check as check_warm, _min_match as warm_min_match
from trip_cases import _obwd, _ofwd, base_size
from warm_cases import EPS, MAX_ITER, PERTURB, extras_of, well_conditioned

pytestmark = pytest.mark.gpu
SENTINEL_BITS = 0x7FF8DEADBEEF0001        # a NaN no kernel produces
SENTINEL_INT = -7                         # no step count, no status word
MARGIN = 2 << 30
EXTRAS = {"qp": (), "qcqp": ("l_n", "mu"), "box": ("l_min", "l_max"), "sbox": ("l_min", "l_max", "v")}
PEAK = [0]


@pytest.fixture(scope="module")
def ops():
    """The shipped library, the hint feedback off: the route of a call is then a function of its arguments alone."""
    assert torch.cuda.is_available(), "these tests need the GPU"
    from diffqcqp_amd import build, ops as _ops, _capi
    build.build()
    _capi.lib()
    was_on = _capi._feedback is not None
    _capi.enable_feedback(False)
    yield _ops
    _capi.enable_feedback(was_on)
    print("peak device memory of tests/test_gpu_offsets.py: %.2f GiB" % (PEAK[0] / 2 ** 30))


def need_bytes(ops, row):
    """Inputs, outputs, the tiling index and the replica keys, the workspace, and 2 GiB of margin (comparison chunks)."""
    pas, kind, N, B, layout = row[:5]
    per_contact = kind == "qcqp"
    ex = len(EXTRAS[kind]) * 8 * (N // 2 if per_contact else N)
    pp = 8 * per_problem(N, layout)                               # P: (N,N), or (N) on the compact layout
    per = pp + 8 * N + ex + 2 * 8 + 1                             # P, q, extras; index and key (int64), queued (bool)
    if pas == J:                                                  # x, dx, ir_steps; the tangents of P, q and two extras
        return B * (per + 2 * 8 * N + 8 + pp + 8 * N + 2 * 8 * (N // 2 if per_contact else N)) + (8 << 30) + MARGIN
    if pas == Pl:                                                 # x, x_out, resid, steps, status; PolishAny's scratch
        return B * (per + 2 * 8 * N + 16 + 8) + (1 << 30) + MARGIN
    if pas == F:
        per += 8 * N + 4
    elif pas == W:
        per += 2 * 8 * N + 4
    elif pas == C:
        per += 8 * N + 4 + 32 + 4
    else:
        dual = 0 if kind == "qp" else 2 * 8 * (N // 2 if per_contact else 2 * N)
        grads = 0 if kind == "qp" else 2 * 8 * (N // 2 if per_contact else N)
        per += 2 * 8 * N + pp + 8 * N + grads + dual + 8
    ws = 0 if pas == C else max(4096, ops.workspace_bytes(B, 2 if (pas == Bw and kind == "sbox") else KIND[kind],
                                                           1 if pas == Bw else 0, N, layout))
    return B * per + ws + MARGIN


def sentinel(shape):
    return torch.full(shape, SENTINEL_BITS, dtype=torch.int64, device="cuda").view(torch.float64)


def sentinel_int(shape):
    return torch.full(shape, SENTINEL_INT, dtype=torch.int32, device="cuda")


def call_direct(ops, row, g):
    """dqq_jvp_f64 / dqq_polish_f64 straight through the C ABI: every output, the optional ones included, is pre-filled."""
    from diffqcqp_amd import _capi
    pas, kind, N, B, layout = row[:5]
    k = KIND[kind]
    ptr = lambda t: 0 if t is None else t.data_ptr()   # noqa: E731
    ex = [g[n] for n in EXTRAS[kind]] + [None] * (3 - len(EXTRAS[kind]))
    stream = torch.cuda.current_stream().cuda_stream
    dev = g["q"].device
    if pas == J:
        dx, steps = sentinel((B, N, 1)), sentinel_int((B, 2) if kind in ("box", "sbox") else (B,))
        ws = None
        if ops.workspace_bytes(B, min(k, 2), 1, N, layout | _capi.F_REFERENCE_ORDER) > ops.workspace_bytes(B) and not compact(row):
            ws = ops.make_workspace(dev, B, min(k, 2), 1, N, layout | _capi.F_REFERENCE_ORDER)
        tan = [g["dP"], g["dq"], g.get("da"), g.get("db")]
        rc = _capi.lib().dqq_jvp_f64(k, g["P"].data_ptr(), g["q"].data_ptr(), *map(ptr, ex), g["x"].data_ptr(), *map(ptr, tan),
                                     dx.data_ptr(), B, N, JC.EPSILON, layout, steps.data_ptr(), ptr(ws),
                                     ws.numel() * 4 if ws is not None else 0, stream)
        _capi.check(rc, "dqq_jvp_f64")
        return {"dx": dx, "ir_steps": steps, "_filled": ("dx", "ir_steps"), "_ws": ws}
    xo, resid = sentinel((B, N, 1)), sentinel((B, 2))
    steps, status = sentinel_int((B,)), sentinel_int((B,))
    ws = ops.polish_workspace(dev, k, N, B) if not compact(row) else None
    rc = _capi.lib().dqq_polish_f64(k, g["P"].data_ptr(), g["q"].data_ptr(), *map(ptr, ex), g["x"].data_ptr(), xo.data_ptr(), B, N,
                                    PC.MAX_STEPS, layout, resid.data_ptr(), steps.data_ptr(), status.data_ptr(), ptr(ws),
                                    ws.numel() * 4 if ws is not None else 0, stream)
    _capi.check(rc, "dqq_polish_f64")
    return {"x_out": xo, "resid": resid, "steps": steps, "status": status, "_filled": ("x_out", "resid", "steps", "status"), "_ws": ws}


def call(ops, row, g):
    """The one call under test -> {name: output tensor}, the pre-filled ones listed in out["_filled"]."""
    pas, kind, N, B, layout = row[:5]
    if pas in (J, Pl):
        return call_direct(ops, row, g)
    ex = [g[n] for n in EXTRAS[kind]]
    if pas in (F, W):
        x = sentinel((B, N, 1))
        kw = dict(layout=layout, return_iters=True, out=x)
        if pas == F:
            if kind == "qp":
                _, it = ops.qp_forward(g["P"], g["q"], 1e-7, 1000, **kw)
            elif kind == "qcqp":
                _, it = ops.qcqp_forward(g["P"], g["q"], *ex, 1e-7, 1000, **kw)
            else:
                _, it = ops.boxqp_forward(g["P"], g["q"], ex[0], ex[1], 1e-7, 1000, v=g.get("v"), **kw)
        elif kind == "qp":
            _, it = ops.qp_forward_warm(g["P"], g["q"], g["x0"], EPS, MAX_ITER, **kw)
        elif kind == "qcqp":
            _, it = ops.qcqp_forward_warm(g["P"], g["q"], *ex, g["x0"], EPS, MAX_ITER, **kw)
        else:
            _, it = ops.boxqp_forward_warm(g["P"], g["q"], ex[0], ex[1], g["x0"], EPS, MAX_ITER, v=g.get("v"), **kw)
        return {"x": x, "iters": it, "_filled": ("x",)}
    if pas == C:
        status = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        resid = sentinel((B, 4))
        counts = torch.zeros(3, dtype=torch.int64, device="cuda")
        ops.solution_check(kind, g["P"], g["q"], ex, g["x"], iters=g["iters"], max_iter=1000, layout=layout,
                           out=(status, resid, counts))
        return {"status": status, "resid": resid, "counts": counts, "_filled": ("resid",)}
    gP, gq = sentinel((B, N) if compact(row) else (B, N, N)), sentinel((B, N, 1))
    if kind == "qp":
        _, _, st = ops.qp_backward(g["P"], g["q"], g["x"], g["grad_x"], layout=layout, return_steps=True, out=(gP, gq))
        return {"grad_P": gP, "grad_q": gq, "ir_steps": st, "_filled": ("grad_P", "grad_q")}
    eshape = (B, N // 2, 1) if kind == "qcqp" else (B, N, 1)
    dshape = (B, N // 2, 1) if kind == "qcqp" else (B, 2 * N)
    ga, gb, gam, dgam = sentinel(eshape), sentinel(eshape), sentinel(dshape), sentinel(dshape)
    if kind == "qcqp":
        out = ops.qcqp_backward(g["P"], g["q"], *ex, g["x"], g["grad_x"], layout=layout, return_steps=True,
                                out=(gP, gq, ga, gb), duals=(gam, dgam))
    else:
        out = ops.boxqp_backward(g["P"], g["q"], ex[0], ex[1], g["x"], g["grad_x"], layout=layout, return_steps=True,
                                 out=(gP, gq, ga, gb), duals=(gam, dgam), v=g.get("v"))
    return {"grad_P": gP, "grad_q": gq, "grad_3": ga, "grad_4": gb, "gamma": gam, "dgamma": dgam, "ir_steps": out[4],
            "_filled": ("grad_P", "grad_q", "grad_3", "grad_4", "gamma", "dgamma")}


def reference_inputs(oracle, row):
    """-> (base: CPU tensors, with x / x0 / iters where the op takes them; ref: what the reference problems are held to)."""
    pas, kind, N = row[:3]
    nb = base_size(N)
    t = lambda a: torch.from_numpy(np.array(a, order="C"))   # noqa: E731
    if pas == Pl:
        d, x = PC.problem(kind, N, nb, row[5])
        base = {k: t(v) for k, v in d.items()}
        base["x"] = t(x)
        P, q, ex = PC.flat(d, kind)
        return base, PC.host_polish(kind, PC.compact(P) if compact(row) else P, q, ex, x[:, :, 0], diag=compact(row))
    base = make_problem(kind, nb, N, row_seed(row), row[5])
    if pas != Bw:
        base.pop("grad_x")
    if pas == W:
        base["P"] = well_conditioned(base["P"])
        P, q, ex = base["P"].numpy(), base["q"].numpy(), extras_of(kind, base)
        x0 = WR.perturbed_start(kind, P, q, ex, PERTURB[kind], row_seed(row))
        base["x0"] = torch.from_numpy(np.ascontiguousarray(x0))
        return base, WR.solve(kind, P, q, EPS, MAX_ITER, ex, x0=x0)
    a = {k: v.numpy() for k, v in base.items()}
    xo, ito = _ofwd(oracle, kind, a)
    if pas == F:
        return base, (xo, ito)
    base["x"] = torch.from_numpy(np.ascontiguousarray(xo))
    if pas == J:
        tan = JR.random_tangents(kind, nb, N, row_seed(row), diag=compact(row))
        base.update(dP=t(tan[0]), dq=t(tan[1][:, :, None]))
        if kind != "qp":
            base.update(da=t(tan[2][:, :, None]), db=t(tan[3][:, :, None]))
        return base, JC.host_jvp(kind, a, xo, tan)
    if pas == C:
        base["iters"] = torch.from_numpy(np.ascontiguousarray(ito.astype(np.int32)))
        ex = tuple(a[n][:, :, 0] for n in EXTRAS[kind])
        return base, R.host_check(R.hostcore(), kind, a["P"], a["q"][:, :, 0], ex, xo[:, :, 0], base["iters"].numpy(), 1000, False)
    return base, _obwd(oracle, kind, a, xo)


def check_reference_problems(oracle, row, base, ref, out, at, queued_at):
    """The problems `at` of the batch (numpy indices; queued_at: which of them the drain solved) against the oracle on base
    problem at mod nb, at the bar of row[8]."""
    pas, kind, N, route = row[0], row[1], row[2], row[6]
    nb = base_size(N)
    src = at % nb
    pick_t = lambda t: t[torch.from_numpy(at).cuda()]
    pick = lambda t: npy(pick_t(t))
    if pas == F:
        check_forward(pick_t(out["x"]), pick_t(out["iters"]), ref[0][src], ref[1][src], min_match=_min_match(N, route))
    elif pas == W:
        check_warm(pick_t(out["x"]), pick_t(out["iters"]), ref[0][src], ref[1][src], warm_min_match(N, route), row_id(row))
    elif pas == C:
        status, resid = ref
        assert np.array_equal(pick(out["status"]), status[src])
        assert R.same_bits(pick(out["resid"]), resid[src])
        B = out["status"].shape[0]
        want = [(B // nb) * int((status == k).sum()) + int((status[:B % nb] == k).sum()) for k in range(3)]
        assert out["counts"].tolist() == want and want[0] > 0, (out["counts"].tolist(), want)
    elif pas == J:
        dx, steps = ref
        assert np.array_equal(pick(out["ir_steps"]).reshape(len(at), -1), steps[src]), "refinement step counts differ"
        assert np.array_equal(pick(out["dx"])[:, :, 0].view(np.int64), np.ascontiguousarray(dx[src]).view(np.int64)), "dx differs"
        assert np.abs(dx).max() > 1e-3
    elif pas == Pl:
        xo, resid, steps, status = ref
        assert (status == 0).sum() >= nb // 4           # (not a comparison of untouched points)
        assert np.array_equal(pick(out["steps"]), steps[src]) and np.array_equal(pick(out["status"]), status[src])
        assert PC.same_bits(pick(out["x_out"])[:, :, 0], xo[src]) and PC.same_bits(pick(out["resid"]), resid[src])
    else:
        names = ("grad_P", "grad_q") if kind == "qp" else ("grad_P", "grad_q", "grad_3", "grad_4")
        grads = [pick(out[n]) for n in names]
        duals = None if kind == "qp" else (pick(out["gamma"]), pick(out["dgamma"]))
        rg, rst, rdu = ref
        refs = ([r[src] for r in rg], rst[src], None if rdu is None else tuple(r[src] for r in rdu))
        if compact(row):   # grad_P comes back as its diagonal (tests/test_gpu_footprint.py holds DQQ_P_DIAG cases the same way)
            refs = ([np.ascontiguousarray(np.diagonal(refs[0][0], axis1=1, axis2=2))] + refs[0][1:],) + refs[1:]
        d = {k: v[torch.from_numpy(src)] for k, v in base.items() if k != "x"}
        x = base["x"].numpy()[src]
        fam_fast, fam_drain = _families(route)
        Pb = base["P"].numpy()[src]
        diag = (Pb == Pb * np.eye(N)).all(axis=(1, 2))
        # a re-associating drain gives a diagonal problem of a queued tile its own bits, a reference-order one the fast
        # kernel's (tests/test_gpu_footprint.py holds those to the fast kernel's bar, and so does this)
        fast = ~queued_at if (fam_drain in REASSOCIATING and queued_at is not None) else diag
        _check_rows(oracle, kind, d, x, grads, pick(out["ir_steps"]), duals, refs, fam_fast, fast, 1e-10, min_same=0.0)
        _check_rows(oracle, kind, d, x, grads, pick(out["ir_steps"]), duals, refs, fam_drain, ~fast, 1e-10, min_same=0.0)


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_addresses_past_the_mark(oracle, ops, row):
    try:
        _run_row(oracle, ops, row)
    except torch.cuda.OutOfMemoryError:
        raise
    except RuntimeError as e:   # a device fault: nothing more is started on this GPU
        pytest.exit("%s: %s" % (row_id(row), e), returncode=3)


def _run_row(oracle, ops, row):
    pas, kind, N, B, layout = row[:5]
    nb = base_size(N)
    torch.cuda.empty_cache()
    need, free = need_bytes(ops, row), torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip("%s needs %.2f GiB of device memory, %.2f GiB are free" % (row_id(row), need / 2 ** 30, free / 2 ** 30))
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    base, ref = reference_inputs(oracle, row)
    t1 = time.perf_counter()
    idx = torch.arange(B, device="cuda") % nb
    small = dict(base)
    if compact(row):   # P -- and the JVP's dP -- go in as their diagonals (B,N)
        for k in ("P", "dP"):
            if k in small:
                small[k] = torch.diagonal(small[k], dim1=1, dim2=2).contiguous()
    g = {k: v.cuda().index_select(0, idx) for k, v in small.items()}
    del idx
    key, first, queued = replica_keys(row, B, "cuda")
    torch.cuda.synchronize()
    t2 = time.perf_counter()

    out = call(ops, row, g)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    filled = out.pop("_filled")
    out.pop("_ws", None)

    # (1) the reference problems against the oracle
    at = first[first < B].cpu().numpy()
    assert len(at) >= nb and set((at % nb).tolist()) == set(range(nb)) and (at < 2 * 64 * nb).all()
    check_reference_problems(oracle, row, base, ref, out, at, None if queued is None else queued[torch.from_numpy(at).cuda()].cpu().numpy())
    # (2) every problem of the batch: the bits of its reference problem
    for name, t in out.items():
        if name == "counts":   # (held to the host core's statuses in (1))
            continue
        bad = first_unequal_replica(t, key, first)
        assert bad is None, ("%s: %s of problem %d (base problem %d, P from double %d on, mark %s) differs from problem %d; %d "
                             "problems differ" % (row_id(row), name, bad[0], bad[0] % nb, bad[0] * per_problem(N, layout), mark_name(row),
                                                  int(first[key[bad[0]]]), bad[1]))
    # (3) written by this call: the last whole replica and the ragged tail
    for name in filled:
        left = count_equal_bits(out[name], B - B % nb - nb, SENTINEL_BITS if out[name].dtype == torch.float64 else SENTINEL_INT)
        assert left == 0, "%s: %d entries of %s above problem %d were not written" % (row_id(row), left, name, B - B % nb - nb)
    t4 = time.perf_counter()
    peak = torch.cuda.max_memory_allocated()
    PEAK[0] = max(PEAK[0], peak)
    print("%s: B %d, oracle %.2f s, tiling %.2f s, the call %.3f s, comparisons %.2f s; needs %.2f GiB, peak %.2f GiB"
          % (row_id(row), B, t1 - t0, t2 - t1, t3 - t2, t4 - t3, need / 2 ** 30, peak / 2 ** 30))
    del g, out, key, first, queued
    torch.cuda.empty_cache()
