"""-m gpu: addressing past 2^32 bytes for the entries added since the offsets matrix -- dqq_polish_ls_f64, dqq_polish_smooth_f64,
dqq_polish_path_f64, dqq_newton_bwd_smooth_f64, dqq_newton_jvp_smooth_f64, dqq_equilibrate_f64 and dqq_unscale_f64 -- on
tests/test_gpu_newton_offsets.py's method with tests/offset_cases.py's helpers.  What is under test is index arithmetic:
DiagTile::co / cc (diag_tile.h), polish_tile_store's b, the teams' prob * N * N, and the grid-stride loop of equil.hip's flat
kernels behind kEquilMaxGrid = 2^20 workgroups, which no other test enters.

Per row a base of nb problems (trip_cases.base_size: prime) is tiled on the device to B = ceil(2^29 / doubles per problem) +
2 nb + 1 problems: two whole replicas lie above the mark and the batch ends ragged.  ONE call, every output pre-filled with a
sentinel.  Then replica 0 is bit-equal to the host core (the equilibration: to the numpy restatement), every problem b is bit-equal
to problem b mod nb in every output, and no sentinel is left in the last whole replica and the ragged tail.  A row skips only when
the card has less free memory than it needs; a device fault ends the session.

Rows: each of the five Newton-family entries once at V32 (DQQ_P_DIAG, N = 64: every (B,N) buffer of the call past 2^32 bytes) and
once at M32 (the teams at N = 8, DQQ_P_DENSE: P -- and grad_P, dP -- past 2^32 bytes), the kinds rotating so that each appears at
least twice; polishes of at most 4 steps, the path on the two stages (1e-2, 2), (0, 2).  The equilibration: box, N = 8, dense at
M32 (equil_kernel), and box, N = 64, compact at V32, where dqq_unscale_f64 then runs over the e the call wrote: 2^28 + (2 nb + 1) 32
pairs of coordinates and twice as many elements, both more than kEquilMaxGrid * 256 threads -- asserted --, so the last threads of
equil_diag_kernel and every thread of unscale_kernel make a second pass of their loop.

TIMES -- the call under test on an MI355X, seconds (one launch and its synchronisation), rows in ROWS' order, V32 then M32:
    polish_ls 0.029 0.031   polish_smooth 0.055 0.031   polish_path 0.046 0.028   bwd_smooth 0.009 0.009   jvp_smooth 0.006 0.008
    equilibrate  M32 0.004   V32 0.008   unscale at V32 0.002
No row comes near 2 s, none was given fewer steps.  The whole file takes 10 s, most of it tiling inputs and comparing outputs;
its peak device memory is 46.3 GiB (the compact equilibration row with the unscale; the smoothed backward at V32: 44.4 GiB)."""
import ctypes
import time

import numpy as np
import pytest
import torch

import equil_ref as ER
import path_cases as PA
import polish_ls_cases as LC
import polish_reference as R
import smooth_cases as SC
from offset_cases import M32, V32, batch, count_equal_bits, first_unequal_replica, per_problem
from trip_cases import base_size

pytestmark = pytest.mark.gpu
DENSE, DIAG = 1, 2
SENTINEL_BITS = 0x7FF8DEADBEEF0001        # a NaN no kernel produces
SENTINEL_INT = -999                       # no step count, status or halving count, and no exponent (equil_core.h: |e| <= 255)
MARGIN = 2 << 30
KAPPA, H, MAX_STEPS = 1e-2, 8, 4
SCHEDULE = ((1e-2, 0.0), (2, 2))
K_EQUIL_MAX_GRID, K_EQUIL_BLOCK = 1 << 20, 256          # equil.hip
V, M = (64, DIAG, "diag", V32), (8, DENSE, "dense", M32)
# (entry, kind, N, layout, structure, mark)
ROWS = [(e, k) + size for e, kinds in (("polish_ls", ("qp", "qcqp")), ("polish_smooth", ("box", "sbox")), ("polish_path", ("qcqp", "qp")),
                                        ("bwd_smooth", ("sbox", "box")), ("jvp_smooth", ("qcqp", "sbox")))
        for k, size in zip(kinds, (V, M))]
EQUIL_ROWS = [("box",) + M, ("box",) + V]


def test_rows_are_what_the_matrix_asks_for():
    assert len(ROWS) == 10 and {r[0] for r in ROWS} == {"polish_ls", "polish_smooth", "polish_path", "bwd_smooth", "jvp_smooth"}
    for entry in {r[0] for r in ROWS}:
        assert sorted(r[5] == V32 and r[3] == DIAG for r in ROWS if r[0] == entry) == [False, True]
    assert all(sum(r[1] == k for r in ROWS) >= 2 for k in LC.KINDS)
    assert MAX_STEPS <= 4 and sum(SCHEDULE[1]) <= 4


def sentinel(shape, dtype=torch.float64):
    if dtype is torch.int32:
        return torch.full(shape, SENTINEL_INT, dtype=torch.int32, device="cuda")
    return torch.full(shape, SENTINEL_BITS, dtype=torch.int64, device="cuda").view(torch.float64)


def cu(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def need_memory(nbytes):
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    free = torch.cuda.mem_get_info()[0]
    if free < nbytes + MARGIN:
        pytest.skip("needs %.2f GiB of device memory, %.2f GiB are free" % ((nbytes + MARGIN) / 2 ** 30, free / 2 ** 30))


def timed(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = call()
    torch.cuda.synchronize()
    return rc, time.perf_counter() - t0


def check_outputs(out, ref, B, nb, pp, same):
    """out: name -> (B, ...) device tensor; ref: name -> replica 0's yardstick."""
    key, first = torch.arange(B, device="cuda") % nb, torch.arange(nb, device="cuda")
    for name, t in out.items():
        got = t[:nb].cpu().numpy()
        want = ref[name]
        assert got.dtype == want.dtype, name
        assert np.array_equal(got.reshape(want.shape), want) if want.dtype == np.int32 else same(got.reshape(want.shape), want), name
        bad = first_unequal_replica(t, key, first)
        assert bad is None, "%s of problem %d (base problem %d, from double %d on) differs from replica 0; %d problems differ" % (
            name, bad[0], bad[0] % nb, bad[0] * pp, bad[1])
        left = count_equal_bits(t, B - B % nb - nb, SENTINEL_BITS if t.dtype == torch.float64 else SENTINEL_INT)
        assert left == 0, "%d entries of %s above problem %d were not written" % (left, name, B - B % nb - nb)


@pytest.mark.parametrize("entry,kind,N,layout,structure,mark", ROWS, ids=lambda v: str(v))
def test_addresses_past_the_mark(entry, kind, N, layout, structure, mark):
    try:
        _run(entry, kind, N, layout, structure, mark)
    except torch.cuda.OutOfMemoryError:
        raise
    except RuntimeError as e:   # a device fault: nothing more is started on this GPU
        pytest.exit("newer offsets %s %s N=%d: %s" % (entry, kind, N, e), returncode=3)


def _run(entry, kind, N, layout, structure, mark):
    from diffqcqp_amd import _capi, build
    build.build()
    lib = _capi.lib()
    nb, B = base_size(N), batch(N, mark, layout)
    pp, ne, diag = per_problem(N, layout), (0 if kind == "qp" else N // 2 if kind == "qcqp" else N), layout == DIAG
    assert B * pp * 8 > 1 << 32 and B - -(-mark // pp) >= 2 * nb
    need_memory(B * 8 * (3 * pp + 8 * N + 4 * ne + 16))
    # the base, the host core's answers
    P, q, ex, x = LC.problem(kind, N, nb, structure)
    Pa = LC.compact(P) if diag else P
    k, S = R.KIND[kind], len(SCHEDULE[0])
    f64, i32 = torch.float64, torch.int32
    if entry.startswith("polish"):
        if entry == "polish_ls":
            h = LC.host_polish_ls(kind, Pa, q, ex, x, MAX_STEPS, H, 0.0, diag=diag)
        elif entry == "polish_smooth":
            h = SC.host_polish(kind, Pa, q, ex, x, MAX_STEPS, H, 0.0, KAPPA, diag=diag)
        else:
            h = PA.host_path(kind, Pa, q, ex, x, SCHEDULE[0], SCHEDULE[1], H, 0.0, diag=diag)
        names = ("x_out", "resid", "steps", "status", "halvings", "stage_resid", "stage_steps")
        ref = dict(zip(names, h))
        assert (ref["status"] == 0).sum() >= nb // 2 and not (ref["status"] == 2).any()
        small = [Pa, q, *ex, x]
        shapes = {"x_out": ((B, N), f64), "resid": ((B, 2), f64), "steps": ((B,), i32), "status": ((B,), i32), "halvings": ((B,), i32),
                  "stage_resid": ((B, S, 2), f64), "stage_steps": ((B, S), i32)}
    else:
        x = SC.host_polish(kind, Pa, q, ex, x, SC.MAX_STEPS, H, 0.0, KAPPA, diag=diag)[0]     # the derivatives at the smoothed polish's point
        dP, dq, da, db, gx = SC.tangents(kind, N, nb, structure)
        dPa = SC.compact(dP) if diag else dP
        if entry == "bwd_smooth":
            h = SC.host_backward(kind, Pa, q, ex, x, gx, 0.0, KAPPA, diag=diag)
            ref = {n: v for n, v in zip(("grad_P", "grad_q", "grad_a", "grad_b", "status"), h) if v is not None}
            small = [Pa, q, *ex, x, gx]
            shapes = {"grad_P": (((B, N) if diag else (B, N, N)), f64), "grad_q": ((B, N), f64), "grad_a": ((B, ne), f64),
                      "grad_b": ((B, ne), f64), "status": ((B,), i32)}
        else:
            h = SC.host_jvp(kind, Pa, q, ex, x, dPa, dq, da, db, 0.0, KAPPA, diag=diag)
            ref = {"dx": h[0], "status": h[1]}
            small = [Pa, q, *ex, x, dPa, dq] + ([da, db] if ne else [])
            shapes = {"dx": ((B, N), f64), "status": ((B,), i32)}
        assert not ref["status"].any()
    idx = torch.arange(B, device="cuda") % nb
    big = [cu(a).index_select(0, idx) for a in small]
    del idx
    out = {n: sentinel(*shapes[n]) for n in ref}
    nex = len(ex)
    head = [k] + [ptr(t) for t in big[:2 + nex]] + [None] * (3 - nex) + [ptr(big[2 + nex])]
    rest = [ptr(t) for t in big[3 + nex:]]
    o = lambda n: ptr(out.get(n))   # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    tail = (o("resid"), o("steps"), o("status"), o("halvings"))
    if entry == "polish_ls":
        call = lambda: lib.dqq_polish_ls_f64(*head, o("x_out"), B, N, MAX_STEPS, layout, 0.0, H, *tail, None, 0, stream)   # noqa: E731
    elif entry == "polish_smooth":
        call = lambda: lib.dqq_polish_smooth_f64(*head, o("x_out"), B, N, MAX_STEPS, layout, 0.0, KAPPA, H, *tail, None, 0, stream)   # noqa: E731
    elif entry == "polish_path":
        ks, ns = (ctypes.c_double * S)(*SCHEDULE[0]), (ctypes.c_int * S)(*SCHEDULE[1])
        call = lambda: lib.dqq_polish_path_f64(*head, o("x_out"), B, N, layout, 0.0, ctypes.addressof(ks), ctypes.addressof(ns), S, H,   # noqa: E731
                                               *tail, o("stage_resid"), o("stage_steps"), None, 0, stream)
    elif entry == "bwd_smooth":
        call = lambda: lib.dqq_newton_bwd_smooth_f64(*head, *rest, o("grad_P"), o("grad_q"), o("grad_a"), o("grad_b"), B, N, layout, 0.0,   # noqa: E731
                                                     KAPPA, o("status"), None, 0, stream)
    else:
        call = lambda: lib.dqq_newton_jvp_smooth_f64(*head, *rest, *([None, None] if not ne else []), o("dx"), B, N, layout, 0.0, KAPPA,   # noqa: E731
                                                     o("status"), None, 0, stream)
    rc, seconds = timed(call)
    _capi.check(rc, entry)
    check_outputs(out, ref, B, nb, pp, SC.same_bits)
    print("%s %s N=%d layout %d: B %d, the call %.3f s, peak %.2f GiB" % (entry, kind, N, layout, B, seconds,
                                                                         torch.cuda.max_memory_allocated() / 2 ** 30))
    del big, out
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kind,N,layout,structure,mark", EQUIL_ROWS, ids=lambda v: str(v))
def test_equilibration_past_the_mark(kind, N, layout, structure, mark):
    try:
        _run_equil(kind, N, layout, mark)
    except torch.cuda.OutOfMemoryError:
        raise
    except RuntimeError as e:   # a device fault: nothing more is started on this GPU
        pytest.exit("newer offsets equilibrate %s N=%d: %s" % (kind, N, e), returncode=3)


def _run_equil(kind, N, layout, mark):
    from diffqcqp_amd import _capi, build
    build.build()
    lib = _capi.lib()
    nb, B = base_size(N), batch(N, mark, layout)
    pp, diag = per_problem(N, layout), layout == DIAG
    assert B * pp * 8 > 1 << 32 and B - -(-mark // pp) >= 2 * nb
    if diag:    # the flat kernels' threads loop: a thread per pair of coordinates / per element, at most kEquilMaxGrid workgroups
        assert B * (N // 2) == (1 << 28) + (2 * nb + 1) * 32 > K_EQUIL_MAX_GRID * K_EQUIL_BLOCK and B * N > K_EQUIL_MAX_GRID * K_EQUIL_BLOCK
    need_memory(B * (8 * (2 * pp + 10 * N) + 4 * N + 16))
    P, q, extras, x0 = ER.make_batch(kind, nb, N, 52000 + N, diag)
    want = ER.equilibrate(kind, P, q, extras, x0, diag)
    ref = {"P": want[0], "q": want[1], "a": want[2][0], "b": want[2][1], "x0": want[3], "e": want[4]}
    idx = torch.arange(B, device="cuda") % nb
    big = [cu(a).index_select(0, idx) for a in (P, q, *extras, x0)]
    del idx
    out = {n: sentinel(tuple(t.shape)) for n, t in zip(("P", "q", "a", "b", "x0"), big)}
    out["e"] = sentinel((B, N), torch.int32)
    stream = torch.cuda.current_stream().cuda_stream
    rc, seconds = timed(lambda: lib.dqq_equilibrate_f64(R.KIND[kind], *[t.data_ptr() for t in big[:4]], None, big[4].data_ptr(), B, N, layout,
                                                        out["P"].data_ptr(), out["q"].data_ptr(), out["a"].data_ptr(), out["b"].data_ptr(),
                                                        None, out["x0"].data_ptr(), out["e"].data_ptr(), stream))
    _capi.check(rc, "dqq_equilibrate_f64")
    check_outputs(out, ref, B, nb, pp, ER.same_bits)
    print("equilibrate %s N=%d layout %d: B %d, the call %.3f s, peak %.2f GiB" % (kind, N, layout, B, seconds,
                                                                                  torch.cuda.max_memory_allocated() / 2 ** 30))
    if diag:    # dqq_unscale_f64 over the same e, y the batch's q
        xo = {"x": sentinel((B, N))}
        rc, seconds = timed(lambda: lib.dqq_unscale_f64(big[1].data_ptr(), out["e"].data_ptr(), B, N, xo["x"].data_ptr(), stream))
        _capi.check(rc, "dqq_unscale_f64")
        check_outputs(xo, {"x": ER.unscale(q, want[4])}, B, nb, pp, ER.same_bits)
        print("unscale N=%d: %d elements, the call %.3f s, peak %.2f GiB" % (N, B * N, seconds, torch.cuda.max_memory_allocated() / 2 ** 30))
    del big, out
    torch.cuda.empty_cache()
