"""-m gpu: every persistent general-P kernel past its first trip through the batch (rows and inputs: tests/trip_cases.py, held
against the launch geometry on the CPU by tests/test_trip_cases.py).

The general kernels run a fixed grid of workgroups, waves or teams over the batch or the work-list, and a worker keeps its
per-problem state -- LDS slices, its slice of the scratch, registers -- where it found it; only the routine's own
re-initialisation and barriers separate one problem from the next.  Each row's batch is the base batch tiled to at least two
full trips of every worker and a ragged third.  Per row, the hint feedback off:
  1. against the oracle on every problem: check_forward at 1e-6 and equal iteration counts on >= 0.999 (N <= 16) / 0.99
     (beyond: tests/test_gpu_warm.py); the backward on the oracle's x, check_backward_exact(exact=False) -- every row's kernel
     is a reference-order one;
  2. trip independence: the call on the base alone (at most one trip, the same kernels; trip_cases.one_trip_size) and on
     all B problems -- x and iters, every gradient, ir_steps and the duals of problem b are the bits of base problem b mod base;
  3. poison: NaN in q (backward: in x) of problem 1 and P[0,0] = inf in problem 4, both in every worker's first trip: those two
     come back non-finite, every other problem keeps the bits of (2), the launch returns (forwards at max_iter = 200);
  4. forwards at max_iter = 3: the bits of the tiled base at max_iter = 3, no count above 3.
A difference in (2)-(4) names the first problem that differs and the trip it was solved on."""
import time

import numpy as np
import pytest
import torch

from param_cases import tile
from test_gpu_parity import check_backward_exact, check_forward
from test_gpu_parameters import _hfwd
from trip_cases import ROWS, Bw, F, base_size, one_trip_size, reference, row_id, tiled

pytestmark = pytest.mark.gpu
POISON_NAN, POISON_INF = 1, 4     # both dense problems of the base, both below every row's per_trip
CAP = 200                         # max_iter of the forwards of (2) and (3): a NaN problem runs to the cap


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


def _forward(ops, row, g, max_iter):
    x, it = _hfwd(ops, row[1], g, row[4], 1e-7, max_iter)
    return {"x": x, "iters": it}


def _backward(ops, row, g, x):
    kind, N, layout = row[1], row[2], row[4]
    B = g["q"].shape[0]
    if kind == "qp":
        gP, gq, st = ops.qp_backward(g["P"], g["q"], x, g["grad_x"], layout=layout, return_steps=True)
        return {"grad_P": gP, "grad_q": gq, "ir_steps": st}
    shape = (B, N // 2, 1) if kind == "qcqp" else (B, 2 * N)
    du = (torch.empty(shape, dtype=torch.float64, device="cuda"), torch.empty(shape, dtype=torch.float64, device="cuda"))
    if kind == "qcqp":
        out = ops.qcqp_backward(g["P"], g["q"], g["l_n"], g["mu"], x, g["grad_x"], layout=layout, return_steps=True, duals=du)
    else:
        out = ops.boxqp_backward(g["P"], g["q"], g["l_min"], g["l_max"], x, g["grad_x"], layout=layout, return_steps=True,
                                 duals=du, v=g.get("v"))
    return {"grad_P": out[0], "grad_q": out[1], "grad_3": out[2], "grad_4": out[3], "ir_steps": out[4], "gamma": du[0],
            "dgamma": du[1]}


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same_bits(row, what, full, base_out, keep=None):
    """Every output of problem b of `full` is base problem b mod base of `base_out`, bit for bit (on the problems `keep`)."""
    B, nb, per = row[3], base_size(row[2]), row[7]
    for name, t in full.items():
        want = base_out[name][:nb]
        want = want.repeat((-(-B // nb),) + (1,) * (want.dim() - 1))[:B]
        diff = (_bits(t) != _bits(want)).reshape(B, -1).any(1)
        if keep is not None:
            diff &= keep
        if bool(diff.any()):
            b = int(torch.nonzero(diff)[0, 0])
            raise AssertionError("%s, %s: %s differs from the one-trip call on %d of %d problems, first on problem %d (base "
                                 "problem %d; entry %d of a direct launch is solved on trip %d of its worker)"
                                 % (row_id(row), what, name, int(diff.sum()), B, b, b % nb, b, b // per))


def _nonfinite(out, b):
    return any(not bool(torch.isfinite(t[b].double()).all()) for name, t in out.items() if name not in ("iters", "ir_steps"))


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_every_worker_solves_its_later_problems_as_its_first(ops, row):
    pas, kind, N, B, layout = row[:5]
    t0 = time.perf_counter()
    ref = reference(row)                                   # the oracle on the base, once
    nb = base_size(N)
    base = {k: v.cuda() for k, v in ref["base"].items()}
    full = tiled(base, B)
    base = tiled(base, one_trip_size(row))                 # the base (a work-list row: with its last tile completed)
    assert B >= 2 * row[7] + 1 and POISON_INF < row[7] and nb > POISON_INF
    torch.cuda.synchronize()
    t1 = time.perf_counter()

    if pas == F:
        # (1) the oracle, every problem
        out = _forward(ops, row, full, 1000)
        check_forward(out["x"], out["iters"], tile(ref["x"], B), tile(ref["iters"], B), min_match=0.999 if N <= 16 else 0.99)
        run = lambda g, max_iter: _forward(ops, row, g, max_iter)
        caps = (CAP, 3)
    else:
        xb = torch.from_numpy(ref["x"]).cuda()
        base["x"] = tiled({"q": xb}, one_trip_size(row))["q"]
        full["x"] = tiled({"q": xb}, B)["q"]
        out = _backward(ops, row, full, full["x"])
        grads = [out[n] for n in ("grad_P", "grad_q", "grad_3", "grad_4") if n in out]
        check_backward_exact(grads, out["ir_steps"], tuple(tile(a, B) for a in ref["grads"]) + (tile(ref["steps"], B),),
                             exact=False)
        run = lambda g, max_iter: _backward(ops, row, g, g["x"])
        caps = (None,)

    # (2) trip independence, bit for bit
    one = run(base, caps[0])
    many = run(full, caps[0])
    torch.cuda.synchronize()
    _same_bits(row, "all B problems", many, one)
    if pas == F:
        assert int(many["iters"].max()) <= CAP and int(one["iters"].max()) < CAP   # (no problem of the base runs to the cap)

    # (3) poison in the first trip does not ride to the second and third
    bad = {k: v.clone() for k, v in full.items()}
    bad["x" if pas == Bw else "q"][POISON_NAN, N // 2, 0] = float("nan")
    bad["P"][POISON_INF, 0, 0] = float("inf")
    poisoned = run(bad, caps[0])
    torch.cuda.synchronize()                                # the launch returns
    keep = torch.ones(B, dtype=torch.bool, device="cuda")
    keep[[POISON_NAN, POISON_INF]] = False
    _same_bits(row, "beside a NaN and an inf problem", poisoned, one, keep)
    for b in (POISON_NAN, POISON_INF):
        assert _nonfinite(poisoned, b), "%s: poisoned problem %d came back finite" % (row_id(row), b)
    if pas == F:
        assert int(poisoned["iters"].max()) <= CAP

    # (4) a capped problem before a quick one
    if pas == F:
        one3 = run(base, 3)
        many3 = run(full, 3)
        torch.cuda.synchronize()
        _same_bits(row, "max_iter = 3", many3, one3)
        assert int(many3["iters"].max()) <= 3 and int(many3["iters"].min()) >= 1
        assert int(one["iters"].max()) > 3                  # (the cap bites)
    t2 = time.perf_counter()
    print("%s: per_trip %d (%s), B %d: oracle and inputs %.2f s, device steps and checks %.2f s"
          % (row_id(row), row[7], row[8], B, t1 - t0, t2 - t1))
