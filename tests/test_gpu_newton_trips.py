"""-m gpu: every persistent dense kernel of the Newton family past its first trip through the batch (rows and inputs:
tests/newton_trip_cases.py, held against the routes, the launch geometry and the host cores on the CPU by
tests/test_newton_trip_cases.py).

The dense routes of dqq_polish[_reg|_ls]_f64, dqq_newton_{bwd,jvp}[_reg]_f64, dqq_newton_jac[_reg]_f64 and dqq_newton_active_f64
run a fixed grid over the batch: a team keeps its slice (LDS, or the caller's scratch) and its registers where it found them, and
only the routine's own re-initialisation and fences separate one problem from the next.  These kernels leave a problem early --
a failed pivot, a rejected step, a problem that is not finite skips the solve beside teams that run theirs -- so each row's batch
is a heterogeneous base tiled to two full trips of every team and a ragged third.  Per row, through the C ABI, every output
(the optional ones too) pre-filled with a sentinel:
  1. the host core, bit for bit: replica 0 of the B-problem call is the entry's one-thread host core on the base (the family's
     contract: the bits are the host core's whatever T is; the host cores are held to the numpy references by the CPU tests);
  2. trip independence: every output of problem b is base problem b mod nb of the one-trip call on the base alone, bit for bit,
     and no sentinel is left anywhere, the last whole replica and the ragged tail included;
  3. poison in the first trip: problems 1 (NaN in x), 4 (P[0,0] = inf) and, where the entry eliminates without a weight, 7 (a
     singular system) of the first replica come back as the host core has them -- the documented status, the polish's x_out = x
     and steps = 0, the derivatives' NaN fill, the active set's -1 --, the launch returns, every other problem keeps the bits of
     (2).  The float sentinel is itself a NaN, which same_bits and isnan cannot tell from a NaN fill: every output of the poisoned
     call, the poisoned problems' rows and the polish's resid included, is also scanned for the sentinel's bit pattern, so a kernel
     that left a bad problem's outputs unwritten fails here;
  4. polish entries, max_steps = 1: the full and the base call are bit-equal, no count above 1 (the uncapped base has a problem
     with two steps and more: the cap bites).
A difference in (2)-(4) names the first problem that differs and the trip it was solved on."""
import time

import numpy as np
import pytest
import torch

import newton_trip_cases as T
import polish_cases as PC
from newton_trip_cases import ROWS, row_id
from trip_cases import base_size

pytestmark = pytest.mark.gpu
KIND = {k: i for i, k in enumerate(T.K4)}
SENTINEL_BITS = 0x7FF8DEADBEEF0001        # a NaN no kernel produces
SENTINEL_INT = -7


@pytest.fixture(scope="module")
def capi():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from diffqcqp_amd import build, _capi
    build.build()
    _capi.lib()
    return _capi


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()     # (a copy: the bases are read-only)


def device_inputs(base):
    """make_base's / poisoned()'s dict on the device: name -> tensor; the extras and tangents as e0.., t0.."""
    d = {k: _dev(base[k]) for k in ("P", "q", "x", "g") if k in base}
    d.update({"e%d" % i: _dev(e) for i, e in enumerate(base["ex"])})
    d.update({"t%d" % i: _dev(t) for i, t in enumerate(base.get("tan", ()))})
    return d


def tiled(d, idx):
    return {k: v.index_select(0, idx) for k, v in d.items()}


def _sentinel(shape, dtype=torch.float64):
    if dtype is torch.float64:
        return torch.full(shape, SENTINEL_BITS, dtype=torch.int64, device="cuda").view(torch.float64)
    return torch.full(shape, SENTINEL_INT, dtype=torch.int32, device="cuda")


def outputs(row, B):
    """The entry's outputs, all of them, pre-filled with the sentinel: name -> tensor, in the order of the C signature."""
    entry, kind, N = row[:3]
    ne, fam, I = T.extra_cols(kind, N), T.family(entry), torch.int32
    if fam in ("polish", "polish_ls"):
        out = {"x_out": _sentinel((B, N)), "resid": _sentinel((B, 2)), "steps": _sentinel((B,), I), "status": _sentinel((B,), I)}
        if fam == "polish_ls":
            out["halvings"] = _sentinel((B,), I)
        return out
    if fam == "active":
        na = N // 2 if kind == "qcqp" else N
        return {"state": _sentinel((B, na), I), "mult": _sentinel((B, na)), "margin": _sentinel((B,)), "where": _sentinel((B,), I),
                "status": _sentinel((B,), I)}
    if fam == "jac":
        out = {"Jq": _sentinel((B, N, N))}
        if ne:
            out.update({"Ja": _sentinel((B, N, ne)), "Jb": _sentinel((B, N, ne))})
    elif entry.startswith("jvp"):
        out = {"dx": _sentinel((B, N))}
    else:
        out = {"grad_P": _sentinel((B, N, N)), "grad_q": _sentinel((B, N))}
        if ne:
            out.update({"grad_a": _sentinel((B, ne)), "grad_b": _sentinel((B, ne))})
    out["status"] = _sentinel((B,), I)
    return out


def call(capi, row, g, max_steps=None):
    """One call of the row's C entry on the device batch g -> its outputs by name."""
    entry, kind, N, _, flags, reg = row[:6]
    lib, fam, k = capi.lib(), T.family(entry), KIND[kind]
    B = g["q"].shape[0]
    out = outputs(row, B)
    p = lambda name: g[name].data_ptr() if name in g else 0      # noqa: E731
    o = lambda name: out[name].data_ptr() if name in out else 0  # noqa: E731
    head = [k, p("P"), p("q"), p("e0"), p("e1"), p("e2"), p("x")]
    layout = T.DENSE | flags
    mid = (float(reg),) if entry.endswith("_reg") else ()
    ws, nbytes = None, 0
    if N > 64 and fam != "active":
        query = {"polish": lib.dqq_polish_scratch_bytes, "polish_ls": lib.dqq_polish_scratch_bytes,
                 "newton": lib.dqq_newton_scratch_bytes, "jac": lib.dqq_newton_jac_scratch_bytes}[fam]
        nbytes = query(k, N, B)
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device="cuda")
    tail = (ws.data_ptr() if ws is not None else 0, nbytes, torch.cuda.current_stream().cuda_stream)
    fn = getattr(lib, T.ENTRY[entry][0])
    if fam == "polish":
        steps = T.MAX_STEPS[fam] if max_steps is None else max_steps
        rc = fn(*head, o("x_out"), B, N, steps, layout, *mid, o("resid"), o("steps"), o("status"), *tail)
    elif fam == "polish_ls":
        steps = T.MAX_STEPS[fam] if max_steps is None else max_steps
        rc = fn(*head, o("x_out"), B, N, steps, layout, float(reg), T.MAX_HALVINGS, o("resid"), o("steps"), o("status"), o("halvings"),
                *tail)
    elif fam == "active":
        rc = fn(*head, o("state"), o("mult"), o("margin"), o("where"), o("status"), B, N, layout, tail[2])
    elif fam == "jac":
        rc = fn(*head, o("Jq"), o("Ja"), o("Jb"), B, N, layout, *mid, o("status"), *tail)
    elif entry.startswith("jvp"):
        rc = fn(*head, p("t0"), p("t1"), p("t2"), p("t3"), o("dx"), B, N, layout, *mid, o("status"), *tail)
    else:
        rc = fn(*head, p("g"), o("grad_P"), o("grad_q"), o("grad_a"), o("grad_b"), B, N, layout, *mid, o("status"), *tail)
    capi.check(rc, T.ENTRY[entry][0])
    torch.cuda.synchronize()                                      # the launch returns (and the scratch may go)
    return out


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same_bits(row, what, full, one, idx, keep=None):
    """Every output of problem b of `full` is problem idx[b] of `one`, bit for bit (on the problems `keep`)."""
    B, nb, per = row[3], base_size(row[2]), row[7]
    for name, t in full.items():
        diff = (_bits(t) != _bits(one[name]).index_select(0, idx)).reshape(B, -1).any(1)
        if keep is not None:
            diff &= keep
        if bool(diff.any()):
            b = int(torch.nonzero(diff)[0, 0])
            raise AssertionError("%s, %s: %s differs from the one-trip call on %d of %d problems, first on problem %d (base "
                                 "problem %d, solved on trip %d of its team)" % (row_id(row), what, name, int(diff.sum()), B, b,
                                                                                 b % nb, b // per))


def _all_written(row, what, out, rows=None, lo=0):
    """No element of any output (on the problems `rows`, or from problem `lo` on) still holds the sentinel's bit pattern.  The
    float sentinel is a NaN, and a NaN fill compares equal to it under same_bits and isnan: this is what tells them apart."""
    for name, t in out.items():
        part = t[lo:] if rows is None else t[rows]
        left = int((_bits(part) == (SENTINEL_BITS if t.dtype == torch.float64 else SENTINEL_INT)).sum())
        assert left == 0, "%s, %s: %d entries of %s were not written" % (row_id(row), what, left, name)


def _host_rows(row, what, got, want, rows):
    """The device's outputs on `rows` are the host core's, bit for bit (but for the payload of a NaN)."""
    for name, w in want.items():
        a = got[name][rows].cpu().numpy()
        w = w[rows.cpu().numpy()]
        assert a.dtype == w.dtype and PC.same_bits(a.reshape(w.shape), w), "%s, %s: %s is not the host core's" % (row_id(row), what, name)


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_every_team_solves_its_later_problems_as_its_first(oracle, capi, row):
    try:
        _run(capi, row)
    except torch.cuda.OutOfMemoryError:
        raise
    except RuntimeError as e:   # a device fault: nothing more is started on this GPU
        pytest.exit("newton trips %s: %s" % (row_id(row), e), returncode=3)


def _run(capi, row):
    entry, kind, N, B, flags, reg = row[:6]
    nb, per, polish = base_size(N), row[7], T.is_polish(entry)
    t0 = time.perf_counter()
    ref = T.reference(row)                                   # the host core on the clean base, once
    plan = T.poison_plan(row)
    pbase = T.poisoned(row)
    pref = T.host(row, pbase)
    assert B >= 2 * per + 1 and B % per != 0 and max(plan) < min(per, nb)
    base = device_inputs(T.make_base(row))
    idx = torch.arange(B, device="cuda") % nb
    full = tiled(base, idx)
    torch.cuda.synchronize()
    t1 = time.perf_counter()

    # (2) trip independence, bit for bit; (1) the host core on replica 0
    one = call(capi, row, base)
    many = call(capi, row, full)
    first = torch.arange(nb, device="cuda")
    _host_rows(row, "the base alone", one, ref, first)
    _host_rows(row, "replica 0 of B problems", many, ref, first)
    _same_bits(row, "all B problems", many, one, idx)
    _all_written(row, "the base alone", one)
    _all_written(row, "all B problems", many)
    _all_written(row, "the last whole replica and the ragged tail", many, lo=B - B % nb - nb)

    # (3) poison in the first trip does not ride to the second and third
    bad = {k: v.clone() for k, v in full.items()}
    where = torch.tensor(sorted(plan), device="cuda")
    for k, v in device_inputs(pbase).items():
        bad[k][where] = v[where]
    poisoned = call(capi, row, bad)                           # the launch returns
    keep = torch.ones(B, dtype=torch.bool, device="cuda")
    keep[where] = False
    _same_bits(row, "beside the poisoned problems", poisoned, one, idx, keep)
    _host_rows(row, "the poisoned problems", poisoned, pref, where)
    _all_written(row, "the poisoned problems", poisoned, rows=where)   # (a NaN fill is not the NaN the buffers started with)
    _all_written(row, "the poisoned call", poisoned)
    for b, status in plan.items():                           # ... which is what include/diffqcqp_hip.h documents
        assert int(poisoned["status"][b]) == status, (row_id(row), b)
        for name, t in poisoned.items():
            if name == "status":
                continue
            if polish:
                if name == "x_out":
                    assert torch.equal(_bits(t[b]), _bits(bad["x"][b])), (row_id(row), b, "x_out is not x")
                elif name in ("steps", "halvings"):
                    assert int(t[b]) == 0, (row_id(row), b, name)
            elif t.dtype == torch.int32:
                assert bool((t[b] == -1).all()), (row_id(row), b, name)
            else:
                assert bool(torch.isnan(t[b]).all()), (row_id(row), b, name)

    # (4) a capped problem before a quick one
    if polish:
        one1 = call(capi, row, base, max_steps=1)
        many1 = call(capi, row, full, max_steps=1)
        _same_bits(row, "max_steps = 1", many1, one1, idx)
        assert int(many1["steps"].max()) <= 1 and int(one["steps"].max()) >= 2     # (the cap bites)
    t2 = time.perf_counter()
    print("%s: per_trip %d (%s), B %d: host cores and inputs %.2f s, device steps and checks %.2f s"
          % (row_id(row), per, row[8], B, t1 - t0, t2 - t1))
