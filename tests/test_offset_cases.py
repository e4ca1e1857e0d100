"""CPU check of tests/offset_cases.py, what tests/test_gpu_offsets.py stands on: every row's largest buffer exceeds its mark in
Python integers with two whole replicas of the base above it, every row takes the route it names (route.cpp behind the host
cores of tests/test_routes.py and tests/check_ref.py), the rows cover every launch family in every mode it has at the marks
the table's docstring states, dqq_workspace_bytes / dqq_scratch_bytes equal their documented formulas in big-int arithmetic at
every row's B and at B = 2^31 - 1, the JVP's and the polish's scratch likewise (plan_jvp / plan_polish behind the host cores of
tests/test_jvp_routes.py and tests/test_polish_routes.py name their rows' routes, `scratch` included) -- and the comparison the GPU test rests on reports a replica that holds another problem's
values."""
import ctypes
import os
import subprocess

import pytest
import torch

import check_ref as R
import offset_cases as OC
from footprint_cases import launches
from offset_cases import (E31, E32, FAMILIES, M32, NO_SUCH_MODE, ONE_LAUNCH, ROWS, STREAMING, V32, C, J, Pl, W, above_mark, batch,
                          compact, count_equal_bits, first_unequal_replica, largest_doubles, modes, per_problem, replica_keys, row_id)
from param_cases import KIND, F, Bw
from test_routes import _build, raw_plan, render
from trip_cases import base_size, listed_mask


@pytest.fixture(scope="module")
def shipped():
    return _build(False)


@pytest.fixture(scope="module")
def lib():
    from diffqcqp_amd import build, _capi
    build.build()
    return _capi.ctypes_lib()


@pytest.fixture(scope="module")
def plans():
    """plan_jvp and plan_polish (route.cpp compiled for the host, as tests/test_jvp_routes.py and tests/test_polish_routes.py
    build it) -> {pass: (plan function, {family id: name})}."""
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "diffqcqp_amd", "csrc")
    out = {}
    for pas, stem, so, names in ((J, "jvp", "libjvproute.so", ONE_LAUNCH[:3]), (Pl, "polish", "libpolishroute.so", ONE_LAUNCH[3:])):
        src, lib = os.path.join(here, "hostcore", stem + "_route_check.cpp"), os.path.join(here, "hostcore", so)
        deps = [src] + [os.path.join(csrc, f) for f in ("route.cpp", "route.h", "tuning.h", "report.h", "worklist.h", "common.h")]
        if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-o", lib + ".tmp", src])
            os.replace(lib + ".tmp", lib)
        core = ctypes.CDLL(lib)
        plan = getattr(core, stem + "_plan")
        plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        ids = (ctypes.c_int * 4)()
        getattr(core, stem + "_family_ids")(ids)
        out[pas] = (plan, dict(zip(list(ids)[:3] if pas == J else list(ids)[1:], names)))
    return out


def check_row_size(row):
    N, B, mark = row[2], row[3], row[7]
    nb = base_size(N)
    per = per_problem(N, row[4])
    assert mark in (M32, E31, E32) and B < 2 ** 31
    assert largest_doubles(row) > mark and 8 * largest_doubles(row) > 8 * mark, row_id(row)
    assert above_mark(row) >= 2 * nb, (row_id(row), above_mark(row))
    # ... 2 nb consecutive problems: every base problem at least twice above the mark, a whole aligned replica among them,
    # and the batch ends inside a replica
    first = -(-mark // per)
    start = -(-first // nb) * nb
    assert start + nb <= B and B % nb != 0, row_id(row)
    assert B == batch(N, mark, row[4])
    assert B * N < 2 ** 31, "vectors of 2^31 elements are out of scope"
    if compact(row):   # V32: EVERY (B,N) buffer of the call -- P, q, x, the bounds, their tangents and gradients -- passes 2^32 bytes
        assert mark == V32 and per == N and 8 * B * N > 2 ** 32 and row[5] == "diag"


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_row_is_above_its_mark(row):
    check_row_size(row)


def test_a_row_below_its_mark_is_caught():
    """The size check has teeth: a row whose B is lowered to the mark, or to one replica above it, fails."""
    row = next(r for r in ROWS if r[7] == E31)
    N, mark = row[2], row[7]
    for B in (mark // (N * N), -(-mark // (N * N)) + base_size(N)):
        with pytest.raises(AssertionError):
            check_row_size(row[:3] + (B,) + row[4:])
    # ... and a compact-layout row sized by the dense rule (B N N past the mark, B N far below it) fails
    row = next(r for r in ROWS if compact(r))
    with pytest.raises(AssertionError):
        check_row_size(row[:3] + (batch(row[2], row[7]),) + row[4:])


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_row_takes_its_route(shipped, plans, row):
    pas, kind, N, B, layout, _, want = row[:7]
    if pas in (J, Pl):
        plan, names = plans[pas]
        out = (ctypes.c_int * 3)()
        plan(KIND[kind], N, B, layout, out)
        assert out[0] == 0 and names[out[1]] + (" scr" if out[2] else "") == want
    elif pas == C:
        out = (ctypes.c_int * 3)()
        R.hostcore().hostcheck_plan(KIND[kind], N, B, layout, out)
        assert out[0] == 0 and out[1] == 15 and "check/%d" % out[2] == want      # (15: route.h Family::Check)
    else:   # (a warm forward's plan is the cold one: tests/test_warm_routes.py)
        assert render(raw_plan(shipped, 1 if pas == Bw else 0, KIND[kind], N, B, layout)) == want


def check_coverage(rows):
    have = {}
    for r in rows:
        for fm in modes(r):
            have[fm] = max(have.get(fm, 0), r[7])
    for fam in FAMILIES:
        for mode in ("direct", "listed"):
            if (fam, mode) in NO_SUCH_MODE:
                assert (fam, mode) not in have, (fam, mode)
            else:
                assert have.get((fam, mode), 0) >= M32, "no row at M32 for %s, %s" % (fam, mode)
    for fam in STREAMING:
        assert max(have.get((fam, m), 0) for m in ("direct", "listed")) >= E31, "no row at E31 for %s" % fam
    assert any(r[7] >= E31 and r[2] == 32 and "bqcqp" in {f for f, _ in modes(r)} for r in rows), "no bqcqp row at N = 32, E31"
    for fam in ("fdiag", "fwave64"):
        assert any(r[0] == F and r[2] == 64 and r[7] == E32 and fam in {f for f, _ in modes(r)} for r in rows), fam
    assert all(r[7] != E32 or r[0] == F for r in rows), "E32 rows are forward rows"
    listed = [r for r in rows if any(m == "listed" for _, m in modes(r))]
    assert all(r[5] == "mixed" for r in listed)
    assert any(r[2] >= 32 and r[7] >= E31 for r in listed), "no segmented-list row at E31"
    assert any(r[2] <= 16 and r[7] >= E31 for r in listed), "no plain-list row at E31"
    for fam in ("JvpDiag", "PolishDiag", "fdiag", "bdiag"):   # the compact layout: the only one of the first two, a public one of the others
        assert any(compact(r) and (fam, "direct") in modes(r) for r in rows), "no DQQ_P_DIAG row for %s" % fam
    for fam in ("JvpTeam", "PolishTeam"):                      # the streaming shape of the team kernels: one small team per problem
        assert any(r[7] >= E31 and r[2] == 8 and (fam, "direct") in modes(r) for r in rows), "no N = 8 row at E31 for %s" % fam
    warm = [r for r in rows if r[0] == W]
    assert any(r[7] >= E31 and r[6].startswith("fdiag") for r in warm) and any(not r[6].startswith("fdiag") for r in warm)
    for k in ("qp", "qcqp", "box", "sbox"):
        assert any(r[0] == F and r[1] == k for r in rows) and any(r[0] == Bw and r[1] == k for r in rows), k
    assert len({r[:6] for r in rows}) == len(rows)


def test_rows_cover_every_family_in_every_mode():
    check_coverage(ROWS)
    assert set(f for f, _ in NO_SUCH_MODE) <= set(FAMILIES)


@pytest.mark.parametrize("fam", FAMILIES)
def test_a_family_taken_out_of_the_table_is_caught(fam):
    """The coverage check has teeth: without the rows of any one family it fails."""
    rest = [r for r in ROWS if fam not in {f for f, _ in modes(r)}]
    assert len(rest) < len(ROWS)
    with pytest.raises(AssertionError):
        check_coverage(rest)


def test_workspace_and_scratch_sizes_in_big_int_arithmetic(shipped, lib):
    Bs = sorted({r[3] for r in ROWS} | {2 ** 31 - 1})
    for B in Bs:
        want = OC.workspace_bytes(B)
        assert lib.dqq_workspace_bytes(B) == want == shipped.route_workspace_bytes(B), B
        assert want > 4 * B
    cases = {(KIND[r[1]], 1 if r[0] == Bw else 0, r[2], r[4]) for r in ROWS if r[0] != C}
    # ... and sizes on both sides of every rule of the formula: LDS-resident and global matrices, the 4 GiB cap on the grid, one slice beyond 4 GiB
    cases |= {(k, p, N, l) for k in range(4) for p in (0, 1) for N in (22, 34, 44, 64, 66, 70, 98, 100, 130, 1024, 1450, 4096, 20000)
              for l in (0, OC.REF) if not (k == 1 and N % 2)}
    seen_scratch = seen_wide = 0
    for kind, pas, N, layout in sorted(cases):
        for B in Bs + [1, 511, 512, 513]:
            kq = 2 if (pas == 1 and kind == 3) else kind          # the signed box backward takes the box QP's scratch
            want = OC.scratch_bytes(kq, pas, N, B, layout)
            assert lib.dqq_scratch_bytes(kq, pas, N, B, layout) == want, (kind, pas, N, B, layout)
            seen_scratch += want > 0
            seen_wide += want >= 2 ** 32
        assert lib.dqq_scratch_bytes(3, 1, N, Bs[-1], layout) == 0
    assert seen_scratch > 100 and seen_wide > 0          # (the formula passes 2^32 bytes: a 32-bit product would show)
    # dqq_jvp_f64's scratch is the backward's reference-order one (the signed box QP's the box QP's), the polish has its own query
    seen_jvp = seen_polish = 0
    for r in [r for r in ROWS if r[0] in (J, Pl)] + [(J, "sbox", 22, 0, 1), (J, "qcqp", 44, 0, 0), (J, "qp", 65, 0, 1), (J, "qp", 64, 0, 2),
                                                    (Pl, "box", 65, 0, 1), (Pl, "qcqp", 1450, 0, 0), (Pl, "sbox", 20000, 0, 1)]:
        pas, kind, N, _, layout = r[:5]
        for B in Bs + [1, 511, 512, 513]:
            if pas == J:
                want = OC.jvp_scratch_bytes(KIND[kind], N, B, layout)
                assert lib.dqq_scratch_bytes(min(KIND[kind], 2), 1, N, B, layout | OC.REF) == (want if layout != OC.DIAG else
                                                                                               OC.scratch_bytes(min(KIND[kind], 2), 1, N, B, OC.REF))
                seen_jvp += want > 0
            else:
                want = OC.polish_scratch_bytes(N, B, layout)
                assert lib.dqq_polish_scratch_bytes(KIND[kind], N, B) == OC.polish_scratch_bytes(N, B, 1)
                seen_polish += want > 0
            row_want = [x for x in ROWS if x[:5] == r[:5]]
            assert not row_want or (want > 0) == row_want[0][6].endswith(" scr")
    assert seen_jvp > 20 and seen_polish > 20


# ---------------------------------------------------------------- the comparison helper can fail
def _tiled(nb, B, width, dtype):
    g = torch.Generator().manual_seed(7)
    base = torch.randn(nb, width, generator=g, dtype=torch.float64)
    if dtype != torch.float64:
        base = (base * 100).to(dtype)
    return base[torch.arange(B) % nb].contiguous()


@pytest.mark.parametrize("dtype", [torch.float64, torch.int32])
def test_comparison_reports_a_replica_that_holds_another_problems_values(dtype):
    row = next(r for r in ROWS if r[6] == "fwave64")      # a direct row: problem b answers to problem b mod 37
    nb, width = base_size(row[2]), 9
    B = 40 * nb + 11
    key, ref, queued = replica_keys(row, B)
    assert queued is None and torch.equal(ref, torch.arange(nb)) and torch.equal(key, torch.arange(B) % nb)
    mark = 25 * nb + 5                                    # a "mark" inside the array: replicas above it are the ones at stake
    for chunk in (1 << 25, 5 * nb * width, 1):           # one chunk, a few replicas per chunk, a problem per chunk
        t = _tiled(nb, B, width, dtype)
        assert first_unequal_replica(t, key, ref, chunk) is None
        # problem 13 of a replica above the mark reads base problem 14's values: the wrapped-address failure
        b = 31 * nb + 13
        assert b > mark
        t[b] = t[14]
        assert first_unequal_replica(t, key, ref, chunk) == (b, 1)
        # ... and one more in the ragged tail
        t[B - 2] = t[0]
        assert first_unequal_replica(t, key, ref, chunk) == (b, 2)
        t[b] = t[13]
        assert first_unequal_replica(t, key, ref, chunk) == (B - 2, 1)
    # a sign bit is a difference (bits, not values), a NaN equals itself
    if dtype == torch.float64:
        t = _tiled(nb, B, width, dtype)
        t[:, 3] = float("nan")
        t[5::nb, 2] = 0.0
        assert first_unequal_replica(t, key, ref) is None
        t[3 * nb + 5, 2] = -0.0
        assert first_unequal_replica(t, key, ref) == (3 * nb + 5, 1)


@pytest.mark.parametrize("row", [r for r in ROWS if r[0] in (F, Bw) and len(launches(r[6])) > 1], ids=row_id)
def test_keys_behind_a_work_list_follow_the_queued_tiles(row):
    """replica_keys against trip_cases.listed_mask (the same rule, tile by tile) on the first problems of the batch; every key
    that occurs has its reference problem, the first of its kind; below N = 64 every whole tile is queued."""
    N = row[2]
    nb = base_size(N)
    n = 5 * nb * 64 + 3
    key, ref, queued = replica_keys(row, n)
    assert queued.tolist() == listed_mask(row, n)
    assert torch.equal(key, torch.arange(n) % nb + nb * queued)
    for k in range(2 * nb):
        at = torch.nonzero(key == k)
        assert int(ref[k]) == (int(at[0, 0]) if len(at) else n)
    if N < 64:
        T = len(queued) - len(queued) % (4 * 64)          # (whole tiles of every layout)
        assert bool(queued[:T].all())
    else:
        # tiles of two: a non-diagonal problem meets the drain only, most diagonal ones both kernels
        fast, drain = ref[:nb] < n, ref[nb:] < n
        assert bool((fast | drain).all()) and int((fast & drain).sum()) > nb // 2
        assert all(bool(drain[b]) and not bool(fast[b]) for b in range(nb) if b % 3 == 1)


def test_sentinel_count():
    t = torch.zeros(10, 4, dtype=torch.float64)
    sentinel = torch.tensor([0x7FF8DEADBEEF0001], dtype=torch.int64).view(torch.float64)
    t[7:] = sentinel
    bits = int(sentinel.view(torch.int64))
    assert count_equal_bits(t, 6, bits) == 12 and count_equal_bits(t, 0, bits) == 12
    t[8, 1] = 1.0
    assert count_equal_bits(t, 7, bits) == 11
