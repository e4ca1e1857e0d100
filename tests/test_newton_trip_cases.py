"""CPU check of tests/newton_trip_cases.py, what tests/test_gpu_newton_trips.py stands on: every row takes the route it names
through the host-compiled route.cpp (the existing tests/hostcore/*_route_check.cpp programs), its B sends each team of the
persistent kernel through at least two trips and ends inside a third, per_trip is the launch geometry -- held against
team_dense.h's own team_geometry compiled for the host, and for the global-memory kernels against the library's count of scratch
slices --, the rows cover every entry at every width and kind, the base is heterogeneous in what a team keeps between problems,
and the host cores give the poisoned base the documented statuses.  Builds nothing but host programs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import newton_trip_cases as T
from newton_trip_cases import ENTRIES, F_INF, K4, ROWS, WIDTHS, row_id

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "diffqcqp_amd", "csrc")
KIND = {k: i for i, k in enumerate(K4)}
TEAM_ROWS = [r for r in ROWS if r[2] <= 64]
ANY_ROWS = [r for r in ROWS if r[2] > 64]


def _shared(name, src, compiler=("g++", "-O1", "-std=c++17"), deps=("route.cpp", "route.h", "tuning.h", "report.h", "worklist.h", "common.h")):
    src = os.path.join(HERE, "hostcore", src)
    so = os.path.join(HERE, "hostcore", name)
    deps = [src] + [os.path.join(CSRC, f) for f in deps]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(list(compiler) + ["-fPIC", "-shared", "-fvisibility=hidden", "-o", so + ".tmp", src])
        os.replace(so + ".tmp", so)
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def routes():
    """-> plan(row, B): (err, the route's name in route.h's Family, scratch, inf_bounds, reg) of the row's entry at a batch of B."""
    reg = _shared("libregroute.so", "reg_route_check.cpp")
    reg.reg_plan.argtypes = [ctypes.c_int] * 4 + [ctypes.c_longlong, ctypes.c_int, ctypes.c_double, ctypes.POINTER(ctypes.c_int)]
    ls = _shared("libpolishlsroute.so", "polish_ls_route_check.cpp")
    ls.polish_ls_plan.argtypes = [ctypes.c_int] * 3 + [ctypes.c_longlong, ctypes.c_int, ctypes.c_double, ctypes.c_int,
                                                       ctypes.POINTER(ctypes.c_int)]
    act = _shared("libactiveroute.so", "active_route_check.cpp")
    act.active_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    ids = _shared("libinfboundsroute.so", "inf_bounds_route_check.cpp")
    names = {}
    nine = (ctypes.c_int * 9)()
    ids.newton_family_ids(nine)
    for i, stem in enumerate(("Polish", "Newton", "NewtonJac")):
        for j, form in enumerate(("Diag", "Team", "Any")):
            names[nine[3 * i + j]] = stem + form
    seven = (ctypes.c_int * 7)()
    ls.polish_ls_families(seven)
    names.update({seven[3]: "PolishLsDiag", seven[4]: "PolishLsTeam", seven[5]: "PolishLsAny"})
    four = (ctypes.c_int * 4)()
    act.active_family_ids(four)
    names.update({four[1]: "ActiveDiag", four[2]: "ActiveTeam", four[3]: "ActiveAny"})
    assert len(names) == 15

    def plan(row, B):
        entry, kind, N, _, flags, w = row[:6]
        out = (ctypes.c_int * 5)()
        layout, fam = T.DENSE | flags, T.family(entry)
        if fam == "polish_ls":
            ls.polish_ls_plan(0, KIND[kind], N, B, layout, w, T.MAX_HALVINGS, out)
        elif fam == "active":
            act.active_plan(KIND[kind], N, B, layout, out)
            out[3], out[2] = out[2], 0                                  # (its third word is inf_bounds; it takes no scratch)
        else:
            reg.reg_plan({"polish": 0, "newton": 1, "jac": 2}[fam], int(not entry.endswith("_reg")), KIND[kind], N, B, layout, w, out)
        return out[0], names.get(out[1]), out[2], out[3], out[4]
    return plan


@pytest.fixture(scope="module")
def lib():
    from diffqcqp_amd import build, _capi
    build.build()
    return _capi.ctypes_lib()


@pytest.fixture(scope="module")
def geometry():
    """team_dense.h's team_geometry and dispatch_team, polish_team.h's polish_slice_doubles: compiled for the host alone."""
    from diffqcqp_amd.build import _hipcc
    g = _shared("libteamgeometry.so", "team_geometry_check.cpp", deps=("team_dense.h", "polish_team.h", "launch.h", "polish_core.h"),
                compiler=(_hipcc(), "--offload-host-only", "-x", "hip", "-O1", "-std=c++17"))
    g.team_geometry_of.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)]
    g.polish_slice_doubles_of.restype = ctypes.c_longlong
    return g


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_row_takes_its_route_and_so_does_its_base(routes, row):
    entry, kind, N, B, flags, reg, want = row[:7]
    err, name, scratch, inf, regged = routes(row, B)
    assert (err, name) == (0, want), row_id(row)
    assert bool(inf) == bool(flags & F_INF) and bool(regged) == bool(reg)
    assert bool(scratch) == (N > 64 and T.family(entry) != "active")
    assert routes(row, T.base_size(N)) == (err, name, scratch, inf, regged)
    assert T.base_size(N) <= row[7]                       # the base alone: at most one trip
    assert (T.ENTRY[entry][0].endswith("_reg_f64") or entry == "polish_ls") or not reg


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_batch_is_two_trips_and_a_ragged_third(row):
    entry, kind, N, B = row[:4]
    per = T.per_trip(entry, kind, N)
    assert row[7] == per and B >= 2 * per + 1 and B % per != 0, row_id(row)
    assert B == T.batch_size(per) == 2 * per + 3
    assert max(T.POISON_NAN, T.POISON_INF, T.POISON_SINGULAR, T.ACTIVE) < min(per, T.base_size(N))
    assert B <= 131075


def test_per_trip_takes_the_values_the_slices_give():
    for entry in ("polish", "polish_ls", "bwd", "jvp_reg"):
        assert [T.per_trip(entry, "qp", N) for N in (6, 12, 20, 34, 64)] == [65536, 32768, 16384, 8192, 2048]
    assert T.team_wpb("polish", "qp", 34) == 4 and T.team_wpb("polish", "qp", 64) == 1
    assert T.team_wpb("jac", "box", 8) == 3 and T.per_trip("jac", "box", 8) == 256 * 8 * 3 * 8
    assert [T.team_wpb("jac", k, 34) for k in K4] == [3, 2, 1, 1]
    assert T.team_wpb("jac", "box", 64) == 1 and 8 * T.slice_doubles("jac", "box", 64) > 65536   # (one wave, more than 64 KiB)


@pytest.mark.parametrize("row", ANY_ROWS, ids=row_id)
def test_any_rows_per_trip_is_the_librarys_count_of_scratch_slices(lib, row):
    entry, kind, N, B = row[:4]
    fam = T.family(entry)
    if fam == "active":
        # ActiveAny takes no scratch: its grid is any_grid(B, 1) = min(B, 512) workgroups (active_dense.hip:193-195, team_dense.h:201-208, general_any.hip:70-76)
        assert row[7] == 512 and "general_any.hip:70-76" in row[8]
        return
    query = {"polish": lib.dqq_polish_scratch_bytes, "polish_ls": lib.dqq_polish_scratch_bytes,
             "newton": lib.dqq_newton_scratch_bytes, "jac": lib.dqq_newton_jac_scratch_bytes}[fam]
    piece = query(KIND[kind], N, 1)
    assert piece == 8 * T.slice_doubles(entry, kind, N) > 0
    assert query(KIND[kind], N, B) == row[7] * piece == query(KIND[kind], N, row[7])


@pytest.mark.parametrize("row", TEAM_ROWS, ids=row_id)
def test_team_rows_geometry_is_the_headers(geometry, row):
    entry, kind, N, B = row[:4]
    Tw, sl = T.team_width(N), T.slice_doubles(entry, kind, N)
    assert geometry.team_width_of(N) == Tw and geometry.team_width_of(65) == 0
    if T.family(entry) in ("polish", "polish_ls"):
        assert geometry.polish_slice_doubles_of(N) == sl
    out = (ctypes.c_longlong * 3)()
    geometry.team_geometry_of(sl, Tw, B, out)
    wpb, lds, grid = out
    assert wpb == T.team_wpb(entry, kind, N) and grid == 256 * 8 and lds == 8 * sl * (64 // Tw) * wpb
    assert grid * wpb * (64 // Tw) == row[7]
    geometry.team_geometry_of(sl, Tw, T.base_size(N), out)     # the base alone: a team per problem, no second trip
    assert out[0] == wpb and out[2] * wpb * (64 // Tw) >= T.base_size(N)


def test_rows_cover_what_the_issue_of_newton_trips_asks_for():
    assert len({r[:6] for r in ROWS}) == len(ROWS)
    for entry in ENTRIES:
        mine = [r for r in ROWS if r[0] == entry and (entry != "polish_ls" or not r[5]) and r[2] != 8]   # (the two rows beside the matrix)
        # every persistent width: T = 8, 16, 32, 64 at four waves and at one wave per workgroup, Any
        got = sorted((T.team_width(r[2]), T.team_wpb(entry, r[1], r[2]) if r[2] <= 64 else 0) for r in mine)
        assert [t for t, _ in got] == [8, 16, 32, 64, 64, 256], (entry, got)
        w64 = [w for t, w in got if t == 64]
        assert 1 in w64 and max(w64) > 1, (entry, got)
        assert {r[2] for r in mine} <= {n for _, n in WIDTHS} | {19}
        assert {r[1] for r in mine} == set(K4), entry                          # every kind
        for k in ("box", "sbox"):                                              # one-sided boxes on both box kinds
            assert any(r[1] == k and r[4] & F_INF for r in mine), (entry, k)
        assert all(bool(r[5]) == entry.endswith("_reg") for r in mine)
    for w, (Tw, N) in enumerate(WIDTHS):                                       # every kind at every width, over the entries
        assert {r[1] for r in ROWS if T.team_width(r[2]) == Tw and (Tw != 64 or r[2] == N)} == set(K4), Tw
    assert any(r[2] == 19 and r[1] != "qcqp" for r in ROWS)                     # ld = n | 1 = n
    assert any(r[0] == "polish_ls" and r[5] for r in ROWS) and any(r[0] == "jac_reg" and r[5] for r in ROWS)
    assert any(r[0] == "jac" and r[1] == "box" and r[2] == 8 and T.team_wpb("jac", "box", 8) == 3 for r in ROWS)
    assert not any(r[1] == "qp" and r[4] for r in ROWS)                        # (the QP has no bounds: the flag is an error there)
    assert 50 <= len(ROWS) <= 60


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_base_is_heterogeneous_and_poison_gets_its_status(oracle, row):
    ref = T.check_heterogeneous(row)
    entry, kind, N = row[:3]
    bad = T.host(row, T.poisoned(row))
    plan = T.poison_plan(row)
    assert set(plan) == ({1, 4} if (row[5] or T.family(entry) == "active") else {1, 4, 7})
    for b, st in plan.items():
        assert bad["status"][b] == st, (row_id(row), b, bad["status"][b])
    keep = np.ones(T.base_size(N), dtype=bool)
    keep[list(plan)] = False
    for name, want in ref.items():                       # a bad problem touches only its own rows
        assert np.array_equal(bad[name][keep], want[keep], equal_nan=True), (row_id(row), name)
    if T.is_polish(entry):                               # x_out = x bit for bit, no step
        x = T.poisoned(row)["x"]
        for b in plan:
            assert bad["steps"][b] == 0 and np.array_equal(bad["x_out"][b], x[b], equal_nan=True), (row_id(row), b)
    else:                                                # the documented NaN fill (the active set: -1 in state and where)
        for b in plan:
            for name, v in bad.items():
                if name != "status":
                    assert (v[b] == -1).all() if v.dtype.kind == "i" else np.isnan(v[b]).all(), (row_id(row), b, name)
