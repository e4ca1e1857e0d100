"""CPU account of which template instantiations of the Newton family and of equil.hip a device test launches.  Every kernel of the
family is held bit for bit to a host core -- by the rows of the tests/test_gpu_*.py tables, which live in the *_cases.py modules --,
and that proves something for the instantiations a row launches and for no other.  What the library compiles, per entry:
dispatch_diag_n's six N (diag_tile.h) x four kinds on the compact diagonal, team_width's four widths (team_dense.h) x four kinds on
the LDS teams, the any-N form x four kinds; the REG = true forms of the polish, the derivatives and the Jacobians beside them, which
only a *_reg_f64 entry with a weight that is not zero launches; both modes of the derivatives.  A row's cell is taken from the plan
functions of route.cpp compiled for the host (tests/hostcore/instantiation_route_check.cpp), not from the row's label.  The same for
equil_kernel: W in {1, 2} columns per lane x {one chunk, further chunks}.  Builds nothing but a host library."""
import ctypes
import os
import subprocess

import pytest

import active_cases as AC
import equil_ref as ER
import inf_bounds_cases as IC
import jac_cases as JC
import newton_cases as NC
import newton_trip_cases as T
import path_cases as PA
import polish_cases as PC
import polish_ls_cases as LC
import reg_cases as RC
import smooth_cases as SC

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "diffqcqp_amd", "csrc")
K4 = ("qp", "qcqp", "box", "sbox")
AUTO, DENSE, DIAG, F_INF = PC.AUTO, PC.DENSE, PC.DIAG, IC.F_INFINITE_BOUNDS
DIAG_N = (2, 4, 8, 16, 32, 64)               # diag_tile.h: dispatch_diag_n
WIDTHS = (8, 16, 32, 64)                     # team_dense.h: dispatch_team
SIZES = [("diag", N) for N in DIAG_N] + [("team", w) for w in WIDTHS] + [("any", 0)]
GROUPS = ("Polish", "Newton", "NewtonJac", "Active", "PolishLs", "PolishSmooth", "NewtonSmooth", "PolishPath")   # family_group_ids' order
REG_FORMS = ("Polish", "Newton", "NewtonJac")             # polish_*_reg.hip, newton_*_reg.hip, newton_jac_*_reg.hip
MODES = {"Newton": ("bwd", "jvp"), "NewtonSmooth": ("bwd", "jvp")}
# entry -> (family_plan's number, the mode it launches)
ENTRY = {"polish": (0, None), "polish_reg": (1, None), "polish_ls": (2, None), "polish_smooth": (3, None), "polish_path": (4, None),
         "bwd": (5, "bwd"), "jvp": (5, "jvp"), "bwd_reg": (6, "bwd"), "jvp_reg": (6, "jvp"), "bwd_smooth": (7, "bwd"),
         "jvp_smooth": (7, "jvp"), "jac": (8, None), "jac_reg": (9, None), "active": (10, None)}
KAPPA = SC.KAPPAS[1]


def compiled():
    """Every (group, kind, form, size, mode, REG) the library holds a kernel for."""
    return {(g, k, form, size, mode, reg) for g in GROUPS for k in K4 for form, size in SIZES for mode in MODES.get(g, (None,))
            for reg in ((False, True) if g in REG_FORMS else (False,))}


def tables():
    """name -> (the entries every row of the table runs, rows as (kind, N, B, layout, reg, kappa)): the bit-equality rows of the
    device tests.  The entries (ENTRIES), the team rows' layouts (TEAM_LAYOUTS, team_layout) and the batches (diag_bs, TEAM_BS,
    ANY_B, diag_b, TEAM_B) are the cases modules' own, which the device tests read too; that a diagonal table runs DQQ_P_DIAG and an
    any-N table DQQ_P_DENSE is restated here, as is the one weight and the one kappa of the two the device tests run: keep them in
    step with the test_*_is_the_host_core functions."""
    def kn(rows, B, layout, reg=0.0, kappa=0.0):
        at = lambda f, r: f(r) if callable(f) else f   # noqa: E731
        return [(r[0], r[1], at(B, r), at(layout, r), reg, kappa) for r in rows]
    third = lambda r: r[2]   # noqa: E731
    ls_team = lambda r: LC.team_layout(r[1])   # noqa: E731
    ls_diag_b = lambda r: LC.diag_bs(r[1])[-1]   # noqa: E731
    return {
        "polish": (PC.ENTRIES, kn(PC.DIAG_ROWS, third, DIAG) + [row for lay in PC.TEAM_LAYOUTS for row in kn(PC.TEAM_ROWS, third, lay)] +
                   kn(PC.ANY_ROWS, third, DENSE)),
        "polish_ls": (LC.ENTRIES, kn(LC.DIAG_ROWS, ls_diag_b, DIAG) + kn(LC.TEAM_ROWS, LC.TEAM_BS[-1], ls_team) + kn(LC.ANY_ROWS, LC.ANY_B, DENSE)),
        "smooth": (SC.ENTRIES, kn(SC.DIAG_ROWS, ls_diag_b, DIAG, kappa=KAPPA) + kn(SC.TEAM_ROWS, SC.TEAM_BS[-1], ls_team, kappa=KAPPA) +
                   kn(SC.ANY_ROWS, SC.ANY_B, DENSE, kappa=KAPPA)),
        "path": (PA.ENTRIES, [(k, N, B, layout, 0.0, KAPPA) for k, N, layout, _, B in PA.ROWS]),
        "newton": (NC.ENTRIES, kn(NC.DIAG_ROWS, third, DIAG) + [row for lay in NC.TEAM_LAYOUTS for row in kn(NC.TEAM_ROWS, third, lay)] +
                   kn(NC.ANY_ROWS, third, DENSE)),
        "jac": (JC.ENTRIES, kn(JC.DIAG_ROWS, third, DIAG) + kn(JC.TEAM_ROWS, third, DENSE) + kn(JC.ANY_ROWS, third, DENSE)),
        "active": (AC.ENTRIES, kn(AC.DIAG_ROWS, lambda r: AC.diag_b(r[1]), DIAG) + kn(AC.TEAM_ROWS, AC.TEAM_B, DENSE) + kn(AC.ANY_ROWS, AC.TEAM_B, DENSE)),
        "reg": (RC.ENTRIES, [(k, N, B, layout, RC.REG, 0.0) for k in RC.KINDS for _, N, B, _, layout in RC.ROWS]),
        "inf_bounds": (IC.ENTRIES, [(k, N, B, layout | F_INF, 0.0, 0.0) for k in IC.KINDS for layout, _, N, B in IC.ROWS]),
    }


@pytest.fixture(scope="module")
def plan():
    src = os.path.join(HERE, "hostcore", "instantiation_route_check.cpp")
    so = os.path.join(HERE, "hostcore", "libinstantiationroute.so")
    deps = [src] + [os.path.join(CSRC, f) for f in ("route.cpp", "route.h", "tuning.h", "report.h", "worklist.h", "common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-o", so + ".tmp", src])
        os.replace(so + ".tmp", so)
    lib = ctypes.CDLL(so)
    lib.family_plan.argtypes = [ctypes.c_int] * 3 + [ctypes.c_longlong, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.POINTER(ctypes.c_int)]
    eight = (ctypes.c_int * 8)()
    lib.family_group_ids(eight)
    group_of = {eight[i] + j: (g, form) for i, g in enumerate(GROUPS) for j, form in enumerate(("diag", "team", "any"))}
    assert len(group_of) == 24

    def cell(entry, kind, N, B, layout, reg, kappa):
        """-> the instantiation the entry launches for this call, as compiled() names it"""
        number, mode = ENTRY[entry]
        out = (ctypes.c_int * 5)()
        lib.family_plan(number, K4.index(kind), N, B, layout, reg, kappa, out)
        assert out[0] == 0, (entry, kind, N, layout, out[0])
        g, form = group_of[out[1]]
        assert ("diag", "team", "any")[out[2] - 1] == form
        assert bool(out[4]) == (g in ("PolishSmooth", "NewtonSmooth")) and bool(out[3]) == (reg != 0.0)
        size = N if form == "diag" else T.team_width(N) if form == "team" else 0
        return (g, kind, form, size, mode, bool(out[3]) and g in REG_FORMS)
    cell.err = lambda entry, kind, N, layout: _err(lib, ENTRY[entry][0], K4.index(kind), N, layout)   # noqa: E731
    return cell


def _err(lib, number, kind, N, layout):
    out = (ctypes.c_int * 5)()
    lib.family_plan(number, kind, N, 37, layout, 0.0, KAPPA, out)
    return out[0]


def missing(plan, tabs):
    """The compiled instantiations no row of the tables launches, sorted."""
    reached = {plan(e, *row) for entries, rows in tabs.values() for e in entries for row in rows}
    assert reached <= compiled()
    return sorted(compiled() - reached, key=str)


def test_the_list_is_what_the_library_compiles(plan):
    """616 kernels; the compact diagonal takes dispatch_diag_n's N and no other; the teams end at N = 64 with the widths of
    team_width, which tests/test_newton_trip_cases.py holds against team_dense.h."""
    assert len(compiled()) == 14 * 4 * 11
    assert ER.FAST_N == DIAG_N and PC.DIAG_N_FIRST + PC.DIAG_N_MORE == (2, 8, 64, 4, 16, 32)
    for entry in ENTRY:
        for kind in K4:
            for N in range(2, 67, 2):
                assert (plan.err(entry, kind, N, DIAG) == 0) == (N in DIAG_N), (entry, kind, N)
    assert sorted({T.team_width(N) for N in range(1, 65)}) == list(WIDTHS) and T.team_width(65) == 256
    assert [PC.ragged_b(N) for N in PC.DIAG_N_MORE] == [289, 73, 37]
    for N in DIAG_N:      # ragged_b: two workgroups of four tiles of 128/N problems, one more tile, one problem
        assert PC.ragged_b(N) == (2 * 4 + 1) * (128 // N) + 1


def test_every_compiled_instantiation_is_launched_by_a_bit_equality_row(plan):
    assert missing(plan, tables()) == []


def test_the_account_fails_when_a_size_leaves_a_table(plan):
    """N = 16 out of the damped polish's diagonal rows: its four kernels are reported, and nothing else."""
    tabs = tables()
    entries, rows = tabs["polish_ls"]
    tabs["polish_ls"] = (entries, [r for r in rows if not (r[1] == 16 and r[3] == DIAG)])
    assert missing(plan, tabs) == sorted((("PolishLs", k, "diag", 16, None, False) for k in K4), key=str)
    tabs = tables()         # the teams of 16 out of the proximal-weight rows: the REG = true forms of three families, both modes
    entries, rows = tabs["reg"]
    tabs["reg"] = (entries, [r for r in rows if T.team_width(r[1]) != 16 or r[3] == DIAG])
    gone = missing(plan, tabs)
    assert len(gone) == 4 * 4 and all(c[2:4] == ("team", 16) and c[5] for c in gone)


def test_one_sided_and_trip_rows_reach_the_new_sizes_too():
    """The flag is a run-time argument of the same kernels: a row per new size, not another instantiation.  The smoothed entries'
    trip table has the teams of 16 for each of its three entries."""
    sizes = {(layout, N) for layout, _, N, _ in IC.ROWS}
    assert {(DIAG, N) for N in PC.DIAG_N_MORE} <= sizes and (DENSE, PC.TEAM_N16) in sizes
    for entry in ("polish", "bwd", "jvp"):
        assert 16 in {T.team_width(N) for e, _, _, N in SC.TRIP_ROWS if e == entry}, entry


def test_equil_kernel_runs_both_widths_with_and_without_further_chunks():
    """equil.hip: equil_kernel<KIND, W>; the chunk loops run when N > 64 W.  The QCQP has W = 2 alone."""
    assert [ER.chunks(N) for N in (2, 3, 64, 65, 70, 128)] == [(2, 1), (1, 1), (2, 1), (1, 2), (2, 1), (2, 1)]
    assert [ER.chunks(N) for N in ER.CHUNKED_N] == [(1, 2), (1, 3), (2, 2)] and 129 - 2 * 64 == 1
    for kind in ER.KINDS:
        got = {(ER.chunks(N)[0], ER.chunks(N)[1] > 1) for N in ER.DENSE_N if not (kind == "qcqp" and N % 2)}
        want = {(W, more) for W in ((2,) if kind == "qcqp" else (1, 2)) for more in (False, True)}
        assert got == want, (kind, got)
    assert {(ER.chunks(N)[0], ER.chunks(N)[1] > 1) for N in ER.DENSE_N if N not in ER.CHUNKED_N} == {(1, False), (2, False)}
