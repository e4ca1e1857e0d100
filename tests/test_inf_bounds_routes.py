"""CPU checks of where DQQ_F_INFINITE_BOUNDS goes (diffqcqp_amd/csrc/route.cpp compiled for the host behind
tests/hostcore/inf_bounds_route_check.cpp): it reaches the plan of dqq_polish_f64, dqq_newton_bwd_f64 / dqq_newton_jvp_f64 and
dqq_newton_jac_f64 for the box kinds on all three families of each, moves no route, and reaches no other plan -- the QCQP of those
entries accepts and ignores it; for the QP and for every other entry the bit stays an unknown one (DQQ_E_BAD_LAYOUT), as the
route tests of those entries have pinned since before the flag.  Then the constant through both Python faces, and the argument
check of the four entry points with it.  No compute call is made here."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
AUTO, DENSE, DIAG = 0, 1, 2
REF, XD, XL, INFB = 0x100, 0x200, 0x400, 0x800
QP, QCQP, BOX, SBOX = 0, 1, 2, 3
POLISH, NEWTON, JAC, FWD, WARM, BWD, CHECK, JVP = range(8)
E_NULLPTR, E_UNSUPPORTED_N, E_BAD_LAYOUT = -1, -3, -4


@pytest.fixture(scope="module")
def core():
    src = os.path.join(HERE, "hostcore", "inf_bounds_route_check.cpp")
    so = os.path.join(HERE, "hostcore", "libinfboundsroute.so")
    csrc = os.path.join(HERE, "..", "diffqcqp_amd", "csrc")
    deps = [src, os.path.join(HERE, "..", "include", "diffqcqp_hip.h")] + [
        os.path.join(csrc, f) for f in ("route.cpp", "route.h", "tuning.h", "report.h", "worklist.h", "common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-o", so + ".tmp", src])
        os.replace(so + ".tmp", so)
    lib = ctypes.CDLL(so)
    lib.any_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    return lib


def plan(core, entry, kind, N, B, p_layout):
    out = (ctypes.c_int * 4)()
    core.any_plan(entry, kind, N, B, p_layout, out)
    return tuple(out)


def families(core):
    ids = (ctypes.c_int * 9)()
    core.newton_family_ids(ids)
    return {POLISH: tuple(ids[0:3]), NEWTON: tuple(ids[3:6]), JAC: tuple(ids[6:9])}


def test_the_flag_reaches_the_box_kinds_plans_on_all_three_families(core):
    fam = families(core)
    for entry in (POLISH, NEWTON, JAC):
        diag, team, any_ = fam[entry]
        for kind in (BOX, SBOX):
            for more in (0, REF, XD | XL):
                rows = [(DIAG, 8, 37, diag, 0), (DIAG, 2, 1, diag, 0), (DIAG, 64, 5, diag, 0),
                        (DENSE, 3, 37, team, 0), (AUTO, 8, 37, team, 0), (DENSE, 64, 5, team, 0),
                        (DENSE, 65, 5, any_, 1), (AUTO, 200, 1, any_, 1)]
                for layout, N, B, family, scratch in rows:
                    assert plan(core, entry, kind, N, B, layout | more | INFB) == (0, family, scratch, 1), (entry, kind, layout, N)
                    assert plan(core, entry, kind, N, B, layout | more) == (0, family, scratch, 0), (entry, kind, layout, N)
            # the error order is the unflagged call's: N last, and an empty batch launches nothing
            assert plan(core, entry, kind, 6, 5, DIAG | INFB)[:2] == (E_UNSUPPORTED_N, 0)
            assert plan(core, entry, kind, 8, 0, DIAG | INFB)[:3] == (0, 0, 0)
            assert plan(core, entry, kind, 8, 5, 7 | INFB)[0] == E_BAD_LAYOUT and plan(core, entry, kind, 8, 5, INFB | 0x1000)[0] == E_BAD_LAYOUT


def test_it_reaches_no_other_plan(core):
    fam = families(core)
    for entry in (POLISH, NEWTON, JAC):
        # the QCQP accepts the bit and ignores it: the unflagged plan, inf_bounds off
        for layout, N, B in ((DIAG, 8, 37), (DENSE, 8, 37), (AUTO, 20, 37), (DENSE, 66, 5)):
            got = plan(core, entry, QCQP, N, B, layout | INFB)
            assert got == plan(core, entry, QCQP, N, B, layout) and got[0] == 0 and got[3] == 0 and got[1] in fam[entry]
        # the QP has no bounds: an unknown bit, as tests/test_polish_routes.py, test_newton_routes.py and test_jac_routes.py pin it
        for layout in (AUTO, DENSE, DIAG):
            assert plan(core, entry, QP, 8, 37, layout | INFB)[0] == E_BAD_LAYOUT
            assert plan(core, entry, QP, 8, 37, layout)[0] == 0 and plan(core, entry, QP, 8, 37, layout)[3] == 0
    # every other entry, every kind: an unknown bit (its plan has no word for it)
    for entry in (FWD, WARM, BWD, CHECK, JVP):
        for kind in (QP, QCQP, BOX, SBOX):
            for layout in (AUTO, DENSE, DIAG):
                got = plan(core, entry, kind, 8, 37, layout | INFB)
                assert got[0] == E_BAD_LAYOUT and got[3] == -1, (entry, kind, layout)
                assert plan(core, entry, kind, 8, 37, layout)[0] == 0, (entry, kind, layout)


@pytest.fixture(scope="module", params=["ctypes", "pybind11"])
def lib(request):
    from diffqcqp_amd import build, _capi
    build.build()
    if request.param == "ctypes":
        return _capi.ctypes_lib()
    mod = _capi.pybind_lib()
    assert mod is not None, "the pybind11 module was not built"
    assert mod.DQQ_F_INFINITE_BOUNDS == INFB
    return mod


def test_the_constant_and_the_entry_points_argument_checks(lib):
    from diffqcqp_amd import _capi
    assert _capi.F_INFINITE_BOUNDS == INFB
    with open(os.path.join(HERE, "..", "include", "diffqcqp_hip.h")) as f:
        assert "#define DQQ_F_INFINITE_BOUNDS 0x800\n" in f.read()
    one = 8   # a pointer as a Python int, never dereferenced: the checks fail first

    def polish(kind, layout, a=one, b=one, c=None, N=6, B=4):
        return lib.dqq_polish_f64(kind, one, one, a, b, c, one, one, B, N, 8, layout, None, None, None, None, 0, None)

    def bwd(kind, layout, a=one, b=one, c=None, N=6, B=4):
        return lib.dqq_newton_bwd_f64(kind, one, one, a, b, c, one, one, one, one, None, None, B, N, layout, None, None, 0, None)

    def jvp(kind, layout, a=one, b=one, c=None, N=6, B=4):
        return lib.dqq_newton_jvp_f64(kind, one, one, a, b, c, one, None, one, None, None, one, B, N, layout, None, None, 0, None)

    def jac(kind, layout, a=one, b=one, c=None, N=6, B=4):
        return lib.dqq_newton_jac_f64(kind, one, one, a, b, c, one, one, None, None, B, N, layout, None, None, 0, None)

    for call in (polish, bwd, jvp, jac):
        # accepted for the kinds with extras: the call goes on to its later checks (N = 6 is not a DQQ_P_DIAG size)
        assert call(BOX, DIAG | INFB) == E_UNSUPPORTED_N and call(SBOX, DIAG | INFB, c=one) == E_UNSUPPORTED_N
        assert call(QCQP, DIAG | INFB) == E_UNSUPPORTED_N
        assert call(BOX, DENSE | INFB, b=None) == E_NULLPTR
        assert call(BOX, DENSE | INFB, B=0) == 0 and call(SBOX, AUTO | INFB | REF, B=0) == 0
        # refused for the QP, as before
        assert call(QP, DIAG | INFB, a=None, b=None) == E_BAD_LAYOUT and call(QP, DENSE | INFB, a=None, b=None, B=0) == E_BAD_LAYOUT
