"""CPU checks of the route plans of the *_reg_f64 entries (diffqcqp_amd/csrc/route.cpp: plan_polish_reg, plan_newton_reg,
plan_newton_jac_reg, compiled for the host behind tests/hostcore/reg_route_check.cpp): the parent's plan but for the `reg`
field, over the route matrix of the parents' route tests; a reg that is negative, a NaN or infinite is refused by the plan and,
through both Python faces of the library, by the entries before any pointer is looked at.  No compute call is made."""
import ctypes
import math
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
AUTO, DENSE, DIAG = 0, 1, 2
REF, XD, XL, INFB = 0x100, 0x200, 0x400, 0x800
QP, QCQP, BOX, SBOX = 0, 1, 2, 3
NONE = 0
E_NULLPTR, E_BAD_SIZE, E_UNSUPPORTED_N, E_BAD_LAYOUT, E_WORKSPACE, E_BAD_KIND = -1, -2, -3, -4, -5, -7
BAD_REGS = (-1e-7, -math.inf, math.inf, math.nan)


@pytest.fixture(scope="module")
def core():
    src = os.path.join(HERE, "hostcore", "reg_route_check.cpp")
    so = os.path.join(HERE, "hostcore", "libregroute.so")
    csrc = os.path.join(HERE, "..", "diffqcqp_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("route.cpp", "route.h", "tuning.h", "report.h", "worklist.h", "common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-o", so + ".tmp", src])
        os.replace(so + ".tmp", so)
    lib = ctypes.CDLL(so)
    lib.reg_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int,
                             ctypes.c_double, ctypes.POINTER(ctypes.c_int)]
    return lib


def plan(core, entry, kind, N, B, p_layout, reg=None):
    """(err, family, scratch, inf_bounds, reg); reg None: the parent's plan"""
    out = (ctypes.c_int * 5)()
    core.reg_plan(entry, int(reg is None), kind, N, B, p_layout, 0.0 if reg is None else reg, out)
    return tuple(out)


MATRIX = [(kind, N, B, layout | flags)
          for kind in (QP, QCQP, BOX, SBOX)
          for flags in (0, REF, XD, XL, REF | XD | XL, INFB)
          for layout, Ns, B in ((DIAG, (2, 4, 8, 16, 32, 64, 3, 6, 10, 128), 67), (AUTO, (1, 2, 3, 8, 16, 20, 21, 22, 42, 44, 63, 64), 37),
                                (DENSE, (2, 8, 20, 64), 37), (DENSE, (65, 66, 72, 100, 200), 5), (AUTO, (8, 72), 0), (DIAG, (8, 6), 0))
          for N in Ns]


@pytest.mark.parametrize("entry", (0, 1, 2))
def test_plan_is_the_parents_but_for_reg(core, entry):
    seen = set()
    for kind, N, B, layout in MATRIX:
        parent = plan(core, entry, kind, N, B, layout)
        assert parent[4] == 0
        assert plan(core, entry, kind, N, B, layout, 0.0) == parent and plan(core, entry, kind, N, B, layout, -0.0) == parent
        for reg in (1e-300, 1e-10, 1e-7, 1e-2, 1.7976931348623157e308):
            got = plan(core, entry, kind, N, B, layout, reg)
            assert got[:4] == parent[:4]
            assert got[4] == int(parent[0] == 0 and parent[1] != NONE), (kind, N, B, layout, reg)
            seen.add((got[1], got[4]))
    assert len({f for f, r in seen if r}) == 3     # the diagonal, team and any-N family of the entry, each with REG


@pytest.mark.parametrize("entry", (0, 1, 2))
def test_bad_reg_is_an_argument_error(core, entry):
    for kind, N, B, layout in MATRIX:
        parent = plan(core, entry, kind, N, B, layout)
        for reg in BAD_REGS:
            got = plan(core, entry, kind, N, B, layout, reg)
            if parent[0] in (0, E_UNSUPPORTED_N):       # after kind, size and layout; before N; with B = 0 too
                assert got == (E_BAD_SIZE, NONE, 0, 0, 0), (kind, N, B, layout, reg)
            else:
                assert got == parent
    assert plan(core, entry, 4, 8, 5, AUTO, -1.0)[0] == E_BAD_KIND and plan(core, entry, QP, 0, 5, AUTO, -1.0)[0] == E_BAD_SIZE
    assert plan(core, entry, QP, 8, 5, 7, -1.0)[0] == E_BAD_LAYOUT and plan(core, entry, QP, 8, 5, INFB, -1.0)[0] == E_BAD_LAYOUT


@pytest.fixture(scope="module", params=["ctypes", "pybind11"])
def lib(request):
    from diffqcqp_amd import build, _capi
    build.build()
    assert {"dqq_polish_reg_f64", "dqq_newton_bwd_reg_f64", "dqq_newton_jvp_reg_f64", "dqq_newton_jac_reg_f64"} <= set(_capi.SIGNATURES)
    if request.param == "ctypes":
        return _capi.ctypes_lib()
    mod = _capi.pybind_lib()
    assert mod is not None, "the pybind11 module was not built"
    return mod


@pytest.mark.parametrize("entry", ("polish", "bwd", "jvp", "jac"))
def test_both_faces_check_the_arguments_in_order(lib, entry):
    one = 8   # a pointer as a Python int, never dereferenced: the checks fail first

    def call(kind=0, P=one, q=one, a=None, b=None, c=None, x=one, req=one, B=4, N=8, layout=0, reg=1e-7, ws=None, ws_bytes=0):
        if entry == "polish":
            return lib.dqq_polish_reg_f64(kind, P, q, a, b, c, x, req, B, N, 8, layout, reg, None, None, None, ws, ws_bytes, None)
        if entry == "bwd":
            return lib.dqq_newton_bwd_reg_f64(kind, P, q, a, b, c, x, req, None, None, None, None, B, N, layout, reg, None, ws, ws_bytes, None)
        if entry == "jvp":
            return lib.dqq_newton_jvp_reg_f64(kind, P, q, a, b, c, x, None, None, None, None, req, B, N, layout, reg, None, ws, ws_bytes, None)
        return lib.dqq_newton_jac_reg_f64(kind, P, q, a, b, c, x, req, None, None, B, N, layout, reg, None, ws, ws_bytes, None)

    for reg in BAD_REGS:                                      # refused before a pointer, N or the workspace is looked at
        assert call(reg=reg, P=None) == E_BAD_SIZE and call(reg=reg, N=6, layout=DIAG) == E_BAD_SIZE
        assert call(reg=reg, N=72) == E_BAD_SIZE and call(reg=reg, B=0) == E_BAD_SIZE
        assert call(reg=reg, kind=4) == E_BAD_KIND and call(reg=reg, layout=7) == E_BAD_LAYOUT and call(reg=reg, B=-1) == E_BAD_SIZE
    for reg in (0.0, 1e-7):                                   # the parents' order
        assert call(kind=4, N=0, reg=reg) == E_BAD_KIND and call(B=-1, layout=7, reg=reg) == E_BAD_SIZE
        assert call(layout=7, P=None, reg=reg) == E_BAD_LAYOUT and call(layout=INFB, reg=reg) == E_BAD_LAYOUT   # the QP has no bounds
        assert call(P=None, reg=reg) == E_NULLPTR and call(req=None, reg=reg) == E_NULLPTR and call(kind=1, reg=reg) == E_NULLPTR
        assert call(N=6, layout=DIAG, req=None, reg=reg) == E_NULLPTR and call(N=6, layout=DIAG, reg=reg) == E_UNSUPPORTED_N
        assert call(N=72, reg=reg) == E_WORKSPACE and call(kind=2, a=one, b=one, N=72, ws=one, ws_bytes=64, layout=INFB, reg=reg) == E_WORKSPACE
        assert call(B=0, P=None, q=None, x=None, req=None, reg=reg) == 0
