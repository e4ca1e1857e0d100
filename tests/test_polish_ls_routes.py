"""CPU checks of the route plan of dqq_polish_ls_f64 (diffqcqp_amd/csrc/route.cpp: plan_polish_ls, compiled for the host behind
tests/hostcore/polish_ls_route_check.cpp): dqq_polish_reg_f64's plan on the damped polish's own three families, over the route
matrix of the parents' route tests; a max_halvings outside 0 .. 60 is refused by the plan and, through both Python faces of the
library, by the entry before any pointer is looked at; a NULL `halvings` is accepted.  No compute call is made."""
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
E_NULLPTR, E_BAD_SIZE, E_UNSUPPORTED_N, E_BAD_LAYOUT, E_WORKSPACE, E_BAD_OPTION, E_BAD_KIND = -1, -2, -3, -4, -5, -6, -7
BAD_HALVINGS = (-1, 61, 1000, -2 ** 31)
GOOD_HALVINGS = (0, 1, 8, 60)


@pytest.fixture(scope="module")
def core():
    src = os.path.join(HERE, "hostcore", "polish_ls_route_check.cpp")
    so = os.path.join(HERE, "hostcore", "libpolishlsroute.so")
    csrc = os.path.join(HERE, "..", "diffqcqp_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("route.cpp", "route.h", "tuning.h", "report.h", "worklist.h", "common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-o", so + ".tmp", src])
        os.replace(so + ".tmp", so)
    lib = ctypes.CDLL(so)
    lib.polish_ls_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_double,
                                   ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.polish_ls_families.argtypes = [ctypes.POINTER(ctypes.c_int)]
    return lib


def plan(core, kind, N, B, p_layout, reg=0.0, max_halvings=None):
    """(err, family, scratch, inf_bounds, reg); max_halvings None: the parent's plan (plan_polish_reg)"""
    out = (ctypes.c_int * 5)()
    core.polish_ls_plan(int(max_halvings is None), kind, N, B, p_layout, reg, 0 if max_halvings is None else max_halvings, out)
    return tuple(out)


MATRIX = [(kind, N, B, layout | flags)
          for kind in (QP, QCQP, BOX, SBOX)
          for flags in (0, REF, XD, XL, REF | XD | XL, INFB)
          for layout, Ns, B in ((DIAG, (2, 4, 8, 16, 32, 64, 3, 6, 10, 128), 67), (AUTO, (1, 2, 3, 8, 16, 20, 21, 22, 42, 44, 63, 64), 37),
                                (DENSE, (2, 8, 20, 64), 37), (DENSE, (65, 66, 72, 100, 200), 5), (AUTO, (8, 72), 0), (DIAG, (8, 6), 0))
          for N in Ns]


def test_plan_is_the_parents_on_the_damped_families(core):
    fam = (ctypes.c_int * 7)()
    core.polish_ls_families(fam)
    assert list(fam[3:6]) == [fam[6] + 1, fam[6] + 2, fam[6] + 3]      # appended: no earlier ordinal moved
    damped = {fam[0]: fam[3], fam[1]: fam[4], fam[2]: fam[5], NONE: NONE}
    seen = set()
    for kind, N, B, layout in MATRIX:
        for reg in (0.0, 1e-7):
            parent = plan(core, kind, N, B, layout, reg)
            for h in GOOD_HALVINGS:      # 0 too: the damped kernels with no halving allowed
                got = plan(core, kind, N, B, layout, reg, h)
                assert got == (parent[0], damped[parent[1]], parent[2], parent[3], parent[4]), (kind, N, B, layout, reg, h)
                seen.add(got[1])
    assert seen == {NONE, fam[3], fam[4], fam[5]}
    # the rows themselves: the compact diagonal, LDS teams up to 64, a workgroup per problem on scratch beyond
    assert plan(core, QCQP, 8, 67, DIAG, 0.0, 8) == (0, fam[3], 0, 0, 0) and plan(core, QP, 6, 67, DIAG, 0.0, 8)[0] == E_UNSUPPORTED_N
    assert plan(core, BOX, 64, 37, AUTO | INFB, 1e-7, 8) == (0, fam[4], 0, 1, 1) and plan(core, SBOX, 65, 5, DENSE, 0.0, 60) == (0, fam[5], 1, 0, 0)
    assert plan(core, QP, 8, 0, AUTO, 0.0, 8) == (0, NONE, 0, 0, 0)


def test_bad_max_halvings_is_an_argument_error(core):
    for kind, N, B, layout in MATRIX:
        parent = plan(core, kind, N, B, layout)
        for h in BAD_HALVINGS:
            got = plan(core, kind, N, B, layout, 0.0, h)
            if parent[0] in (0, E_UNSUPPORTED_N):       # after kind, size and layout; before N; with B = 0 too
                assert got == (E_BAD_OPTION, NONE, 0, 0, 0), (kind, N, B, layout, h)
            else:
                assert got == parent
            if parent[0] in (0, E_UNSUPPORTED_N):       # reg's error comes first
                assert plan(core, kind, N, B, layout, -1.0, h)[0] == E_BAD_SIZE and plan(core, kind, N, B, layout, math.nan, h)[0] == E_BAD_SIZE
    assert plan(core, 4, 8, 5, AUTO, 0.0, -1)[0] == E_BAD_KIND and plan(core, QP, 0, 5, AUTO, 0.0, -1)[0] == E_BAD_SIZE
    assert plan(core, QP, 8, 5, 7, 0.0, 61)[0] == E_BAD_LAYOUT and plan(core, QP, 8, 5, INFB, 0.0, 61)[0] == E_BAD_LAYOUT


@pytest.fixture(scope="module", params=["ctypes", "pybind11"])
def lib(request):
    from diffqcqp_amd import build, _capi
    build.build()
    assert "dqq_polish_ls_f64" in _capi.SIGNATURES
    if request.param == "ctypes":
        return _capi.ctypes_lib()
    mod = _capi.pybind_lib()
    assert mod is not None, "the pybind11 module was not built"
    return mod


def test_both_faces_check_the_arguments_in_order(lib):
    one = 8   # a pointer as a Python int, never dereferenced: the checks fail first

    def call(kind=0, P=one, q=one, a=None, b=None, c=None, x=one, xo=one, B=4, N=8, layout=0, reg=0.0, h=8, halvings=None, ws=None,
             ws_bytes=0):
        return lib.dqq_polish_ls_f64(kind, P, q, a, b, c, x, xo, B, N, 8, layout, reg, h, None, None, None, halvings, ws, ws_bytes, None)

    for h in BAD_HALVINGS:                                    # refused before a pointer, N or the workspace is looked at
        assert call(h=h, P=None) == E_BAD_OPTION and call(h=h, N=6, layout=DIAG) == E_BAD_OPTION
        assert call(h=h, N=72) == E_BAD_OPTION and call(h=h, B=0) == E_BAD_OPTION and call(h=h, halvings=one) == E_BAD_OPTION
        assert call(h=h, kind=4) == E_BAD_KIND and call(h=h, layout=7) == E_BAD_LAYOUT and call(h=h, B=-1) == E_BAD_SIZE
        assert call(h=h, reg=-1.0) == E_BAD_SIZE and call(h=h, reg=math.inf, P=None) == E_BAD_SIZE
    for h in GOOD_HALVINGS:                                   # the parents' order; a NULL `halvings` is no error
        for halvings in (None, one):
            kw = dict(h=h, halvings=halvings)
            assert call(kind=4, N=0, **kw) == E_BAD_KIND and call(B=-1, layout=7, **kw) == E_BAD_SIZE
            assert call(layout=7, P=None, **kw) == E_BAD_LAYOUT and call(layout=INFB, **kw) == E_BAD_LAYOUT   # the QP has no bounds
            assert call(reg=-1e-7, P=None, **kw) == E_BAD_SIZE
            assert call(P=None, **kw) == E_NULLPTR and call(xo=None, **kw) == E_NULLPTR and call(kind=1, **kw) == E_NULLPTR
            assert call(N=6, layout=DIAG, xo=None, **kw) == E_NULLPTR and call(N=6, layout=DIAG, **kw) == E_UNSUPPORTED_N
            assert call(N=72, **kw) == E_WORKSPACE and call(kind=2, a=one, b=one, N=72, ws=one, ws_bytes=64, layout=INFB, **kw) == E_WORKSPACE
            assert call(B=0, P=None, q=None, x=None, xo=None, **kw) == 0
