"""CPU checks of the route plan of dqq_polish_path_f64 (diffqcqp_amd/csrc/route.cpp: plan_polish_path, compiled for the host
behind tests/hostcore/path_route_check.cpp): the smoothed polish's plan on the path's own three families, appended to Family,
whatever the schedule is; the N -> route boundaries at 64 / 65; the scratch the parents'; and the schedule's argument rules and
their order, in the plan and through both Python faces of the library.  No compute call is made: every call fails its checks or
has B = 0."""
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
DEFAULT = ((1e-1, 1e-2, 1e-3, 1e-4, 0.0), (4, 4, 4, 4, 60))
SCHEDULES = (DEFAULT, ((0.0,), (60,)), ((1e-2,), (0,)), ((0.0, 0.0), (1, 1)), ((1e-3, 1.0, 0.0, 1e-4, 1e-2, 0.0, 1e-1, 5e-1), (0, 1, 2, 3, 4, 5, 6, 2 ** 31 - 1)))
BAD_KAPPAS = (-1e-9, -1.0, math.nan, math.inf, -math.inf)


@pytest.fixture(scope="module")
def core():
    src = os.path.join(HERE, "hostcore", "path_route_check.cpp")
    so = os.path.join(HERE, "hostcore", "libpathroute.so")
    csrc = os.path.join(HERE, "..", "diffqcqp_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("route.cpp", "route.h", "tuning.h", "report.h", "worklist.h", "common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-o", so + ".tmp", src])
        os.replace(so + ".tmp", so)
    lib = ctypes.CDLL(so)
    lib.path_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_double, ctypes.c_void_p,
                              ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.path_families.argtypes = [ctypes.POINTER(ctypes.c_int)]
    return lib


def _host(kappas, steps):
    """The schedule as HOST arrays (kept alive by the caller) -> (kappas array or None, steps array or None)"""
    k = None if kappas is None else (ctypes.c_double * max(len(kappas), 1))(*kappas)
    n = None if steps is None else (ctypes.c_int * max(len(steps), 1))(*steps)
    return k, n


def _addr(a):
    return None if a is None else ctypes.addressof(a)


def plan(core, kind, N, B, p_layout, reg=0.0, schedule=DEFAULT, h=8, n_stages=None):
    """(err, family, scratch, inf_bounds, reg, smooth) of plan_polish_path; n_stages: another count than the schedule's length"""
    k, n = _host(*schedule)
    out = (ctypes.c_int * 6)()
    core.path_plan(0, kind, N, B, p_layout, reg, _addr(k), _addr(n), len(schedule[0]) if n_stages is None else n_stages, h, out)
    return tuple(out)


def smooth_plan(core, kind, N, B, p_layout, reg=0.0, kappa=1e-2, h=8):
    k = (ctypes.c_double * 1)(kappa)
    out = (ctypes.c_int * 6)()
    core.path_plan(1, kind, N, B, p_layout, reg, ctypes.addressof(k), None, 0, h, out)
    return tuple(out)


MATRIX = [(kind, N, B, layout | flags)
          for kind in (QP, QCQP, BOX, SBOX)
          for flags in (0, REF, XD, XL, REF | XD | XL, INFB)
          for layout, Ns, B in ((DIAG, (2, 4, 8, 16, 32, 64, 3, 6, 10, 128), 67), (AUTO, (1, 2, 3, 8, 16, 20, 21, 22, 42, 44, 63, 64), 37),
                                (DENSE, (2, 8, 20, 64), 37), (DENSE, (65, 66, 72, 100, 200), 5), (AUTO, (8, 72), 0), (DIAG, (8, 6), 0))
          for N in Ns]


def test_plan_is_the_smoothed_polishs_on_the_path_families(core):
    fam = (ctypes.c_int * 8)()
    core.path_families(fam)
    assert list(fam[3:6]) == [fam[6] + 1, fam[6] + 2, fam[6] + 3] and fam[7] == 8      # appended: no earlier ordinal moved
    path = {fam[0]: fam[3], fam[1]: fam[4], fam[2]: fam[5], NONE: NONE}
    seen = set()
    for kind, N, B, layout in MATRIX:
        for reg in (0.0, 1e-7):
            parent = smooth_plan(core, kind, N, B, layout, reg)
            for schedule in SCHEDULES:       # a single stage and a schedule of zeros too: always the path's own families
                got = plan(core, kind, N, B, layout, reg, schedule)
                # err, scratch, inf_bounds (never: the flag is an unknown bit, for every kind) and reg are the parent's; `smooth` stays unset
                assert got == (parent[0], path[parent[1]], parent[2], 0, parent[4], 0), (kind, N, B, layout, reg, schedule)
                assert parent[3] == 0
                seen.add(got[1])
    assert seen == {NONE, fam[3], fam[4], fam[5]}
    # the rows themselves: the compact diagonal, LDS teams up to 64, a workgroup per problem on scratch from 65
    assert plan(core, QCQP, 8, 67, DIAG) == (0, fam[3], 0, 0, 0, 0) and plan(core, QP, 6, 67, DIAG)[0] == E_UNSUPPORTED_N
    assert plan(core, BOX, 64, 37, AUTO, 1e-7) == (0, fam[4], 0, 0, 1, 0) and plan(core, BOX, 65, 37, AUTO, 1e-7) == (0, fam[5], 1, 0, 1, 0)
    assert plan(core, SBOX, 64, 5, DENSE) == (0, fam[4], 0, 0, 0, 0) and plan(core, SBOX, 65, 5, DENSE) == (0, fam[5], 1, 0, 0, 0)
    assert plan(core, QP, 8, 0, AUTO) == (0, NONE, 0, 0, 0, 0)
    for kind in (QP, QCQP, BOX, SBOX):       # DQQ_F_INFINITE_BOUNDS: an unknown bit even when every kappa is 0
        assert plan(core, kind, 8, 5, AUTO | INFB, 0.0, ((0.0, 0.0), (1, 1)))[0] == E_BAD_LAYOUT


def test_scratch_is_the_parents(core):
    from diffqcqp_amd import build, _capi
    build.build()
    lib = _capi.ctypes_lib()
    for kind in (QP, QCQP, BOX, SBOX):
        for N, B in ((8, 37), (64, 37), (66, 3), (72, 5), (200, 2000)):
            need = lib.dqq_polish_scratch_bytes(kind, N, B)
            assert (need > 0) == bool(plan(core, kind, N, B, DENSE)[2]) == bool(smooth_plan(core, kind, N, B, DENSE)[2]) == (N > 64)


def test_bad_schedules_are_argument_errors_in_the_plan(core):
    bad = [dict(n_stages=0), dict(n_stages=9), dict(n_stages=-2 ** 31), dict(h=-1), dict(h=61),
           dict(schedule=((1e-1, 0.0), (4, -1))), dict(schedule=((0.0,), (-2 ** 31,)))]
    bad += [dict(schedule=((1e-1, k, 0.0), (4, 4, 4))) for k in BAD_KAPPAS]
    for kind, N, B, layout in MATRIX:
        parent = plan(core, kind, N, B, layout)
        for kw in bad:
            got = plan(core, kind, N, B, layout, **kw)
            if parent[0] in (0, E_UNSUPPORTED_N):       # after kind, size and layout; before N; with B = 0 too
                assert got == (E_BAD_OPTION, NONE, 0, 0, 0, 0), (kind, N, B, layout, kw)
                assert plan(core, kind, N, B, layout, -1.0, **kw)[0] == E_BAD_SIZE      # reg's error comes first
            else:
                assert got == parent
        if parent[0] in (0, E_UNSUPPORTED_N):           # a NULL schedule; the count and max_halvings are looked at first
            assert plan(core, kind, N, B, layout, schedule=(None, (4,)), n_stages=1)[0] == E_NULLPTR
            assert plan(core, kind, N, B, layout, schedule=((0.0,), None), n_stages=1)[0] == E_NULLPTR
            assert plan(core, kind, N, B, layout, schedule=(None, None), n_stages=9)[0] == E_BAD_OPTION
            assert plan(core, kind, N, B, layout, schedule=(None, None), n_stages=1, h=61)[0] == E_BAD_OPTION
    assert plan(core, 4, 8, 5, AUTO, n_stages=0)[0] == E_BAD_KIND and plan(core, QP, 0, 5, AUTO, n_stages=0)[0] == E_BAD_SIZE
    assert plan(core, QP, 8, 5, 7, n_stages=9)[0] == E_BAD_LAYOUT and plan(core, BOX, 8, 5, INFB, n_stages=9)[0] == E_BAD_LAYOUT


@pytest.fixture(scope="module", params=["ctypes", "pybind11"])
def lib(request):
    from diffqcqp_amd import build, _capi
    build.build()
    assert "dqq_polish_path_f64" in _capi.SIGNATURES
    if request.param == "ctypes":
        return _capi.ctypes_lib()
    mod = _capi.pybind_lib()
    assert mod is not None, "the pybind11 module was not built"
    return mod


def test_both_faces_check_the_arguments_in_order(lib):
    one = 8   # a pointer as a Python int, never dereferenced: the checks fail first
    keep = []

    def call(kind=0, P=one, q=one, a=None, b=None, c=None, x=one, xo=one, B=4, N=8, layout=0, reg=0.0, schedule=DEFAULT, S=None, h=8,
             outs=(None,) * 6, ws=None, ws_bytes=0):
        k, n = _host(*schedule)
        keep.append((k, n))
        return lib.dqq_polish_path_f64(kind, P, q, a, b, c, x, xo, B, N, layout, reg, _addr(k), _addr(n),
                                       len(schedule[0]) if S is None else S, h, *outs, ws, ws_bytes, None)

    bad = [dict(S=0), dict(S=9), dict(h=61), dict(h=-1), dict(schedule=((1e-1, 0.0), (4, -1)))]
    bad += [dict(schedule=((1e-1, k), (4, 4))) for k in BAD_KAPPAS]
    for kw in bad:                                              # refused before a pointer, N or the workspace is looked at
        assert call(P=None, **kw) == E_BAD_OPTION and call(N=6, layout=DIAG, **kw) == E_BAD_OPTION
        assert call(N=72, **kw) == E_BAD_OPTION and call(B=0, **kw) == E_BAD_OPTION and call(kind=1, **kw) == E_BAD_OPTION
        assert call(kind=4, **kw) == E_BAD_KIND and call(layout=7, **kw) == E_BAD_LAYOUT and call(B=-1, **kw) == E_BAD_SIZE
        assert call(reg=-1.0, **kw) == E_BAD_SIZE and call(reg=math.inf, P=None, **kw) == E_BAD_SIZE
        assert call(kind=2, a=one, b=one, layout=INFB, **kw) == E_BAD_LAYOUT
    for schedule in ((None, (4,)), ((0.0,), None), (None, None)):       # a NULL schedule, at the same place
        kw = dict(schedule=schedule, S=1)
        assert call(P=None, **kw) == E_NULLPTR and call(N=6, layout=DIAG, **kw) == E_NULLPTR and call(B=0, **kw) == E_NULLPTR
        assert call(kind=4, **kw) == E_BAD_KIND and call(layout=7, **kw) == E_BAD_LAYOUT and call(reg=-1.0, **kw) == E_BAD_SIZE
        assert call(S=9, schedule=schedule) == E_BAD_OPTION and call(h=61, **kw) == E_BAD_OPTION
    for schedule in SCHEDULES:                                  # the smoothed polish's order otherwise
        for outs in ((None,) * 6, (one,) * 6):
            kw = dict(schedule=schedule, outs=outs)
            assert call(kind=4, N=0, **kw) == E_BAD_KIND and call(B=-1, layout=7, **kw) == E_BAD_SIZE
            assert call(kind=1, N=7, a=one, b=one, **kw) == E_BAD_SIZE
            assert call(layout=7, P=None, **kw) == E_BAD_LAYOUT and call(reg=-1e-7, P=None, **kw) == E_BAD_SIZE
            for kind, ex in ((0, {}), (1, dict(a=one, b=one)), (2, dict(a=one, b=one)), (3, dict(a=one, b=one, c=one))):
                assert call(kind=kind, layout=INFB, **ex, **kw) == E_BAD_LAYOUT and call(kind=kind, layout=DIAG | INFB, B=0, **ex, **kw) == E_BAD_LAYOUT
                assert call(kind=kind, layout=DENSE | REF, B=0, **ex, **kw) == 0        # the flags every entry knows stay known
            assert call(P=None, **kw) == E_NULLPTR and call(xo=None, **kw) == E_NULLPTR and call(kind=1, **kw) == E_NULLPTR
            assert call(kind=3, a=one, b=one, **kw) == E_NULLPTR
            assert call(N=6, layout=DIAG, xo=None, **kw) == E_NULLPTR and call(N=6, layout=DIAG, **kw) == E_UNSUPPORTED_N
            assert call(N=72, **kw) == E_WORKSPACE and call(kind=2, a=one, b=one, N=72, ws=one, ws_bytes=64, **kw) == E_WORKSPACE
            assert call(B=0, P=None, q=None, x=None, xo=None, **kw) == 0
