"""CPU checks of dqq_jvp_f64's route plan (diffqcqp_amd/csrc/route.cpp: plan_jvp, compiled for the host behind
tests/hostcore/jvp_route_check.cpp) against DESIGN.md section 3's table, of its scratch query, and of the argument checks of
the entry point through both Python faces of the library.  No compute call is made here."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
AUTO, DENSE, DIAG = 0, 1, 2
REF, XD, XL = 0x100, 0x200, 0x400
QP, QCQP, BOX, SBOX = 0, 1, 2, 3
NONE = 0                                     # route.h: Family::None; JvpDiag, JvpTeam, JvpAny are asked of the host build
E_NULLPTR, E_BAD_SIZE, E_UNSUPPORTED_N, E_BAD_LAYOUT, E_WORKSPACE, E_BAD_KIND = -1, -2, -3, -4, -5, -7


@pytest.fixture(scope="module")
def core():
    src = os.path.join(HERE, "hostcore", "jvp_route_check.cpp")
    so = os.path.join(HERE, "hostcore", "libjvproute.so")
    csrc = os.path.join(HERE, "..", "diffqcqp_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("route.cpp", "route.h", "tuning.h", "report.h", "worklist.h", "common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-o", so + ".tmp", src])
        os.replace(so + ".tmp", so)
    lib = ctypes.CDLL(so)
    lib.jvp_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.jvp_scratch_applies.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int]
    ids = (ctypes.c_int * 3)()
    lib.jvp_family_ids(ids)
    global JDIAG, JTEAM, JANY
    JDIAG, JTEAM, JANY = ids
    assert len({NONE, JDIAG, JTEAM, JANY}) == 4
    return lib


def plan(core, kind, N, B, p_layout):
    out = (ctypes.c_int * 3)()
    core.jvp_plan(kind, N, B, p_layout, out)
    return tuple(out)


LIMIT = {QP: 64, QCQP: 42, BOX: 21, SBOX: 21}     # the reference-order limits of the LDS team kernel
BEYOND = {QP: 65, QCQP: 44, BOX: 22, SBOX: 22}


def test_plan_is_the_table(core):
    for kind in (QP, QCQP, BOX, SBOX):
        for flags in (0, REF, XD, XL, REF | XD | XL):     # accepted and ignored
            for N in (2, 4, 8, 16, 32, 64):
                assert plan(core, kind, N, 67, DIAG | flags) == (0, JDIAG, 0)
            for N in (3, 6, 10, 128):
                if kind == QCQP and N % 2:
                    continue
                assert plan(core, kind, N, 67, DIAG | flags) == (E_UNSUPPORTED_N, NONE, 0)
            for layout in (AUTO, DENSE):                   # AUTO is not classified: the general kernel
                for N in (2, 8, 16, 20, LIMIT[kind]):
                    assert plan(core, kind, N, 37, layout | flags) == (0, JTEAM, 0), (kind, N)
                for N in (BEYOND[kind], 100, 200):
                    assert plan(core, kind, N, 5, layout | flags) == (0, JANY, 1), (kind, N)
                assert plan(core, kind, 8, 5, layout | flags) == plan(core, kind, 8, 10 ** 6, layout | flags)   # B plays no part
    assert plan(core, QP, 63, 5, AUTO) == (0, JTEAM, 0) and plan(core, BOX, 21, 5, DENSE) == (0, JTEAM, 0)


def test_scratch_is_the_backwards_reference_order_query(core):
    """JvpAny runs exactly where dqq_scratch_bytes(kind == 3 ? 2 : kind, 1, N, B, p_layout | DQQ_F_REFERENCE_ORDER) is not 0."""
    for kind in (QP, QCQP, BOX, SBOX):
        for N in range(2, 80, 2):
            for layout in (AUTO, DENSE, AUTO | XD):
                needs = core.jvp_scratch_applies(BOX if kind == SBOX else kind, 1, N, 5, layout | REF)
                assert plan(core, kind, N, 5, layout)[2] == needs and (plan(core, kind, N, 5, layout)[1] == JANY) == bool(needs)


def test_empty_batch_and_error_order(core):
    for layout in (AUTO, DENSE, DIAG):
        assert plan(core, QP, 8, 0, layout) == (0, NONE, 0)
    assert plan(core, QP, 6, 0, DIAG) == (0, NONE, 0)
    assert plan(core, 4, 0, -1, 7)[0] == E_BAD_KIND and plan(core, -1, 8, 5, AUTO)[0] == E_BAD_KIND     # the kind first
    assert plan(core, QP, 0, 5, 7)[0] == E_BAD_SIZE and plan(core, QCQP, 7, 5, AUTO)[0] == E_BAD_SIZE   # then the sizes
    assert plan(core, QP, 8, 2 ** 31, AUTO)[0] == E_BAD_SIZE
    assert plan(core, QP, 6, 5, 7)[0] == E_BAD_LAYOUT and plan(core, QP, 6, 5, DIAG | 0x800)[0] == E_BAD_LAYOUT   # the layout
    assert plan(core, QP, 6, 5, DIAG)[0] == E_UNSUPPORTED_N                                              # N last


@pytest.fixture(scope="module", params=["ctypes", "pybind11"])
def lib(request):
    from diffqcqp_amd import build, _capi
    build.build()
    assert "dqq_jvp_f64" in _capi.SIGNATURES
    if request.param == "ctypes":
        return _capi.ctypes_lib()
    mod = _capi.pybind_lib()
    assert mod is not None, "the pybind11 module was not built"
    return mod


def test_both_faces_check_the_arguments_in_order(lib):
    one = 8   # a pointer as a Python int, never dereferenced: the checks fail first

    def call(kind=0, P=one, q=one, a=None, b=None, c=None, x=one, dP=None, dq=None, da=None, db=None, dx=one, B=4, N=8,
             layout=0, ws=None, ws_bytes=0):
        return lib.dqq_jvp_f64(kind, P, q, a, b, c, x, dP, dq, da, db, dx, B, N, 1e-10, layout, None, ws, ws_bytes, None)

    assert call(kind=4, N=0) == E_BAD_KIND and call(kind=-1) == E_BAD_KIND
    assert call(B=-1, layout=7) == E_BAD_SIZE and call(kind=1, a=one, b=one, N=7) == E_BAD_SIZE
    assert call(layout=7) == E_BAD_LAYOUT and call(layout=0x800) == E_BAD_LAYOUT
    assert call(P=None) == E_NULLPTR and call(q=None) == E_NULLPTR and call(x=None) == E_NULLPTR and call(dx=None) == E_NULLPTR
    assert call(kind=1) == E_NULLPTR and call(kind=2, a=one) == E_NULLPTR and call(kind=3, a=one, b=one) == E_NULLPTR
    assert call(da=one) == E_NULLPTR and call(db=one) == E_NULLPTR            # the QP has no extras: their tangents must be NULL
    assert call(N=6, layout=DIAG, dx=None) == E_NULLPTR and call(N=6, layout=DIAG) == E_UNSUPPORTED_N   # as the backward orders them
    assert call(N=65) == E_WORKSPACE and call(kind=2, a=one, b=one, N=22, ws=one, ws_bytes=64) == E_WORKSPACE
    for layout in (AUTO, DENSE, DIAG, AUTO | REF | XD | XL):                  # an empty batch is a no-op, whatever the pointers
        assert call(B=0, P=None, q=None, x=None, dx=None, layout=layout) == 0
