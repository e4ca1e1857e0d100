"""CPU checks of the Newton derivatives' route plan (diffqcqp_amd/csrc/route.cpp: plan_newton, compiled for the host behind
tests/hostcore/newton_route_check.cpp) against DESIGN.md section 3's table, of the scratch query, and of the argument checks of
dqq_newton_bwd_f64 / dqq_newton_jvp_f64 through both Python faces of the library.  No compute call is made here."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
AUTO, DENSE, DIAG = 0, 1, 2
REF, XD, XL = 0x100, 0x200, 0x400
QP, QCQP, BOX, SBOX = 0, 1, 2, 3
NONE = 0
E_NULLPTR, E_BAD_SIZE, E_UNSUPPORTED_N, E_BAD_LAYOUT, E_WORKSPACE, E_BAD_KIND = -1, -2, -3, -4, -5, -7


@pytest.fixture(scope="module")
def core():
    src = os.path.join(HERE, "hostcore", "newton_route_check.cpp")
    so = os.path.join(HERE, "hostcore", "libnewtonroute.so")
    csrc = os.path.join(HERE, "..", "diffqcqp_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("route.cpp", "route.h", "tuning.h", "report.h", "worklist.h", "common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-o", so + ".tmp", src])
        os.replace(so + ".tmp", so)
    lib = ctypes.CDLL(so)
    lib.newton_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    ids = (ctypes.c_int * 4)()
    lib.newton_family_ids(ids)
    global NDIAG, NTEAM, NANY
    last, NDIAG, NTEAM, NANY = ids
    assert (NDIAG, NTEAM, NANY) == (last + 1, last + 2, last + 3)     # appended: no earlier family moved
    return lib


def plan(core, kind, N, B, p_layout):
    out = (ctypes.c_int * 3)()
    core.newton_plan(kind, N, B, p_layout, out)
    return tuple(out)


def test_plan_is_the_table(core):
    for kind in (QP, QCQP, BOX, SBOX):
        for flags in (0, REF, XD, XL, REF | XD | XL):     # accepted and ignored
            for N in (2, 4, 8, 16, 32, 64):
                assert plan(core, kind, N, 67, DIAG | flags) == (0, NDIAG, 0)
            for N in (3, 6, 10, 128):
                if kind == QCQP and N % 2:
                    continue
                assert plan(core, kind, N, 67, DIAG | flags) == (E_UNSUPPORTED_N, NONE, 0)
            for layout in (AUTO, DENSE):                   # AUTO is not classified: the general kernel
                for N in (1, 2, 3, 8, 16, 20, 21, 22, 42, 44, 63, 64):
                    if kind == QCQP and N % 2:
                        continue
                    assert plan(core, kind, N, 37, layout | flags) == (0, NTEAM, 0), (kind, N)
                for N in (65, 66, 100, 200):
                    if kind == QCQP and N % 2:
                        continue
                    assert plan(core, kind, N, 5, layout | flags) == (0, NANY, 1), (kind, N)
                for N in (8, 64, 66):                       # B plays no part
                    assert plan(core, kind, N, 1, layout | flags) == plan(core, kind, N, 10 ** 6, layout | flags)
            assert plan(core, kind, 8, 1, DIAG | flags) == plan(core, kind, 8, 10 ** 6, DIAG | flags)


def test_empty_batch_and_error_order(core):
    for layout in (AUTO, DENSE, DIAG):
        assert plan(core, QP, 8, 0, layout) == (0, NONE, 0)
    assert plan(core, QP, 6, 0, DIAG) == (0, NONE, 0) and plan(core, QP, 100, 0, DENSE) == (0, NONE, 0)
    assert plan(core, 4, 0, -1, 7)[0] == E_BAD_KIND and plan(core, -1, 8, 5, AUTO)[0] == E_BAD_KIND     # the kind first
    assert plan(core, QP, 0, 5, 7)[0] == E_BAD_SIZE and plan(core, QCQP, 7, 5, AUTO)[0] == E_BAD_SIZE   # then the sizes
    assert plan(core, QP, 8, 2 ** 31, AUTO)[0] == E_BAD_SIZE
    assert plan(core, QP, 6, 5, 7)[0] == E_BAD_LAYOUT and plan(core, QP, 6, 5, DIAG | 0x800)[0] == E_BAD_LAYOUT   # the layout
    assert plan(core, QP, 6, 5, DIAG)[0] == E_UNSUPPORTED_N                                              # N last


@pytest.fixture(scope="module", params=["ctypes", "pybind11"])
def lib(request):
    from diffqcqp_amd import build, _capi
    build.build()
    assert {"dqq_newton_bwd_f64", "dqq_newton_jvp_f64", "dqq_newton_scratch_bytes"} <= set(_capi.SIGNATURES)
    if request.param == "ctypes":
        return _capi.ctypes_lib()
    mod = _capi.pybind_lib()
    assert mod is not None, "the pybind11 module was not built"
    return mod


def test_scratch_query(lib):
    """Nothing up to N = 64; beyond it a slice of N (N|1) + 7 N doubles (rounded up to even) per workgroup of a grid that is B up
    to 512 workgroups, in Python integers.  dqq_scratch_bytes knows nothing of these entries."""
    for kind in (QP, QCQP, BOX, SBOX):
        for N in (2, 8, 20, 64):
            assert lib.dqq_newton_scratch_bytes(kind, N, 1000) == 0
        for N in (66, 100, 130):
            sl = 8 * ((N * (N | 1) + 7 * N + 1) // 2 * 2)
            assert lib.dqq_newton_scratch_bytes(kind, N, 1) == sl
            assert lib.dqq_newton_scratch_bytes(kind, N, 5) == 5 * sl
            assert lib.dqq_newton_scratch_bytes(kind, N, 512) == 512 * sl == lib.dqq_newton_scratch_bytes(kind, N, 10 ** 6)
            assert lib.dqq_newton_scratch_bytes(kind, N, 0) == 0 and lib.dqq_newton_scratch_bytes(kind, N, -1) == 0
    assert lib.dqq_newton_scratch_bytes(QP, 65, 3) == 3 * 8 * (65 * 65 + 7 * 65)
    assert lib.dqq_newton_scratch_bytes(4, 100, 5) == 0 and lib.dqq_newton_scratch_bytes(QCQP, 67, 5) == 0   # no such call
    assert lib.dqq_scratch_bytes(QP, 0, 64, 5, DENSE) == 0     # (the forward's and backward's query: as before)


@pytest.mark.parametrize("mode", ["bwd", "jvp"])
def test_both_faces_check_the_arguments_in_order(lib, mode):
    one = 8   # a pointer as a Python int, never dereferenced: the checks fail first

    def call(kind=0, P=one, q=one, a=None, b=None, c=None, x=one, req=one, o2=None, o3=None, B=4, N=8, layout=0, ws=None, ws_bytes=0):
        """req: grad_x / dx, the mode's required argument; o2, o3: grad_a, grad_b / da, db"""
        if mode == "bwd":
            return lib.dqq_newton_bwd_f64(kind, P, q, a, b, c, x, req, None, None, o2, o3, B, N, layout, None, ws, ws_bytes, None)
        return lib.dqq_newton_jvp_f64(kind, P, q, a, b, c, x, None, None, o2, o3, req, B, N, layout, None, ws, ws_bytes, None)

    assert call(kind=4, N=0) == E_BAD_KIND and call(kind=-1, P=None) == E_BAD_KIND
    assert call(B=-1, layout=7) == E_BAD_SIZE and call(kind=1, a=one, b=one, N=7) == E_BAD_SIZE and call(N=0, P=None) == E_BAD_SIZE
    assert call(layout=7, P=None) == E_BAD_LAYOUT and call(layout=0x800) == E_BAD_LAYOUT
    assert call(P=None) == E_NULLPTR and call(q=None) == E_NULLPTR and call(x=None) == E_NULLPTR and call(req=None) == E_NULLPTR
    assert call(kind=1) == E_NULLPTR and call(kind=2, a=one) == E_NULLPTR and call(kind=3, a=one, b=one) == E_NULLPTR
    assert call(o2=one) == E_NULLPTR and call(o3=one) == E_NULLPTR                             # the QP has no extras to move
    assert call(N=6, layout=DIAG, req=None) == E_NULLPTR and call(N=6, layout=DIAG) == E_UNSUPPORTED_N
    assert call(N=65) == E_WORKSPACE and call(N=65, req=None) == E_NULLPTR                      # the workspace last
    assert call(kind=2, a=one, b=one, N=66, ws=one, ws_bytes=64) == E_WORKSPACE
    for layout in (AUTO, DENSE, DIAG, AUTO | REF | XD | XL):                  # an empty batch is a no-op, whatever the pointers
        assert call(B=0, P=None, q=None, x=None, req=None, layout=layout) == 0
        assert call(B=0, N=100, P=None, q=None, x=None, req=None, layout=layout) == 0
