"""CPU checks of the Newton Jacobians' route plan (diffqcqp_amd/csrc/route.cpp: plan_newton_jac, compiled for the host behind
tests/hostcore/newton_jac_route_check.cpp) against a Python statement of the route table, of the scratch query in Python's big
integers, and of the argument checks of dqq_newton_jac_f64 through both Python faces of the library.  No compute call is made."""
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
NS = (2, 8, 20, 64, 65, 66)


def _build(out, flags):
    src = os.path.join(HERE, "hostcore", "newton_jac_route_check.cpp")
    csrc = os.path.join(HERE, "..", "diffqcqp_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("route.cpp", "route.h", "tuning.h", "report.h", "worklist.h", "common.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17"] + flags + ["-o", out + ".tmp", src])
        os.replace(out + ".tmp", out)
    return out


@pytest.fixture(scope="module")
def core():
    lib = ctypes.CDLL(_build(os.path.join(HERE, "hostcore", "libnewtonjacroute.so"), ["-fPIC", "-shared", "-fvisibility=hidden"]))
    lib.newton_jac_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    ids = (ctypes.c_int * 4)()
    lib.newton_jac_family_ids(ids)
    global JDIAG, JTEAM, JANY
    last, JDIAG, JTEAM, JANY = ids
    assert (JDIAG, JTEAM, JANY) == (last + 1, last + 2, last + 3)     # appended: no earlier family moved
    return lib


def plan(core, kind, N, B, p_layout):
    out = (ctypes.c_int * 3)()
    core.newton_jac_plan(kind, N, B, p_layout, out)
    return tuple(out)


def table(kind, N, B, p_layout):
    """The route table in Python: (err, family, scratch)."""
    if kind not in (QP, QCQP, BOX, SBOX):
        return (E_BAD_KIND, NONE, 0)
    if B < 0 or B >= 2 ** 31 or N < 1 or (kind == QCQP and N % 2):
        return (E_BAD_SIZE, NONE, 0)
    if (p_layout & 0xff) not in (AUTO, DENSE, DIAG) or p_layout & ~(0xff | REF | XD | XL):
        return (E_BAD_LAYOUT, NONE, 0)
    if B == 0:
        return (0, NONE, 0)
    if (p_layout & 0xff) == DIAG:
        return (0, JDIAG, 0) if N in (2, 4, 8, 16, 32, 64) else (E_UNSUPPORTED_N, NONE, 0)
    return (0, JANY, 1) if N > 64 else (0, JTEAM, 0)


def test_plan_is_the_table(core):
    for kind in (QP, QCQP, BOX, SBOX):
        for N in NS + (1, 3, 4, 6, 16, 32, 63, 200):
            for layout in (AUTO, DENSE, DIAG):
                for flags in (0, REF, XD | XL, REF | XD | XL):     # accepted and ignored
                    for B in (0, 1, 67, 10 ** 6):                  # B plays no part but for the empty batch
                        assert plan(core, kind, N, B, layout | flags) == table(kind, N, B, layout | flags), (kind, N, layout, B)
    assert plan(core, QP, 6, 5, DIAG) == (E_UNSUPPORTED_N, NONE, 0)


def test_empty_batch_and_error_order(core):
    assert plan(core, QP, 6, 0, DIAG) == (0, NONE, 0) and plan(core, QP, 100, 0, DENSE) == (0, NONE, 0)
    assert plan(core, 4, 0, -1, 7)[0] == E_BAD_KIND and plan(core, -1, 8, 5, AUTO)[0] == E_BAD_KIND     # the kind first
    assert plan(core, QP, 0, 5, 7)[0] == E_BAD_SIZE and plan(core, QCQP, 7, 5, AUTO)[0] == E_BAD_SIZE   # then the sizes
    assert plan(core, QP, 8, 2 ** 31, AUTO)[0] == E_BAD_SIZE
    assert plan(core, QP, 6, 5, 7)[0] == E_BAD_LAYOUT and plan(core, QP, 6, 5, DIAG | 0x800)[0] == E_BAD_LAYOUT   # the layout
    assert plan(core, QP, 6, 5, DIAG)[0] == E_UNSUPPORTED_N                                              # N last


def test_stand_alone_host_check_runs_clean():
    exe = _build(os.path.join(HERE, "hostcore", "newton_jac_route_check"), ["-DNEWTON_JAC_ROUTE_MAIN"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "0 failures" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


@pytest.fixture(scope="module", params=["ctypes", "pybind11"])
def lib(request):
    from diffqcqp_amd import build, _capi
    build.build()
    assert {"dqq_newton_jac_f64", "dqq_newton_jac_scratch_bytes"} <= set(_capi.SIGNATURES)
    if request.param == "ctypes":
        return _capi.ctypes_lib()
    mod = _capi.pybind_lib()
    assert mod is not None, "the pybind11 module was not built"
    return mod


def test_scratch_query(lib):
    """Nothing up to N = 64; beyond it a slice of N (N|1) + N C + 7 N doubles (rounded up to even), C = N (QP), 2N (QCQP) or 3N
    (box kinds) columns, per workgroup of a grid that is B up to 512 workgroups (fewer where 512 slices would pass 4 GiB), in
    Python integers."""
    cols = {QP: 1, QCQP: 2, BOX: 3, SBOX: 3}
    for kind in (QP, QCQP, BOX, SBOX):
        for N in (2, 8, 20, 64):
            assert lib.dqq_newton_jac_scratch_bytes(kind, N, 1000) == 0
        for N in (66, 100, 130, 1000):
            doubles = (N * (N | 1) + N * cols[kind] * N + 7 * N + 1) // 2 * 2
            sl = 8 * doubles
            grid = max(1, min(512, (4 << 30) // sl))
            assert lib.dqq_newton_jac_scratch_bytes(kind, N, 1) == sl
            assert lib.dqq_newton_jac_scratch_bytes(kind, N, 5) == 5 * sl
            assert lib.dqq_newton_jac_scratch_bytes(kind, N, 10 ** 6) == grid * sl == lib.dqq_newton_jac_scratch_bytes(kind, N, 512)
            assert lib.dqq_newton_jac_scratch_bytes(kind, N, 0) == 0 and lib.dqq_newton_jac_scratch_bytes(kind, N, -1) == 0
    assert lib.dqq_newton_jac_scratch_bytes(QP, 65, 3) == 3 * 8 * (65 * 65 + 65 * 65 + 7 * 65 + 1)
    assert lib.dqq_newton_jac_scratch_bytes(4, 100, 5) == 0 and lib.dqq_newton_jac_scratch_bytes(QCQP, 67, 5) == 0   # no such call
    assert lib.dqq_newton_scratch_bytes(QP, 66, 1) == 8 * ((66 * 67 + 7 * 66 + 1) // 2 * 2)    # (the single-vector entries': as before)


def test_both_faces_check_the_arguments_in_order(lib):
    one = 8   # a pointer as a Python int, never dereferenced: the checks fail first

    def call(kind=0, P=one, q=one, a=None, b=None, c=None, x=one, Jq=one, Ja=None, Jb=None, B=4, N=8, layout=0, ws=None, ws_bytes=0):
        return lib.dqq_newton_jac_f64(kind, P, q, a, b, c, x, Jq, Ja, Jb, B, N, layout, None, ws, ws_bytes, None)

    assert call(kind=4, N=0) == E_BAD_KIND and call(kind=-1, P=None) == E_BAD_KIND
    assert call(B=-1, layout=7) == E_BAD_SIZE and call(kind=1, a=one, b=one, N=7) == E_BAD_SIZE and call(N=0, P=None) == E_BAD_SIZE
    assert call(layout=7, P=None) == E_BAD_LAYOUT and call(layout=0x800) == E_BAD_LAYOUT
    assert call(P=None) == E_NULLPTR and call(q=None) == E_NULLPTR and call(x=None) == E_NULLPTR
    assert call(Jq=None) == E_NULLPTR and call(kind=2, a=one, b=one, Jq=None, N=65) == E_NULLPTR    # nothing requested
    assert call(kind=1) == E_NULLPTR and call(kind=2, a=one) == E_NULLPTR and call(kind=3, a=one, b=one) == E_NULLPTR
    assert call(Ja=one) == E_NULLPTR and call(Jb=one) == E_NULLPTR                             # the QP has no extras to move
    assert call(N=6, layout=DIAG, Jq=None) == E_NULLPTR and call(N=6, layout=DIAG) == E_UNSUPPORTED_N
    assert call(N=65) == E_WORKSPACE and call(N=65, x=None) == E_NULLPTR                        # the workspace last
    assert call(kind=2, a=one, b=one, Jq=None, Ja=one, N=66, ws=one, ws_bytes=64) == E_WORKSPACE
    for layout in (AUTO, DENSE, DIAG, AUTO | REF | XD | XL):                  # an empty batch is a no-op, whatever the pointers
        assert call(B=0, P=None, q=None, x=None, Jq=None, layout=layout) == 0
        assert call(B=0, N=100, P=None, q=None, x=None, Jq=None, layout=layout) == 0
