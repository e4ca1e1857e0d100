"""CPU checks of the solution check's plan (diffqcqp_amd/csrc/route.cpp: plan_check, compiled for the host behind
tests/hostcore/check_core_check.cpp) and of the argument checks of dqq_check_f64 through both Python faces of the library.
No compute call is made here."""
import ctypes

import pytest

import check_ref as R

AUTO, DENSE, DIAG = 0, 1, 2
REF, XD, XL = 0x100, 0x200, 0x400
FAM_CHECK, FAM_CHECK_DIAG = 15, 16          # route.h: Family::Check, Family::CheckDiag (behind the 14 solver families)
E_NULLPTR, E_BAD_SIZE, E_BAD_LAYOUT, E_BAD_KIND = -1, -2, -4, -7


@pytest.fixture(scope="module")
def core():
    return R.hostcore()


def plan(core, kind, N, B, p_layout):
    out = (ctypes.c_int * 3)()
    core.hostcheck_plan(kind, N, B, p_layout, out)
    return tuple(out)


def test_every_size_has_a_built_family_and_a_lane_count_that_divides_64(core):
    for kind in range(4):
        for N in range(1, 131):
            if kind == 1 and N % 2:
                assert plan(core, kind, N, 5, AUTO)[0] == E_BAD_SIZE
                continue
            for layout in (AUTO, DENSE, DIAG):
                for flags in (0, REF, XD, XL, REF | XD | XL):
                    err, fam, lanes = plan(core, kind, N, 5, layout | flags)
                    assert err == 0 and fam == (FAM_CHECK_DIAG if layout == DIAG else FAM_CHECK), (kind, N, layout, flags)
                    assert lanes in (1, 2, 4, 8, 16, 32, 64) and 64 % lanes == 0
                    # the instantiated mapping: two columns per lane for even N, one for odd; a row fits the lanes up to 64 of them
                    w = 2 if N % 2 == 0 else 1
                    assert lanes == 64 or (lanes * w >= N and (lanes == 1 or lanes * w < 2 * N)), (N, lanes)
                    assert plan(core, kind, N, 5, layout | flags) == plan(core, kind, N, 10 ** 6, layout | flags)   # B plays no part
    assert plan(core, 0, 8, 5, AUTO)[2] == 4 and plan(core, 0, 2, 5, AUTO)[2] == 1 and plan(core, 0, 3, 5, AUTO)[2] == 4
    assert plan(core, 0, 64, 5, AUTO)[2] == 32 and plan(core, 0, 65, 5, AUTO)[2] == 64 and plan(core, 0, 130, 5, DIAG)[2] == 64


def test_plan_errors_and_the_empty_batch(core):
    assert plan(core, 0, 8, 0, AUTO) == (0, 0, 0)                       # B = 0: nothing to launch
    assert plan(core, 4, 8, 5, AUTO)[0] == E_BAD_KIND and plan(core, -1, 8, 5, AUTO)[0] == E_BAD_KIND
    assert plan(core, 0, 0, 5, AUTO)[0] == E_BAD_SIZE and plan(core, 0, 8, -1, AUTO)[0] == E_BAD_SIZE
    assert plan(core, 0, 8, 2 ** 31, AUTO)[0] == E_BAD_SIZE
    assert plan(core, 0, 8, 5, 3)[0] == E_BAD_LAYOUT and plan(core, 0, 8, 5, 0x800)[0] == E_BAD_LAYOUT
    assert plan(core, 0, 200, 5, DIAG)[0] == 0                           # the compact diagonal at any N


@pytest.fixture(scope="module", params=["ctypes", "pybind11"])
def lib(request):
    from diffqcqp_amd import build, _capi
    build.build()
    assert "dqq_check_f64" in _capi.SIGNATURES
    if request.param == "ctypes":
        return _capi.ctypes_lib()
    mod = _capi.pybind_lib()
    assert mod is not None, "the pybind11 module was not built"
    return mod


def test_both_faces_list_the_symbol_and_check_its_arguments(lib):
    f = lib.dqq_check_f64
    one = 8   # a pointer as a Python int, never dereferenced: the checks fail first

    def call(kind=0, P=one, q=one, a=None, b=None, c=None, x=one, iters=None, max_iter=10, B=4, N=8, layout=0, resid=one,
             status=one, counts=None):
        return f(kind, P, q, a, b, c, x, iters, max_iter, B, N, layout, resid, status, counts, None)

    assert call(kind=4) == E_BAD_KIND and call(kind=-1) == E_BAD_KIND
    assert call(B=-1) == E_BAD_SIZE and call(N=0) == E_BAD_SIZE
    assert call(kind=1, a=one, b=one, N=7) == E_BAD_SIZE                 # odd N for a QCQP
    assert call(layout=7) == E_BAD_LAYOUT and call(layout=0x800) == E_BAD_LAYOUT
    assert call(P=None) == E_NULLPTR and call(q=None) == E_NULLPTR and call(x=None) == E_NULLPTR
    assert call(resid=None, status=None) == E_NULLPTR                    # each may be NULL, not both
    assert call(kind=1) == E_NULLPTR and call(kind=1, a=one) == E_NULLPTR            # l_n, mu
    assert call(kind=2, a=one) == E_NULLPTR                                          # l_min, l_max
    assert call(kind=3, a=one, b=one) == E_NULLPTR                                   # ... and v
    # an empty batch is a no-op, whatever the pointers, in every layout and with every flag
    for layout in (AUTO, DENSE, DIAG, AUTO | REF | XD | XL):
        assert call(B=0, P=None, q=None, x=None, resid=None, status=None, layout=layout) == 0
    from diffqcqp_amd import _capi
    assert -7 in _capi._ERRORS
