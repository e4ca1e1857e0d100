"""CPU checks of the smoothed Newton Jacobians' route plan (diffqcqp_amd/csrc/route.cpp: plan_newton_jac_smooth, compiled for the
host behind tests/hostcore/jac_smooth_route_check.cpp) and of the argument rules of dqq_newton_jac_smooth_f64 through both Python
faces of the library: the three families appended with every earlier ordinal where it was; the 64 / 65 boundary and the scratch
size; kappa = 0 giving the parent's plan; a kappa that is negative, a NaN or infinite refused (DQQ_E_BAD_OPTION) after kind, size,
layout and reg, before any pointer, N or the workspace, with B = 0 too; DQQ_F_INFINITE_BOUNDS an unknown bit for every kind; the QP
with Ja.  No compute call is made: every call fails its checks or has B = 0."""
import math

import pytest

import jac_smooth_cases as C

AUTO, DENSE, DIAG = 0, 1, 2
REF, XD, XL, INFB = 0x100, 0x200, 0x400, 0x800
QP, QCQP, BOX, SBOX = 0, 1, 2, 3
E_NULLPTR, E_BAD_SIZE, E_UNSUPPORTED_N, E_BAD_LAYOUT, E_WORKSPACE, E_BAD_OPTION, E_BAD_KIND = -1, -2, -3, -4, -5, -6, -7
BAD_KAPPAS = (-1e-9, -1.0, math.nan, math.inf, -math.inf)
GOOD_KAPPAS = (0.0, 1e-4, 1.0)
# route.h's Family as it stood before the three were appended, None = 0 first
BEFORE = 44


def test_the_three_families_are_appended():
    ids = C.family_ids()
    assert len(ids) == BEFORE + 3 and ids == list(range(BEFORE + 3))     # every earlier ordinal where it was, the three behind them


def _table(kind, N, B, layout, reg, kappa):
    """The route table in Python: (err, family, route, scratch, reg, smooth, inf_bounds)."""
    none = lambda err: (err, 0, 0, 0, 0, 0, 0)     # noqa: E731
    if kind not in (QP, QCQP, BOX, SBOX):
        return none(E_BAD_KIND)
    if B < 0 or B >= 2 ** 31 or N < 1 or (kind == QCQP and N % 2):
        return none(E_BAD_SIZE)
    if (layout & 0xff) not in (AUTO, DENSE, DIAG) or layout & ~(0xff | REF | XD | XL):
        return none(E_BAD_LAYOUT)
    if not (0.0 <= reg < math.inf):
        return none(E_BAD_SIZE)
    if not (0.0 <= kappa < math.inf):
        return none(E_BAD_OPTION)
    if B == 0:
        return none(0)
    smooth = kappa != 0.0
    first = BEFORE if smooth else 26       # NewtonJacDiag (tests/test_jac_routes.py pins it behind NewtonAny)
    if (layout & 0xff) == DIAG:
        return (0, first, 1, 0, int(reg != 0.0), int(smooth), 0) if N in (2, 4, 8, 16, 32, 64) else none(E_UNSUPPORTED_N)
    return (0, first + 2, 3, 1, int(reg != 0.0), int(smooth), 0) if N > 64 else (0, first + 1, 2, 0, int(reg != 0.0), int(smooth), 0)


def test_plan_is_the_table():
    for kind in (-1, QP, QCQP, BOX, SBOX, 4):
        for N in (0, 1, 2, 3, 4, 6, 8, 16, 20, 32, 63, 64, 65, 66, 200):
            for layout in (AUTO, DENSE, DIAG, 7, DENSE | REF | XD | XL, DIAG | INFB, AUTO | INFB):
                for B in (-1, 0, 1, 67, 10 ** 6):
                    for reg in (0.0, 1e-3, -1.0):
                        for kappa in (0.0, 1e-2, -1.0, math.nan):
                            got = C.plan(kind, N, B, layout, reg, kappa)
                            assert got == _table(kind, N, B, layout, reg, kappa), (kind, N, layout, B, reg, kappa, got)


def test_the_team_families_end_at_64_and_the_scratch_is_the_parents():
    for kind in (QP, QCQP, BOX, SBOX):
        assert C.plan(kind, 64, 5, DENSE)[1:4] == (BEFORE + 1, 2, 0) and C.plan(kind, 66, 5, DENSE)[1:4] == (BEFORE + 2, 3, 1)
        assert C.plan(kind, 64, 5, DIAG)[1:4] == (BEFORE, 1, 0)
    assert C.plan(QP, 65, 5, AUTO)[1:4] == (BEFORE + 2, 3, 1)


def test_kappa_zero_is_the_parents_plan():
    for kind in (QP, QCQP, BOX, SBOX):
        for N in (2, 6, 8, 64, 66):
            for layout in (AUTO, DENSE, DIAG, DENSE | REF):
                for reg in (0.0, 1e-3):
                    for B in (0, 5):
                        for zero in (0.0, -0.0):
                            assert C.plan(kind, N, B, layout, reg, zero) == C.plan_reg(kind, N, B, layout, reg)
    # but for the flag: one rule per entry
    assert C.plan(BOX, 8, 5, DENSE | INFB, 0.0, 0.0)[0] == E_BAD_LAYOUT and C.plan_reg(BOX, 8, 5, DENSE | INFB, 0.0)[0] == 0


@pytest.fixture(scope="module", params=["ctypes", "pybind11"])
def lib(request):
    from diffqcqp_amd import build, _capi
    build.build()
    assert "dqq_newton_jac_smooth_f64" in _capi.SIGNATURES
    if request.param == "ctypes":
        return _capi.ctypes_lib()
    mod = _capi.pybind_lib()
    assert mod is not None, "the pybind11 module was not built"
    return mod


one = 8   # a pointer as a Python int, never dereferenced: the checks fail first


def _call(lib):
    def call(kind=0, P=one, q=one, a=None, b=None, c=None, x=one, Jq=one, Ja=None, Jb=None, B=4, N=8, layout=0, reg=0.0, kappa=1e-2,
             ws=None, ws_bytes=0):
        return lib.dqq_newton_jac_smooth_f64(kind, P, q, a, b, c, x, Jq, Ja, Jb, B, N, layout, reg, kappa, None, ws, ws_bytes, None)
    return call


def test_bad_kappa_is_refused_before_anything_but_kind_size_layout_and_reg(lib):
    call = _call(lib)
    for k in BAD_KAPPAS:
        assert call(kappa=k, P=None) == E_BAD_OPTION and call(kappa=k, N=6, layout=DIAG) == E_BAD_OPTION
        assert call(kappa=k, Jq=None) == E_BAD_OPTION and call(kappa=k, Ja=one) == E_BAD_OPTION
        assert call(kappa=k, N=72) == E_BAD_OPTION and call(kappa=k, B=0) == E_BAD_OPTION and call(kappa=k, kind=1) == E_BAD_OPTION
        assert call(kappa=k, kind=4) == E_BAD_KIND and call(kappa=k, layout=7) == E_BAD_LAYOUT and call(kappa=k, B=-1) == E_BAD_SIZE
        assert call(kappa=k, reg=-1.0) == E_BAD_SIZE and call(kappa=k, reg=math.inf, P=None) == E_BAD_SIZE
        assert call(kappa=k, kind=2, a=one, b=one, layout=INFB) == E_BAD_LAYOUT


def test_infinite_bounds_flag_is_an_unknown_bit(lib):
    call = _call(lib)
    for k in GOOD_KAPPAS:
        for kind, ex in ((0, {}), (1, dict(a=one, b=one)), (2, dict(a=one, b=one)), (3, dict(a=one, b=one, c=one))):
            assert call(kind=kind, kappa=k, layout=INFB, **ex) == E_BAD_LAYOUT
            assert call(kind=kind, kappa=k, layout=DIAG | INFB, B=0, **ex) == E_BAD_LAYOUT
            assert call(kind=kind, kappa=k, layout=DENSE | REF, B=0, **ex) == 0        # the flags every entry knows stay known


def test_the_parents_order_otherwise_and_the_argument_order(lib):
    """Every argument in its place: each check below fails on exactly the argument named, so a face that shifted one would answer
    something else."""
    call = _call(lib)
    for k in GOOD_KAPPAS:
        kw = dict(kappa=k)
        assert call(kind=4, N=0, **kw) == E_BAD_KIND and call(B=-1, layout=7, **kw) == E_BAD_SIZE
        assert call(kind=1, N=7, a=one, b=one, **kw) == E_BAD_SIZE and call(N=0, P=None, **kw) == E_BAD_SIZE
        assert call(layout=7, P=None, **kw) == E_BAD_LAYOUT and call(reg=-1e-7, P=None, **kw) == E_BAD_SIZE
        assert call(P=None, **kw) == E_NULLPTR and call(q=None, **kw) == E_NULLPTR and call(x=None, **kw) == E_NULLPTR
        assert call(Jq=None, **kw) == E_NULLPTR and call(kind=2, a=one, b=one, Jq=None, N=65, **kw) == E_NULLPTR    # nothing requested
        assert call(kind=1, **kw) == E_NULLPTR and call(kind=2, a=one, **kw) == E_NULLPTR and call(kind=3, a=one, b=one, **kw) == E_NULLPTR
        assert call(Ja=one, **kw) == E_NULLPTR and call(Jb=one, **kw) == E_NULLPTR                 # the QP has no extras to move
        assert call(N=6, layout=DIAG, Jq=None, **kw) == E_NULLPTR and call(N=6, layout=DIAG, **kw) == E_UNSUPPORTED_N
        assert call(N=65, **kw) == E_WORKSPACE and call(N=65, x=None, **kw) == E_NULLPTR            # the workspace last
        assert call(kind=2, a=one, b=one, Jq=None, Ja=one, N=66, ws=one, ws_bytes=64, **kw) == E_WORKSPACE
        assert call(kind=2, a=one, b=one, Jq=None, Jb=one, N=66, ws=one, ws_bytes=64, **kw) == E_WORKSPACE
        for layout in (AUTO, DENSE, DIAG, AUTO | REF | XD | XL):                  # an empty batch is a no-op, whatever the pointers
            assert call(B=0, P=None, q=None, x=None, Jq=None, layout=layout, **kw) == 0
            assert call(B=0, N=100, P=None, q=None, x=None, Jq=None, layout=layout, **kw) == 0
    # reg and kappa are where the header puts them: reg first
    assert call(reg=-1.0, kappa=1e-2) == E_BAD_SIZE and call(reg=1e-2, kappa=-1.0) == E_BAD_OPTION
