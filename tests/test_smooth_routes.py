"""CPU checks of the argument rules of dqq_polish_smooth_f64, dqq_newton_bwd_smooth_f64 and dqq_newton_jvp_smooth_f64 through
both Python faces of the library: a kappa that is negative, a NaN or infinite is DQQ_E_BAD_OPTION where the damped polish refuses
max_halvings -- after kind, size, layout and reg, before any pointer, N or the workspace is looked at, with B = 0 too --;
DQQ_F_INFINITE_BOUNDS is an unknown bit to the three entries for every kind; otherwise the parents' order, at kappa = 0 and
kappa > 0 alike.  No compute call is made: every call fails its checks or has B = 0."""
import math

import pytest

AUTO, DENSE, DIAG = 0, 1, 2
INFB = 0x800
E_NULLPTR, E_BAD_SIZE, E_UNSUPPORTED_N, E_BAD_LAYOUT, E_WORKSPACE, E_BAD_OPTION, E_BAD_KIND = -1, -2, -3, -4, -5, -6, -7
BAD_KAPPAS = (-1e-9, -1.0, math.nan, math.inf, -math.inf)
GOOD_KAPPAS = (0.0, 1e-4, 1.0)


@pytest.fixture(scope="module", params=["ctypes", "pybind11"])
def lib(request):
    from diffqcqp_amd import build, _capi
    build.build()
    for name in ("dqq_polish_smooth_f64", "dqq_newton_bwd_smooth_f64", "dqq_newton_jvp_smooth_f64"):
        assert name in _capi.SIGNATURES
    if request.param == "ctypes":
        return _capi.ctypes_lib()
    mod = _capi.pybind_lib()
    assert mod is not None, "the pybind11 module was not built"
    return mod


one = 8   # a pointer as a Python int, never dereferenced: the checks fail first


def _calls(lib):
    def polish(kind=0, P=one, q=one, a=None, b=None, c=None, x=one, out=one, B=4, N=8, layout=0, reg=0.0, kappa=1e-2, h=8, ws=None, ws_bytes=0):
        return lib.dqq_polish_smooth_f64(kind, P, q, a, b, c, x, out, B, N, 8, layout, reg, kappa, h, None, None, None, None, ws, ws_bytes, None)

    def bwd(kind=0, P=one, q=one, a=None, b=None, c=None, x=one, out=one, B=4, N=8, layout=0, reg=0.0, kappa=1e-2, h=8, ws=None, ws_bytes=0):
        # (`out` plays grad_x, the pointer the mode requires; h has no part)
        return lib.dqq_newton_bwd_smooth_f64(kind, P, q, a, b, c, x, out, one, one, None, None, B, N, layout, reg, kappa, None, ws, ws_bytes, None)

    def jvp(kind=0, P=one, q=one, a=None, b=None, c=None, x=one, out=one, B=4, N=8, layout=0, reg=0.0, kappa=1e-2, h=8, ws=None, ws_bytes=0):
        return lib.dqq_newton_jvp_smooth_f64(kind, P, q, a, b, c, x, one, one, None, None, out, B, N, layout, reg, kappa, None, ws, ws_bytes, None)

    return polish, bwd, jvp


def test_bad_kappa_is_refused_before_anything_but_kind_size_layout_and_reg(lib):
    for call in _calls(lib):
        for k in BAD_KAPPAS:
            assert call(kappa=k, P=None) == E_BAD_OPTION and call(kappa=k, N=6, layout=DIAG) == E_BAD_OPTION
            assert call(kappa=k, N=72) == E_BAD_OPTION and call(kappa=k, B=0) == E_BAD_OPTION and call(kappa=k, kind=1) == E_BAD_OPTION
            assert call(kappa=k, kind=4) == E_BAD_KIND and call(kappa=k, layout=7) == E_BAD_LAYOUT and call(kappa=k, B=-1) == E_BAD_SIZE
            assert call(kappa=k, reg=-1.0) == E_BAD_SIZE and call(kappa=k, reg=math.inf, P=None) == E_BAD_SIZE
            assert call(kappa=k, kind=2, a=one, b=one, layout=INFB) == E_BAD_LAYOUT
    polish = _calls(lib)[0]
    assert polish(h=-1, kappa=-1.0) == E_BAD_OPTION and polish(h=61) == E_BAD_OPTION and polish(h=61, kappa=0.0, B=0) == E_BAD_OPTION


def test_infinite_bounds_flag_is_an_unknown_bit(lib):
    for call in _calls(lib):
        for k in GOOD_KAPPAS:
            for kind, ex in ((0, {}), (1, dict(a=one, b=one)), (2, dict(a=one, b=one)), (3, dict(a=one, b=one, c=one))):
                assert call(kind=kind, kappa=k, layout=INFB, **ex) == E_BAD_LAYOUT
                assert call(kind=kind, kappa=k, layout=DIAG | INFB, B=0, **ex) == E_BAD_LAYOUT
                assert call(kind=kind, kappa=k, layout=DENSE | 0x100, B=0, **ex) == 0        # the flags every entry knows stay known


def test_the_parents_order_otherwise(lib):
    for call in _calls(lib):
        for k in GOOD_KAPPAS:
            kw = dict(kappa=k)
            assert call(kind=4, N=0, **kw) == E_BAD_KIND and call(B=-1, layout=7, **kw) == E_BAD_SIZE
            assert call(kind=1, N=7, a=one, b=one, **kw) == E_BAD_SIZE
            assert call(layout=7, P=None, **kw) == E_BAD_LAYOUT and call(reg=-1e-7, P=None, **kw) == E_BAD_SIZE
            assert call(P=None, **kw) == E_NULLPTR and call(out=None, **kw) == E_NULLPTR and call(kind=1, **kw) == E_NULLPTR
            assert call(kind=3, a=one, b=one, **kw) == E_NULLPTR
            assert call(N=6, layout=DIAG, out=None, **kw) == E_NULLPTR and call(N=6, layout=DIAG, **kw) == E_UNSUPPORTED_N
            assert call(N=72, **kw) == E_WORKSPACE and call(kind=2, a=one, b=one, N=72, ws=one, ws_bytes=64, **kw) == E_WORKSPACE
            assert call(B=0, P=None, q=None, x=None, out=None, **kw) == 0
    _, bwd, jvp = _calls(lib)
    # the QP has no extras to move
    assert lib.dqq_newton_bwd_smooth_f64(0, one, one, None, None, None, one, one, one, one, one, None, 4, 8, 0, 0.0, 1e-2, None, None, 0, None) == E_NULLPTR
    assert lib.dqq_newton_jvp_smooth_f64(0, one, one, None, None, None, one, one, one, one, None, one, 4, 8, 0, 0.0, 1e-2, None, None, 0, None) == E_NULLPTR
