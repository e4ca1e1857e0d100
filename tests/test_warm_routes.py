"""CPU checks of the warm-started forward (dqq_fwd_warm_f64) that need no GPU:

  * route.cpp: plan_fwd_warm equals plan_fwd -- family, lanes per problem, fused / drained, work-list, scratch, counters -- for
    every forward (kind, N, B, layout, knobs) of tests/test_routes.py:TABLE and of tests/param_cases.py, in the shipped and in
    the developer build.  Documented fallbacks would be the only exceptions: every forward family has a warm form today
    (DESIGN.md section 3), so there are none, and the test says so;
  * the argument errors of the entry point, through both bindings (DQQ_E_BAD_KIND first, then the cold forward's);
  * the warm prologues compiled for the host (tests/hostcore/warm_check.cpp): the diagonal path's (admm_core.h) against the
    first iteration of tests/warm_reference.py, and the lane-per-problem kernel's start state (warm_start.h) against the
    restatement's."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import warm_reference as W
from conftest import make_problem
from param_cases import FWD, KIND
from test_routes import KNOBS, SHIPPED, TABLE, render
from warm_cases import extras_of, well_conditioned

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "diffqcqp_amd", "csrc")
FWD_FAMILIES = range(1, 7)   # route.h Family: FwdDiag .. FwdAny


def _build(tuning):
    src = os.path.join(HERE, "hostcore", "warm_check.cpp")
    so = os.path.join(HERE, "hostcore", "libwarm%s.so" % ("_tuning" if tuning else ""))
    deps = [src, os.path.join(ROOT, "include", "diffqcqp_hip.h")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fPIC", "-shared",
                               "-ffp-contract=off", "-fvisibility=hidden"] + (["-DDQQ_TUNING"] if tuning else []) +
                              ["-o", so + ".tmp", src])
        os.replace(so + ".tmp", so)
    lib = ctypes.CDLL(so)
    lib.warm_route_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int,
                                    ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    dp = ctypes.POINTER(ctypes.c_double)
    lib.warm_diag_fwd8.argtypes = [ctypes.c_int] + [dp] * 6 + [ctypes.c_double, ctypes.c_double, ctypes.c_int, dp]
    lib.warm_lane_state8.argtypes = [dp, dp, dp, ctypes.c_double, dp]
    return lib


@pytest.fixture(scope="module")
def host():
    return {False: _build(False), True: _build(True)}


def _plan(lib, warm, kind, N, B, p_layout, **knobs):
    k = dict(SHIPPED, **knobs)
    kn = (ctypes.c_int * 8)(*[k[n] for n in KNOBS])
    out = (ctypes.c_int * 14)()
    lib.warm_route_plan(warm, kind, N, B, p_layout, kn, out)
    return list(out)


def test_every_forward_family_has_a_warm_form(host):
    assert all(host[False].warm_family_built(f) == 1 for f in FWD_FAMILIES)
    assert host[False].warm_family_built(0) == 0 and host[False].warm_family_built(7) == 0   # None, a backward family


def test_warm_plan_is_the_cold_plan(host):
    rows = [(kind, N, B, layout, knobs) for pas, kind, N, B, layout, knobs, _ in TABLE if pas == 0]
    rows += [(KIND[kind], N, B, layout, {}) for _, kind, N, B, layout, _, _ in FWD]
    rows += [(kind, N, 0, layout, {}) for kind in range(4) for N in (8, 24) for layout in (0, 1, 2)]
    assert len(rows) > 100
    seen = set()
    for kind, N, B, layout, knobs in rows:
        tuning = any(SHIPPED[k] != v for k, v in knobs.items())
        cold = _plan(host[tuning], 0, kind, N, B, layout, **knobs)
        warm = _plan(host[tuning], 1, kind, N, B, layout, **knobs)
        assert warm == cold, (kind, N, B, hex(layout), knobs, render(cold), render(warm))
        seen.update((cold[4], cold[9]))
    assert seen >= set(FWD_FAMILIES), "the rows do not reach every forward family"


@pytest.fixture(scope="module", params=["ctypes", "pybind11"])
def lib(request):
    from diffqcqp_amd import build, _capi
    build.build()
    if request.param == "ctypes":
        return _capi.ctypes_lib()
    mod = _capi.pybind_lib()
    assert mod is not None
    return mod


def test_argument_errors(lib):
    one = 8   # a pointer as a Python int, never dereferenced: the checks fail first
    f = lib.dqq_fwd_warm_f64

    def call(kind, P=one, q=one, a=one, b=one, c=one, x0=one, x=one, B=4, N=8, layout=0):
        return f(kind, P, q, a, b, c, x0, x, B, N, 1e-7, 1e-7, 10, 1, layout, None, None, None, None, 0, None)
    assert call(4) == -7 and call(-1) == -7
    assert call(4, B=-1) == -7 and call(7, layout=77) == -7      # DQQ_E_BAD_KIND comes first
    for kind in range(4):
        assert call(kind, B=-1) == -2 and call(kind, N=0) == -2
        assert call(kind, layout=7) == -4 and call(kind, layout=0x800) == -4
        assert call(kind, x0=None) == -1                          # a NULL x0 with B > 0
        assert call(kind, P=None) == -1 and call(kind, q=None) == -1 and call(kind, x=None) == -1
        assert call(kind, B=0, x0=None, P=None) == 0              # an empty batch: no launch, nothing looked at
        assert call(kind) == -5                                   # DQQ_P_AUTO needs the workspace
        assert call(kind, N=80, layout=1) == -5                   # the global-memory kernels: the caller's scratch
        assert call(kind, N=12 if kind == 1 else 7, layout=2) == -3
    assert call(1, N=7) == -2                                     # QCQP: odd N
    assert call(0, a=None, b=None, c=None, x0=None) == -1
    assert call(1, a=None) == -1 and call(2, b=None) == -1 and call(3, c=None) == -1
    assert call(0, a=None, b=None, c=None) == -5                  # a QP has no extras: not missing


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


@pytest.mark.parametrize("kind", ("qp", "qcqp", "box", "sbox"))
def test_diagonal_warm_prologue_on_the_host(host, kind):
    """admm_fwd_diag<KIND, 8, one lane, WARM> against the restatement: max_iter = 0 returns x0 bit for bit; the first iteration
    from a random (infeasible) x0 and the whole solve agree to rounding; a NaN start is a NaN solution."""
    B = 64
    d = make_problem(kind, B, 8, 901, "diag")
    P = well_conditioned(d["P"]).numpy()
    q, ex = d["q"].numpy(), extras_of(kind, d)
    x0 = np.random.default_rng(3).standard_normal(q.shape)
    p = np.ascontiguousarray(np.diagonal(P, axis1=1, axis2=2))
    z = np.zeros(8)

    def run(b, start, max_iter):
        e = [np.ascontiguousarray(a[b].ravel()) for a in ex] + [z] * (3 - len(ex))
        x = np.empty(8)
        it = host[False].warm_diag_fwd8(KIND[kind], _dp(p[b]), _dp(np.ascontiguousarray(q[b].ravel())), _dp(e[0]), _dp(e[1]),
                                        _dp(e[2]), _dp(np.ascontiguousarray(start.ravel())), 1e-7, 1e-7, max_iter, _dp(x))
        return x, it
    for max_iter, tol in ((1, 1e-12), (1000, 1e-6)):
        xr, itr = W.solve(kind, P, q, 1e-7, max_iter, ex, x0=x0)
        got = [run(b, x0[b], max_iter) for b in range(B)]
        xh = np.array([g[0] for g in got]).reshape(B, 8, 1)
        assert np.abs(xh - xr).max() <= tol * max(1.0, np.abs(xr).max())
        assert (np.array([g[1] for g in got]) == itr).mean() >= 0.98
    x, it = run(0, x0[0], 0)
    assert np.array_equal(x, x0[0].ravel()) and it == 0
    bad = x0[1].copy()
    bad[3] = np.nan
    assert np.isnan(run(1, bad, 50)[0]).all()


def test_lane_warm_state_on_the_host(host):
    d = make_problem("qp", 32, 8, 902, "dense")
    P, q = well_conditioned(d["P"]).numpy(), d["q"].numpy().reshape(32, 8)
    x0 = np.random.default_rng(4).standard_normal((32, 8))
    for b in range(32):
        out = np.empty(24)
        assert host[False].warm_lane_state8(_dp(np.ascontiguousarray(P[b])), _dp(np.ascontiguousarray(q[b])),
                                            _dp(np.ascontiguousarray(x0[b])), 1e-7, _dp(out)) == 0
        u = -(W._matvec(P[b:b + 1], x0[b:b + 1]) + q[b:b + 1])[0]       # the restatement's start state
        assert np.array_equal(out[:8], x0[b]) and np.array_equal(out[8:16], u)
        assert np.array_equal(out[16:], q[b] - 1e-7 * x0[b])
    x0[0, 2] = np.inf
    assert host[False].warm_lane_state8(_dp(np.ascontiguousarray(P[0])), _dp(np.ascontiguousarray(q[0])),
                                        _dp(np.ascontiguousarray(x0[0])), 1e-7, _dp(np.empty(24))) == 1
