"""CPU check of csrc/sbox_bounds.h, the one helper behind every signed box backward kernel: compiled for the host
(tests/hostcore/sbox_bounds_check.cpp) and compared, over a grid, with the forward's own projection
s min(s clamp(t, l_min, l_max), 0), s = sign(v) (Solver.cpp:395-398) -- the effective bounds must describe the same map -- and
with the definition of the keep flags (include/diffqcqp_hip.h: dqq_signedboxqp_bwd_f64).  Values are compared with ==, so
-0.0 and +0.0 are equal.  The host build is a test artefact; the product never calls it."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
D, I = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)

INF, TINY, SUB, HUGE = np.inf, 5e-324, 1.1e-308, 1e300
# bounds: +-inf, huge, ordinary, subnormal (the smallest, and one just below the normal range), both zeros
BOUNDS = [-INF, -HUGE, -2.5, -1.0, -SUB, -TINY, -0.0, 0.0, TINY, SUB, 1.0, 2.5, HUGE, INF]
VS = [-INF, -HUGE, -3.0, -TINY, -0.0, 0.0, TINY, 2.0, HUGE, INF]
# 64 finite values of t: the finite bound values, points between and beyond them, huge and subnormal magnitudes
_T = [b for b in BOUNDS if np.isfinite(b)] + [-1e308, -3.0, -1.75, -0.5, -1e-300, 1e-300, 0.5, 1.75, 3.0, 1e308]
T = np.array(_T + list(np.linspace(-4.0, 4.0, 64 - len(_T))))
assert T.size == 64 and np.isfinite(T).all()


@pytest.fixture(scope="module")
def helper():
    src = os.path.join(HERE, "hostcore", "sbox_bounds_check.cpp")
    so = os.path.join(HERE, "hostcore", "libsboxbounds.so")
    deps = [src] + [os.path.join(HERE, "..", "diffqcqp_amd", "csrc", f) for f in ("sbox_bounds.h", "common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fvisibility=hidden",
                               "-o", so + ".tmp", src])
        os.replace(so + ".tmp", so)
    lib = ctypes.CDLL(so)
    lib.sbox_bounds_many.argtypes = [ctypes.c_long, D, D, D, D, D, I, I]
    lib.sbox_bounds_many.restype = None

    def call(lo, hi, v):
        lo, hi, v = (np.ascontiguousarray(a, dtype=np.float64) for a in (lo, hi, v))
        n = lo.size
        lo_e, hi_e = np.full(n, np.nan), np.full(n, np.nan)
        klo, khi = np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
        lib.sbox_bounds_many(n, lo.ctypes.data_as(D), hi.ctypes.data_as(D), v.ctypes.data_as(D), lo_e.ctypes.data_as(D),
                             hi_e.ctypes.data_as(D), klo.ctypes.data_as(I), khi.ctypes.data_as(I))
        return lo_e, hi_e, klo.astype(bool), khi.astype(bool)
    return call


def grid():
    # l_min <= l_max; a box pinned AT infinity is no problem the forward can solve (0 * inf under v = 0) and is left out
    g = [(lo, hi, v) for lo, hi in itertools.product(BOUNDS, BOUNDS) if lo <= hi and not (lo == hi and np.isinf(lo)) for v in VS]
    lo, hi, v = (np.array(c) for c in zip(*g))
    return lo, hi, v


def test_the_grid_holds_every_case():
    lo, hi, v = grid()
    for name, m in (("v = +0.0", (v == 0) & ~np.signbit(v)), ("v = -0.0", (v == 0) & np.signbit(v)),
                    ("l_min > 0 with v > 0", (lo > 0) & (v > 0)), ("l_max < 0 with v < 0", (hi < 0) & (v < 0)),
                    ("l_min == 0 with v < 0", (lo == 0) & (v < 0)), ("l_max == 0 with v > 0", (hi == 0) & (v > 0)),
                    ("plain, v > 0", (lo < 0) & (hi > 0) & (v > 0)), ("plain, v < 0", (lo < 0) & (hi > 0) & (v < 0)),
                    ("infinite bounds", np.isinf(lo) | np.isinf(hi)), ("subnormal", (np.abs(lo) == TINY) | (np.abs(hi) == SUB)),
                    ("huge", (np.abs(lo) == HUGE) | (np.abs(hi) == HUGE))):
        assert m.sum() >= 4, name


def test_effective_bounds_describe_the_forwards_projection(helper):
    lo, hi, v = grid()
    lo_e, hi_e, _, _ = helper(lo, hi, v)
    assert not np.isnan(lo_e).any() and not np.isnan(hi_e).any() and (lo_e <= hi_e).all()
    s = np.sign(v)[:, None]
    t = T[None, :]
    with np.errstate(invalid="raise", over="raise"):
        clamped = np.minimum(np.maximum(t, lo[:, None]), hi[:, None])          # cwiseMax(l_min), cwiseMin(l_max), :396-397
        want = s * np.minimum(s * clamped, 0.0)                                # v o min(v o l_2, 0), :398
        got = np.minimum(np.maximum(t, lo_e[:, None]), hi_e[:, None])
    bad = np.argwhere(want != got)                                             # as values: -0.0 == +0.0
    assert bad.size == 0, [(lo[i], hi[i], v[i], T[j], want[i, j], got[i, j]) for i, j in bad[:5]]
    # the effective bounds are selected from {l_min, l_max, 0}: nothing is rounded
    assert ((lo_e == lo) | (lo_e == hi) | (lo_e == 0)).all() and ((hi_e == lo) | (hi_e == hi) | (hi_e == 0)).all()


def test_effective_bounds_follow_the_table(helper):
    lo, hi, v = grid()
    lo_e, hi_e, klo, khi = helper(lo, hi, v)
    pos, neg, zero = v > 0, v < 0, v == 0
    hi_p = np.minimum(hi, 0.0)
    assert np.array_equal(hi_e[pos], hi_p[pos]) and np.array_equal(lo_e[pos], np.minimum(lo, hi_p)[pos])
    lo_n = np.maximum(lo, 0.0)
    assert np.array_equal(lo_e[neg], lo_n[neg]) and np.array_equal(hi_e[neg], np.maximum(hi, lo_n)[neg])
    assert (lo_e[zero] == 0).all() and (hi_e[zero] == 0).all()
    # keep flags: the bound gradient belongs to the caller's bound exactly where the effective bound equals it as a value
    assert np.array_equal(klo, lo_e == lo) and np.array_equal(khi, hi_e == hi)
    # ... spelled out for the cases the backward's tests rest on
    m = (lo > 0) & pos                       # the box lies on the wrong side: x = 0, neither bound is the caller's
    assert m.any() and not klo[m].any() and not khi[m].any() and (lo_e[m] == 0).all() and (hi_e[m] == 0).all()
    m = (hi < 0) & neg
    assert m.any() and not klo[m].any() and not khi[m].any() and (lo_e[m] == 0).all() and (hi_e[m] == 0).all()
    m = (lo == 0) & neg                      # ties pass the gradient to the bound (a subgradient choice)
    assert m.any() and klo[m].all()
    m = (hi == 0) & pos
    assert m.any() and khi[m].all()
    m = zero                                 # v = +-0.0: pinned to 0; a bound keeps its gradient only if it is 0 itself
    assert np.array_equal(klo[m], lo[m] == 0) and np.array_equal(khi[m], hi[m] == 0)
    m = (lo < 0) & (hi > 0)                  # plain coordinates: the sign constraint replaces the bound on its side only
    assert klo[m & pos].all() and not khi[m & pos].any() and khi[m & neg].all() and not klo[m & neg].any()
    # -0.0 and +0.0 are one value
    a = helper([-0.0, 0.0, -1.0, -1.0], [1.0, 1.0, -0.0, 0.0], [-1.0, -1.0, 1.0, 1.0])
    assert a[2][:2].all() and a[3][2:].all()


def test_a_nan_v_has_no_sign(helper):
    lo_e, hi_e, klo, khi = helper([-1.0, 0.0], [1.0, 2.0], [np.nan, np.nan])
    assert (lo_e == 0).all() and (hi_e == 0).all() and list(klo) == [False, True] and not khi.any()
