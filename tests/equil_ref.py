"""numpy restatement of the power-of-two equilibration (diffqcqp_amd/csrc/equil_core.h has the rule; include/diffqcqp_hip.h:
dqq_equilibrate_f64, dqq_unscale_f64), with np.frexp and np.ldexp only -- no log2 -- so that it must give the bits of the host
core and of the device.  Shared by tests/test_equil_hostcore.py, tests/test_equil_oracle.py and tests/test_gpu_equil.py, with
the batch generator, the list of diagonal entries every comparison has to include, and the loader of the host-compiled core
(tests/hostcore/equil_core_check.cpp).

Arrays are float64 numpy: P (B,N,N), or (B,N) with diag; q, x0, the box kinds' extras (B,N); the QCQP's extras (B,N/2)."""
import ctypes
import os
import subprocess

import numpy as np

from check_ref import KIND_ID, KINDS, same_bits  # noqa: F401  (re-exported: the tests import them from here)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MAX_EXP = 255
D = ctypes.POINTER(ctypes.c_double)
I = ctypes.POINTER(ctypes.c_int32)
FAST_N = (2, 4, 8, 16, 32, 64)   # the N DQQ_P_DIAG takes
# The N of the (B,N,N) comparisons (a QCQP takes the even ones).  equil.hip's equil_kernel gives a row 64 lanes of W columns, W = 2
# for an even N and 1 for an odd one, and walks the columns past 64 W in further chunks: 67 is two chunks at W = 1, 129 three, the
# last one column wide, 130 the first even N with a second chunk.
CHUNKED_N = (67, 129, 130)
DENSE_N = (2, 3, 8, 17, 64, 70) + CHUNKED_N


def chunks(N):
    """-> (W, the chunks equil_kernel walks a row in): route.h's check_cols_per_lane and check_lanes, equil.hip's span = L W"""
    W = 2 if N % 2 == 0 else 1
    need, L = (N + W - 1) // W, 1
    while L < need and L < 64:
        L *= 2
    return W, -(-N // (L * W))

_S = float(np.sqrt(0.5))
# what the diagonal of a test batch has to hold: ordinary entries, far ones, clamped ones, the smallest subnormal, the entries
# whose exponent is 0 by rule, and the rounding boundaries -- every power of two near 1 (the odd ones are the ties) and a
# mantissa of sqrt(1/2) (no boundary of this rule: it must round like its neighbours), each with both of its neighbours
SPECIAL = [1.0, 2.0, 0.5, 2.0 ** 40, 2.0 ** -40, 2.0 ** 600, 2.0 ** -600, 5e-324, 0.0, -0.0, -1.0, float("nan"), float("inf"),
           -float("inf"), 3.0, 2.0 ** 510, 2.0 ** 511, 2.0 ** -510, 2.0 ** -511, 2.0 ** 1023, 2.0 ** -1022, 2.0 ** -1030]
for _k in range(-7, 8):
    for _v in (2.0 ** _k, _S * 2.0 ** _k):
        SPECIAL += [_v, float(np.nextafter(_v, 0.0)), float(np.nextafter(_v, np.inf))]
SPECIAL = np.array(SPECIAL)


def exponents(kind, d):
    """e (B,N) int32 from the diagonal d (B,N): equil_core.h's rule."""
    d = np.asarray(d, dtype=np.float64)
    if kind == "qcqp":
        pa, pb = d[:, 0::2], d[:, 1::2]
        d = np.repeat(np.where(pb > pa, pb, pa), 2, axis=1)
    with np.errstate(invalid="ignore"):
        ok = (d > 0.0) & (d <= np.finfo(np.float64).max)
    m, k = np.frexp(np.where(ok, d, 1.0))
    k = k.astype(np.int64)
    n = k >> 1                                             # floor(k / 2)
    n = n - ((m == 0.5) & (k % 2 == 0) & (n % 2 != 0))     # the tie at an odd power of two: the even neighbour
    return np.where(ok, np.clip(-n, -MAX_EXP, MAX_EXP), 0).astype(np.int32)


def equilibrate(kind, P, q, extras, x0=None, diag=False):
    """-> (P~, q~, extras~, x0~ or None, e)."""
    e = exponents(kind, P if diag else np.diagonal(P, axis1=1, axis2=2))
    with np.errstate(all="ignore"):
        Pt = np.ldexp(P, 2 * e) if diag else np.ldexp(P, e[:, :, None] + e[:, None, :])
        qt = np.ldexp(q, e)
        if kind == "qcqp":
            ext = (np.ldexp(extras[0], -e[:, 0::2]), extras[1].copy())
        else:
            ext = tuple(np.ldexp(b, -e) for b in extras[:2]) + tuple(v.copy() for v in extras[2:])
        x0t = None if x0 is None else np.ldexp(x0, -e)
    return Pt, qt, ext, x0t, e


def unscale(y, e):
    with np.errstate(all="ignore"):
        return np.ldexp(y, e)


def make_batch(kind, B, N, seed, diag=False, special=True, inf_bounds=True):
    """A seeded batch (P, q, extras, x0): P = D0 (S S'/N + 0.1 I) D0 with D0 = diag(2^U{-20..20}) (diag: its diagonal);
    special: the entries of SPECIAL written over diagonal entries, cycling from an offset the seed picks, so that the batches of
    a test module together hold all of them; inf_bounds: box kinds with some l_min = -inf and l_max = +inf."""
    r = np.random.default_rng(seed)
    s = np.ldexp(1.0, r.integers(-20, 21, (B, N)))
    S = r.uniform(-1.0, 1.0, (B, N, N))
    P = (S @ S.transpose(0, 2, 1) / N + 0.1 * np.eye(N)) * s[:, :, None] * s[:, None, :]
    if special:
        idx = np.arange(B)[:, None] * N + np.arange(N)[None, :]
        put = r.random((B, N)) < 0.5
        vals = SPECIAL[(idx + seed * 7) % len(SPECIAL)]
        i = np.arange(N)
        P[:, i, i] = np.where(put, vals, P[:, i, i])
    if diag:
        P = np.ascontiguousarray(np.diagonal(P, axis1=1, axis2=2))
    q = r.uniform(-1.0, 1.0, (B, N)) * s
    x0 = r.uniform(-1.0, 1.0, (B, N)) / s
    if kind == "qp":
        extras = ()
    elif kind == "qcqp":
        extras = (r.uniform(0.0, 1.0, (B, N // 2)), r.uniform(0.0, 1.0, (B, N // 2)))
    else:
        lo, hi = -0.6 * r.uniform(0.5, 1.5, (B, N)) / s, 0.6 * r.uniform(0.5, 1.5, (B, N)) / s
        if inf_bounds:
            lo[r.random((B, N)) < 0.2] = -np.inf
            hi[r.random((B, N)) < 0.2] = np.inf
        extras = (lo, hi)
        if kind == "sbox":
            v = r.uniform(-1.0, 1.0, (B, N))
            v[:, 0] = 0.0
            extras += (v,)
    return P, q, extras, x0


def same_problem(got, want):
    """None if (P~, q~, extras~, x0~, e) agree bit for bit (any NaN equals any NaN), else what differs."""
    names = ("P", "q", "extras", "x0", "e")
    for name, g, w in zip(names, got, want):
        if name == "extras":
            if len(g) != len(w) or not all(same_bits(a, b) for a, b in zip(g, w)):
                return "extras"
        elif name == "e":
            if not (g.dtype == w.dtype == np.int32 and np.array_equal(g, w)):
                return "e"
        elif (g is None) != (w is None) or (g is not None and not same_bits(g, w)):
            return name
    return None


def hostcore():
    """The host-compiled core (tests/hostcore/equil_core_check.cpp over diffqcqp_amd/csrc/equil_core.h)."""
    src = os.path.join(HERE, "hostcore", "equil_core_check.cpp")
    so = os.path.join(HERE, "hostcore", "libequilcore.so")
    csrc = os.path.join(ROOT, "diffqcqp_amd", "csrc")
    deps = [src, os.path.join(csrc, "equil_core.h"), os.path.join(csrc, "common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fvisibility=hidden",
                               "-Wall", "-Werror", "-o", so + ".tmp", src])
        os.replace(so + ".tmp", so)
    lib = ctypes.CDLL(so)
    lib.hostequil.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int] + [D] * 12 + [I]
    lib.hostequil.restype = ctypes.c_int
    lib.hostequil_exp.argtypes = [D, ctypes.c_int, I]
    lib.hostunscale.argtypes = [D, I, ctypes.c_int, D]
    return lib


def host_equilibrate(lib, kind, P, q, extras, x0=None, diag=False):
    """The host core over a batch, one problem at a time -> (P~, q~, extras~, x0~, e) as equilibrate()."""
    B, N = q.shape
    P, q = np.ascontiguousarray(P, dtype=np.float64), np.ascontiguousarray(q, dtype=np.float64)
    ex = [np.ascontiguousarray(a, dtype=np.float64) for a in extras] + [None] * (3 - len(extras))
    x0 = None if x0 is None else np.ascontiguousarray(x0, dtype=np.float64)
    Pt, qt, e = np.full_like(P, np.nan), np.full_like(q, np.nan), np.full((B, N), -999, dtype=np.int32)
    ext = [None if a is None else np.full_like(a, np.nan) for a in ex]
    x0t = None if x0 is None else np.full_like(x0, np.nan)
    p = lambda a, b: None if a is None else a[b].ctypes.data_as(D)
    for b in range(B):
        rc = lib.hostequil(KIND_ID[kind], int(diag), N, p(P, b), p(q, b), p(ex[0], b), p(ex[1], b), p(ex[2], b), p(x0, b),
                           p(Pt, b), p(qt, b), p(ext[0], b), p(ext[1], b), p(ext[2], b), p(x0t, b), e[b].ctypes.data_as(I))
        assert rc == 0
    return Pt, qt, tuple(a for a in ext if a is not None), x0t, e


def host_exponents(lib, d):
    d = np.ascontiguousarray(d, dtype=np.float64).ravel()
    e = np.full(d.size, -999, dtype=np.int32)
    lib.hostequil_exp(d.ctypes.data_as(D), d.size, e.ctypes.data_as(I))
    return e


def host_unscale(lib, y, e):
    y, e = np.ascontiguousarray(y, dtype=np.float64), np.ascontiguousarray(e, dtype=np.int32)
    x = np.full_like(y, np.nan)
    lib.hostunscale(y.ctypes.data_as(D), e.ctypes.data_as(I), y.size, x.ctypes.data_as(D))
    return x
