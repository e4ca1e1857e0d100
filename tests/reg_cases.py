"""Inputs and host-side yardsticks of the proximal-weight tests -- tests/test_reg_*.py on the CPU, tests/test_gpu_reg.py on the
device.  Not a test file.  Problems: P only positive semidefinite with a singular free block, built as newton_cases.agree_problem
builds its batches -- z chosen per coordinate (contact) with a margin, x = PI(z), q = x - z - P x -- so that x is a solution
whatever the rank of P.  The yardstick of the kernels is the host core (tests/hostcore/reg_core_check.cpp: csrc/polish_core.h and
csrc/newton_core.h on one CPU thread, loaded through ctypes), itself held bit-equal to the numpy restatement
tests/reg_reference.py."""
import ctypes
import functools
import os
import subprocess

import numpy as np

import polish_reference as R
from polish_cases import DENSE, DIAG

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ("qp", "qcqp", "box", "sbox")
REGS = (1e-10, 1e-7, 1e-2)          # the weights every bit-equality test runs; 0 beside them where the parents are the yardstick
REG = 1e-7                          # the weight of the property tests: the reference-order derivatives' Tikhonov weight
MODES = ("lowrank", "duprow", "diagzero")
B = 37                              # ragged against every tile size
MARGIN = 0.2                        # newton_cases.AGREE_MARGIN: how far z is from a bound / a disc's rim, of the width / radius
# (family, N, B, mode, layout) of tests/test_gpu_reg.py: the diagonal form at N = 2 and 8, teams of 8, a team that does not fill
# its wave share, one wave with a full LDS slice, the any-N form on scratch; the exact-zero pivot on a dense P; then the diagonal
# form's other compiled N (diag_tile.h) -- 9 (128/N) + 1 problems: a last wave with one valid problem -- and the teams of 16
ROWS = [("diag", 2, 37, "diagzero", DIAG), ("diag", 8, 37, "diagzero", DIAG), ("team", 8, 37, "lowrank", DENSE),
        ("team", 20, 37, "lowrank", DENSE), ("team", 64, 37, "lowrank", DENSE), ("any", 72, 5, "lowrank", DENSE),
        ("team", 8, 37, "duprow", DENSE), ("team", 20, 37, "duprow", DENSE),
        ("diag", 4, 289, "diagzero", DIAG), ("diag", 16, 73, "diagzero", DIAG), ("diag", 32, 37, "diagzero", DIAG),
        ("diag", 64, 37, "diagzero", DIAG), ("team", 12, 37, "lowrank", DENSE)]
ENTRIES = ("polish_reg", "bwd_reg", "jvp_reg", "jac_reg")     # what gpu_all of the device test runs on every row, at REGS and 0
_D = ctypes.POINTER(ctypes.c_double)
_I = ctypes.POINTER(ctypes.c_int)

# ---- records (measured by tests/test_reg_reference.py, which holds them) ------------------------------------------------------
# What the unregularised restatement does on each singular batch of CPU_BATCHES: "status1" -- every problem ends with status 1
# (an exactly zero pivot); "huge" -- at least one problem passes the pivot test with status 0 and max |dx| > 1e8; "mixed" -- both
# occur in the batch.  The gap `reg` closes.  As measured: the rank-deficient P = A'A passes the pivot test with numbers of size
# 1e16, the duplicated pair and the exact zeros of a diagonal P end with status 1.
GAP_AT_ZERO = {(k, N, m): "huge" if m == "lowrank" else "status1" for k in KINDS for N in (8, 20) for m in MODES}
# The largest relative adjoint gap (jvp_cases.adjoint_gap) of the restatement's two modes at REG over CPU_BATCHES, per kind, to
# two digits.  Both modes eliminate M_reg, once plain and once transposed: rounding times the elimination's growth, which on a
# singular free block is of the order |P| / reg.  The device tests allow 10 x the record (newton_cases.ADJOINT_GAP_CPU's rule).
# As measured the gap sits at 1e-10 on the rank-deficient batches, where |dx| reaches 1e7 and the two sides cancel, and at 1e-16 on
# the others.
ADJOINT_GAP_CPU = {"qp": 8.9e-11, "qcqp": 1.8e-10, "box": 1.2e-10, "sbox": 2.2e-10}
# How many of the 3 x B problems of a kind's three N = 8 batches (POLISH_BATCHES) the regularised polish (REG) brings to
# r <= 64 x 2.8e-16 of the check's scale from the oracle's forward at eps = 1e-3, within 8 and within 32 steps, as measured (the
# rate is linear; nothing was promised).  One signed box problem stops at r = 6.1e-4 on a rejected step.  Without the weight the
# same starts reach it on 49, 5, 16 and 50 problems; the others end with status 1.
POLISH_REACHED = {"qp": (111, 111), "qcqp": (111, 111), "box": (111, 111), "sbox": (110, 110)}
POLISH_BATCHES = [(8, m) for m in MODES]
POLISH_BAR = 64 * 2.8e-16
# The largest relative difference (newton_cases.agreement: max |newton - oracle| / max |oracle| over a problem's gradients, then
# over the batch) between the oracle's backward (epsilon 1e-10, its Tikhonov iterate of weight 1e-7) and the restatement's Newton
# backward at REG, at the same x, over the three N = 8 singular margin batches of a kind (AGREE_BATCHES), as measured, to two
# digits.  A measurement of two different regularisations, not a bar: for a seeded N(0,1) cotangent, which has a component outside
# the range of the singular free block, M_reg answers with |g| / reg (gradients of size 1e7) where the oracle's refined Tikhonov
# iterate stays at size 1 to 1e3 -- the two differ by their whole size, 1e7 to 1e8 relative to the oracle.
AGREE_REG_CPU = {"qp": 1.6e8, "qcqp": 2.3e7, "box": 2.4e7, "sbox": 3.8e7}
# ... and the same figure for the cotangents the unregularised system has a solution for (range_cotangent: g_F = P_FF s): there
# the two regularisations agree, worst on the rank-deficient P = A'A.
AGREE_REG_RANGE_CPU = {"qp": 4.6e-5, "qcqp": 3.6e-4, "box": 5.4e-4, "sbox": 2.3e-5}
AGREE_BATCHES = [(8, m) for m in MODES]


def _gram(A):
    """A'A with every sum taken in index order (no BLAS: the same bits on every host)."""
    G = np.zeros((A.shape[1], A.shape[1]))
    for k in range(A.shape[0]):
        G = G + A[k][:, None] * A[k][None, :]
    return G


def _rows(P, x):
    """P x per problem, in index order."""
    s = np.zeros(x.shape)
    for j in range(x.shape[1]):
        s = s + P[:, :, j] * x[:, j:j + 1]
    return s


def ne_of(kind, N):
    return 0 if kind == "qp" else (N // 2 if kind == "qcqp" else N)


def lowrank_rows(N):
    """Rows of A in P = A'A / rows: 5 x 8, 12 x 20, and five eighths of N elsewhere (at least 1)."""
    return {8: 5, 20: 12}.get(N, max(1, (5 * N) // 8))


@functools.lru_cache(maxsize=None)
def batch(kind, N, mode, B=B):
    """-> dict: P (B,N,N), pdiag (B,N) for mode "diagzero" (P is diagonal) else None, q (B,N), ex (tuple of (B,.)), x (B,N) the
    solution, free (B,N) bool: the coordinates with D_ii = 1 (QCQP: of contacts inside their disc).  Active elements: a quarter
    ("lowrank": the free block must outgrow the rank) or half of the coordinates / contacts."""
    seed = 97000 + 1000 * R.KIND[kind] + 10 * N + MODES.index(mode)
    r = np.random.default_rng(seed)
    nel = N // 2 if kind == "qcqp" else N
    nact = nel // 4 if mode == "lowrank" else nel // 2
    active = r.permuted(np.tile(np.arange(nel) < nact, (B, 1)), axis=1)
    free_c = np.repeat(~active, 2, axis=1) if kind == "qcqp" else ~active
    P = np.zeros((B, N, N))
    pdiag = None
    for b in range(B):
        fc = np.nonzero(free_c[b])[0]
        if mode == "lowrank":
            A = r.standard_normal((lowrank_rows(N), N))
            P[b] = _gram(A) / A.shape[0]
        elif mode == "duprow":      # coordinate j is a copy of coordinate i, both free: rows / columns i and j of P are equal
            G = r.standard_normal((N - 1, N - 1))
            P0 = _gram(G) / (N - 1) + 0.5 * np.eye(N - 1)
            i, j = int(fc[0]), int(fc[-1])
            src = np.array([c - (c > j) for c in range(N)])   # P0's index of every coordinate but j ...
            src[j] = src[i]                                   # ... which reads i's: no arithmetic, the pair is equal bit for bit
            P[b] = P0[np.ix_(src, src)]
        else:                        # exact zeros on every other free coordinate (QCQP: free contact), the first one included
            d = r.uniform(0.5, 2.0, N)
            fe = np.nonzero(~active[b])[0][::2]
            d[np.concatenate([2 * fe, 2 * fe + 1]) if kind == "qcqp" else fe] = 0.0
            P[b] = np.diag(d)
    if mode == "diagzero":
        pdiag = np.ascontiguousarray(np.einsum("bii->bi", P))
    m = MARGIN
    if kind == "qcqp":
        nc = N // 2
        ln, mu = r.uniform(0.5, 1.5, (B, nc)), r.uniform(0.3, 1.0, (B, nc))
        rad = ln * mu
        nrm = rad * np.where(active, r.uniform(1 + m, 3.0, (B, nc)), r.uniform(0.1, 1 - m, (B, nc)))
        phi = r.uniform(0.0, 2 * np.pi, (B, nc))
        z = np.stack([nrm * np.cos(phi), nrm * np.sin(phi)], axis=2).reshape(B, N)
        ex = (ln, mu)
    else:
        if kind == "qp":
            lo, w, hi, ex = np.zeros((B, N)), np.ones((B, N)), np.full((B, N), R.INF), ()
        else:
            ex = (-r.uniform(0.3, 1.0, (B, N)), r.uniform(0.3, 1.0, (B, N)))
            if kind == "sbox":
                ex += (r.choice([-1.0, 1.0], (B, N)) * r.uniform(0.2, 1.0, (B, N)),)
            lo, hi = (np.stack(a) for a in zip(*(R.effective_bounds(kind, tuple(e[b] for e in ex), N) for b in range(B))))
            w = hi - lo
        below = r.random((B, N)) < 0.5 if kind != "qp" else np.ones((B, N), dtype=bool)
        out = r.uniform(m, 1.0, (B, N)) * w
        inside = lo + r.uniform(m, 1 - m, (B, N)) * w if kind != "qp" else r.uniform(m, 1.0, (B, N))
        z = np.where(active, np.where(below, lo - out, np.where(np.isfinite(hi), hi, 0.0) + out), inside)
    x = np.stack([R.project(kind, z[b], tuple(e[b] for e in ex), N) for b in range(B)])
    q = x - z - _rows(P, x)
    d = {"P": P, "pdiag": pdiag, "q": np.ascontiguousarray(q), "ex": tuple(np.ascontiguousarray(e) for e in ex),
         "x": np.ascontiguousarray(x), "free": free_c}
    for a in (P, d["q"], d["x"]) + d["ex"]:
        a.setflags(write=False)
    return d


# the batches of the CPU property tests: every kind and mode at N = 8, the dense modes at N = 20 too
CPU_BATCHES = [(k, N, m) for k in KINDS for N in (8, 20) for m in MODES if not (N == 20 and m == "diagzero")]


def inputs(kind, N, B, seed=0):
    """-> (tangents (dP (B,N,N), dq[, da, db]), g (B,N)): seeded."""
    import jvp_reference as JR
    s = 99000 + 1000 * R.KIND[kind] + 10 * N + 7 * seed
    return JR.random_tangents(kind, B, N, s), np.random.default_rng(s + 1).standard_normal((B, N))


def range_cotangent(d, g):
    """g with its free part replaced by P_FF s, s the free part of g: a cotangent the unregularised backward has a solution for
    (rows in index order, no BLAS)."""
    out = g.copy()
    for b in range(g.shape[0]):
        f = np.nonzero(d["free"][b])[0]
        Pff, acc = d["P"][b][np.ix_(f, f)], np.zeros(f.size)
        for j in range(f.size):
            acc = acc + Pff[:, j] * g[b, f[j]]
        out[b, f] = acc
    return out


def free_rank(d, b):
    """(rank of the free block of problem b, its size)"""
    f = np.nonzero(d["free"][b])[0]
    return int(np.linalg.matrix_rank(d["P"][b][np.ix_(f, f)])), f.size


# ---- the host core ------------------------------------------------------------------------------------------------------------
_DEPS = ("newton_core.h", "polish_core.h", "check_core.h", "sbox_bounds.h", "common.h")


@functools.lru_cache(maxsize=None)
def hostcore():
    """The host core as a shared library, built on demand (plain: the yardstick of the device tests too)."""
    src = os.path.join(HERE, "hostcore", "reg_core_check.cpp")
    so = os.path.join(HERE, "hostcore", "libregcheck.so")
    deps = [src] + [os.path.join(HERE, "..", "diffqcqp_amd", "csrc", f) for f in _DEPS]
    if not os.path.exists(so) or any(os.path.getmtime(p) > os.path.getmtime(so) for p in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fvisibility=hidden",
                               "-Wno-unknown-pragmas", "-o", so + ".tmp", src])
        os.replace(so + ".tmp", so)
    return ctypes.CDLL(so)


def hostcore_program():
    """The same file as a stand-alone program with the address and undefined-behaviour sanitizers -- CPU tests only."""
    src = os.path.join(HERE, "hostcore", "reg_core_check.cpp")
    exe = os.path.join(HERE, "hostcore", "reg_core_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                           "-ffp-contract=off", "-Wno-unknown-pragmas", "-DREG_CHECK_MAIN", "-o", exe, src])
    return exe


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return None if a is None else a.ctypes.data_as(_D)


def _head(kind, P, q, ex, x, diag):
    Bn, N = x.shape
    P, q, x = _c(P), _c(q), _c(x)
    assert P.shape == ((Bn, N) if diag else (Bn, N, N))
    ex = [_c(e) for e in ex] + [None] * (3 - len(ex))
    return Bn, N, P, q, ex, x


def host_polish(kind, P, q, ex, x, max_steps=8, reg=0.0, diag=False, inf_ok=False):
    """-> (x_out (B,N), resid (B,2), steps (B) int32, status (B) int32)"""
    Bn, N, P, q, ex, x = _head(kind, P, q, ex, x, diag)
    xo, rs = np.full((Bn, N), 7.0), np.full((Bn, 2), 7.0)
    st, ss = np.full(Bn, -1, dtype=np.int32), np.full(Bn, -1, dtype=np.int32)
    rc = hostcore().reg_polish_batch(R.KIND[kind], Bn, N, int(diag), int(inf_ok), ctypes.c_double(reg), int(max_steps), _p(P), _p(q),
                                     _p(ex[0]), _p(ex[1]), _p(ex[2]), _p(x), _p(xo), _p(rs), st.ctypes.data_as(_I),
                                     ss.ctypes.data_as(_I))
    assert rc == 0
    return xo, rs, st, ss


def host_jvp(kind, P, q, ex, x, tangents=(), reg=0.0, diag=False, inf_ok=False):
    """tangents (dP (as P), dq[, da, db]), None = NULL -> (dx (B,N), status (B) int32)"""
    Bn, N, P, q, ex, x = _head(kind, P, q, ex, x, diag)
    t = [_c(v) for v in tuple(tangents) + (None,) * (4 - len(tangents))]
    dx, st = np.full((Bn, N), 7.0), np.full(Bn, -1, dtype=np.int32)
    rc = hostcore().reg_jvp_batch(R.KIND[kind], Bn, N, int(diag), int(inf_ok), ctypes.c_double(reg), _p(P), _p(q), _p(ex[0]),
                                  _p(ex[1]), _p(ex[2]), _p(x), _p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), _p(dx), st.ctypes.data_as(_I))
    assert rc == 0
    return dx, st


def host_backward(kind, P, q, ex, x, gx, reg=0.0, diag=False, inf_ok=False):
    """-> (grad_P (as P), grad_q (B,N), grad_a, grad_b (B,.) or None for the QP, status (B) int32)"""
    Bn, N, P, q, ex, x = _head(kind, P, q, ex, x, diag)
    ne = ne_of(kind, N)
    gP, gq = np.full(P.shape, 7.0), np.full((Bn, N), 7.0)
    ga, gb = (np.full((Bn, ne), 7.0), np.full((Bn, ne), 7.0)) if ne else (None, None)
    st = np.full(Bn, -1, dtype=np.int32)
    rc = hostcore().reg_bwd_batch(R.KIND[kind], Bn, N, int(diag), int(inf_ok), ctypes.c_double(reg), _p(P), _p(q), _p(ex[0]),
                                  _p(ex[1]), _p(ex[2]), _p(x), _p(_c(gx)), _p(gP), _p(gq), _p(ga), _p(gb), st.ctypes.data_as(_I))
    assert rc == 0
    return gP, gq, ga, gb, st


def jac_shapes(kind, Bn, N, diag):
    """(Jq, Ja, Jb) as include/diffqcqp_hip.h has them"""
    if diag:
        return ((Bn, N, 2) if kind == "qcqp" else (Bn, N), (Bn, N), (Bn, N))
    return ((Bn, N, N), (Bn, N, ne_of(kind, N)), (Bn, N, ne_of(kind, N)))


def host_jacobian(kind, P, q, ex, x, reg=0.0, diag=False, inf_ok=False):
    """-> (Jq, Ja, Jb (None for the QP), status (B) int32)"""
    Bn, N, P, q, ex, x = _head(kind, P, q, ex, x, diag)
    sq, sa, sb = jac_shapes(kind, Bn, N, diag)
    Jq = np.full(sq, 7.0)
    Ja, Jb = (np.full(sa, 7.0), np.full(sb, 7.0)) if kind != "qp" else (None, None)
    st = np.full(Bn, -1, dtype=np.int32)
    rc = hostcore().reg_jac_batch(R.KIND[kind], Bn, N, int(diag), int(inf_ok), ctypes.c_double(reg), _p(P), _p(q), _p(ex[0]),
                                  _p(ex[1]), _p(ex[2]), _p(x), _p(Jq), _p(Ja), _p(Jb), st.ctypes.data_as(_I))
    assert rc == 0
    return Jq, Ja, Jb, st


def same_bits(a, b):
    """Equal as bit patterns but for the payload of a NaN (polish_cases.same_bits); None equals None."""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=True)) and bool(
        np.array_equal(np.signbit(a[~np.isnan(a)]), np.signbit(b[~np.isnan(b)])))


def two_digits(v):
    return float("%.1e" % v)
