"""Inputs and host-side yardsticks of the Newton-derivative tests -- tests/test_newton_*.py on the CPU, tests/test_gpu_newton.py
on the device.  Not a test file.  Problems: polish_cases' well-conditioned batches (spectrum on [0.5, 2]; for the recorded
figures the copies frozen under tests/golden/polish), x the oracle's forward at eps = 1e-3 polished by the numpy restatement of
the polish.  The yardstick of the kernels is the host core
(tests/hostcore/newton_core_check.cpp: csrc/newton_core.h on one CPU thread, loaded through ctypes), itself held bit-equal to the
numpy restatement tests/newton_reference.py."""
import ctypes
import functools
import os
import subprocess

import numpy as np

import jvp_cases as JC
import jvp_reference as JR
import newton_reference as NR
import polish_cases as PC
import polish_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = PC.KINDS
B_CPU = 32
BATCHES = [(k, N, s) for k in KINDS for N in (8, 20) for s in ("diag", "dense")]
# (kind, N, B) of tests/test_gpu_newton.py (both modes run every row); the sizes and ragged_b are polish_cases'
DIAG_ROWS = ([(k, N, B) for k in KINDS for N in PC.DIAG_N_FIRST for B in (1, 67)] +
             [(k, N, PC.ragged_b(N)) for k in KINDS for N in PC.DIAG_N_MORE])
TEAM_ROWS = [("qp", 3, 37), ("box", 3, 37), ("sbox", 3, 37)] + [(k, N, 37) for k in KINDS for N in (8, 20, 64)] + [(k, PC.TEAM_N16, 37) for k in KINDS]
ANY_ROWS = [(k, 66, 5) for k in KINDS]
ENTRIES = ("bwd", "jvp")                 # check_family of the device test runs both modes on every row
TEAM_LAYOUTS = PC.TEAM_LAYOUTS
_D = ctypes.POINTER(ctypes.c_double)
_I = ctypes.POINTER(ctypes.c_int)

# The largest relative adjoint gap |<g, dx> - sum <grad, tangent>| / sum |terms| (jvp_cases.adjoint_gap: exactly rounded sums) of
# the numpy restatement's two modes over BATCHES (B_CPU problems each), per kind, as measured, to two digits:
# tests/test_newton_reference.py measures it again and holds the record to those digits.  Both modes eliminate the same matrix,
# once plain and once transposed, so the gap is rounding: a few ulps times the elimination's growth.  Beside it
# jvp_cases.ADJOINT_GAP_CPU, the reference derivatives': 0.054 (QCQP), 0.060 (signed box), 2.6e-4 (box).  The device tests allow
# 10 x the record, the JVP tests' margin.
ADJOINT_GAP_CPU = {"qp": 1.1e-16, "qcqp": 1.8e-16, "box": 8.1e-17, "sbox": 1.1e-16}

# The largest relative difference max |newton - oracle| / max |oracle| over a problem's gradients between the restatement's
# backward and the oracle's (epsilon = 1e-10) at the same polished x, on the strictly complementary problems of AGREE_BATCHES, per
# kind, as measured, to two digits; the CPU test allows 10 x it (the regularisation error scales with the batch's conditioning).
AGREE_CPU = {"qp": 4.1e-7, "qcqp": 3.8e-5, "box": 6.5e-6, "sbox": 5.1e-5}
AGREE_N, AGREE_B = 8, 32
STRICT = 1e-6   # of the check's scale: how far every z_i must be from its bounds / disc boundary
MARGIN_OF_SCALE = 0.02   # ... and how far it is on the built agreement batches (AGREE_MARGIN of a width, below), asserted


def _p(a):
    return None if a is None else a.ctypes.data_as(_D)


@functools.lru_cache(maxsize=None)
def hostcore():
    """The host core as a shared library, built on demand (plain: the yardstick of the device tests too)."""
    src = os.path.join(HERE, "hostcore", "newton_core_check.cpp")
    so = os.path.join(HERE, "hostcore", "libnewtoncheck.so")
    deps = [src] + [os.path.join(HERE, "..", "diffqcqp_amd", "csrc", f)
                    for f in ("newton_core.h", "polish_core.h", "check_core.h", "sbox_bounds.h", "common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(p) > os.path.getmtime(so) for p in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fvisibility=hidden",
                               "-Wno-unknown-pragmas", "-o", so + ".tmp", src])
        os.replace(so + ".tmp", so)
    return ctypes.CDLL(so)


def hostcore_program():
    """The same file as a stand-alone program with the address and undefined-behaviour sanitizers -- CPU tests only."""
    src = os.path.join(HERE, "hostcore", "newton_core_check.cpp")
    exe = os.path.join(HERE, "hostcore", "newton_core_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                           "-ffp-contract=off", "-Wno-unknown-pragmas", "-DNEWTON_CHECK_MAIN", "-o", exe, src])
    return exe


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def host_jvp(kind, P, q, ex, x, tangents=(), diag=False, status=True):
    """P (B,N,N), or (B,N) with diag (dP alike); q, x (B,N); ex each (B,.); tangents (dP, dq[, da, db]), None = NULL
    -> (dx (B,N), status (B) int32)."""
    B, N = x.shape
    P, q, x = _c(P), _c(q), _c(x)
    assert P.shape == ((B, N) if diag else (B, N, N))
    ex = [_c(e) for e in ex] + [None] * (3 - len(ex))
    t = [_c(v) for v in tuple(tangents) + (None,) * (4 - len(tangents))]
    dx, st = np.full((B, N), 7.0), np.full(B, -1, dtype=np.int32)
    rc = hostcore().newton_jvp_batch(R.KIND[kind], B, N, int(diag), _p(P), _p(q), _p(ex[0]), _p(ex[1]), _p(ex[2]), _p(x), _p(t[0]),
                                     _p(t[1]), _p(t[2]), _p(t[3]), _p(dx), st.ctypes.data_as(_I) if status else None)
    assert rc == 0
    return dx, st


def host_backward(kind, P, q, ex, x, gx, need=(True, True, True, True), diag=False, status=True):
    """-> (grad_P (as P), grad_q (B,N), grad_a, grad_b (B,.); None where not needed or the QP has none, status (B) int32)."""
    B, N = x.shape
    P, q, x, gx = _c(P), _c(q), _c(x), _c(gx)
    ne = 0 if kind == "qp" else (N // 2 if kind == "qcqp" else N)
    ex = [_c(e) for e in ex] + [None] * (3 - len(ex))
    gP = np.full(P.shape, 7.0) if need[0] else None
    gq = np.full((B, N), 7.0) if need[1] else None
    ga = np.full((B, ne), 7.0) if ne and need[2] else None
    gb = np.full((B, ne), 7.0) if ne and need[3] else None
    st = np.full(B, -1, dtype=np.int32)
    rc = hostcore().newton_bwd_batch(R.KIND[kind], B, N, int(diag), _p(P), _p(q), _p(ex[0]), _p(ex[1]), _p(ex[2]), _p(x), _p(gx),
                                     _p(gP), _p(gq), _p(ga), _p(gb), st.ctypes.data_as(_I) if status else None)
    assert rc == 0
    return gP, gq, ga, gb, st


@functools.lru_cache(maxsize=None)
def problem(kind, N, structure, B=B_CPU):
    """-> (P (B,N,N), q (B,N), ex, x (B,N)): polish_cases' batch as tests/golden/polish froze it (the same arrays on every
    host: the builders' last bits are not), its x polished by polish_reference (read-only)."""
    assert B == B_CPU
    d, x0 = PC.frozen(kind, N, structure)
    P, q, ex = PC.flat(d, kind)
    x = R.polish_batch(kind, P, q, ex, np.ascontiguousarray(x0[:, :, 0]), PC.MAX_STEPS)[0]
    x.setflags(write=False)
    return P, q, ex, x


def inputs(kind, N, B, structure, seed=0):
    """-> (tangents (dP (B,N,N) -- diagonal with structure "diag" --, dq[, da, db]), g (B,N)): seeded."""
    s = 31000 + 1000 * R.KIND[kind] + 10 * N + (structure == "diag") + 7 * seed
    return JR.random_tangents(kind, B, N, s, diag=structure == "diag"), np.random.default_rng(s + 1).standard_normal((B, N))


def restatement_gap(kind, N, structure):
    P, q, ex, x = problem(kind, N, structure)
    tan, g = inputs(kind, N, x.shape[0], structure)
    dx, sj = NR.jvp_batch(kind, P, q, ex, x, *tan)
    gP, gq, ga, gb, sb = NR.backward_batch(kind, P, q, ex, x, g)
    assert not sj.any() and not sb.any()
    return JC.adjoint_gap(g, dx, [gP, gq] + ([ga, gb] if kind != "qp" else []), tan)


def strictly_complementary(kind, P, q, ex, x, strict=STRICT):
    """Per problem: every z_i at least `strict` of the check's scale away from its bounds (contacts: from the disc's boundary).
    -> (mask (B) bool, active fraction, free fraction over the batch's coordinates / contacts)"""
    B, n = x.shape
    scale = R.scale(P, q, x)
    ok, active, total = np.ones(B, dtype=bool), 0, 0
    for b in range(B):
        exb = tuple(e[b] for e in ex)
        z = R.evaluate(kind, P[b], q[b], exb, x[b])[0]
        if kind == "qcqp":
            rad = exb[0] * exb[1]
            nrm = np.hypot(z[0::2], z[1::2])
            dist, act = np.abs(nrm - rad), nrm > rad
        else:
            lo, hi = R.effective_bounds(kind, exb, n)
            dist, act = np.minimum(np.abs(z - lo), np.abs(z - hi)), ~((lo < z) & (z < hi))
        ok[b] = dist.min() >= strict * scale[b]
        active += int(act.sum())
        total += act.size
    return ok, active / total, 1.0 - active / total


# The batches of the agreement test, all four kinds on a diagonal and on a dense P.  The reference's derivative is a Tikhonov
# iterate (weight 1e-7) of a system whose complementarity rows are scaled by the multipliers: where a multiplier is small against
# the square root of that weight the reference is off by its own regularisation, whatever the strictness rule says (a box
# coordinate 8e-5 outside its bound is strictly complementary at 1e-6 and the reference's grad_l_min there is -0.07 where finite
# differences give -1.61).  So the batches are BUILT with a multiplier margin: z is chosen per coordinate (contact) -- half of them
# free, at least AGREE_MARGIN of the interval's width (the radius) inside; half active, at least AGREE_MARGIN outside, on either
# side; the signed box on its effective bounds, so both the caller's bounds and the sign constraint's 0 are sat on -- and
# q = x - z - P x with x = PI(z) makes x the solution.  The test asserts the margin, the quarter active / quarter free and the
# at-most-a-tenth-left-out conditions on the oracle's own polished solutions.
AGREE_MARGIN = 0.2
AGREE_BATCHES = [(k, s) for k in KINDS for s in ("diag", "dense")]


@functools.lru_cache(maxsize=None)
def agree_problem(kind, structure):
    """-> (d with grad_x, P, q, ex, x (B,N)): x the oracle's forward at eps = 1e-3 polished by the restatement."""
    from conftest import make_problem
    from warm_cases import well_conditioned
    B, n = AGREE_B, AGREE_N
    seed = 83000 + 1000 * R.KIND[kind] + (structure == "diag")
    t = make_problem(kind, B, n, seed, structure)
    P = np.ascontiguousarray(well_conditioned(t["P"]).numpy())
    r = np.random.default_rng(seed)
    m = AGREE_MARGIN
    d = {"P": P, "grad_x": np.ascontiguousarray(t["grad_x"].numpy())}
    if kind == "qcqp":
        nc = n // 2
        d["l_n"], d["mu"] = r.uniform(0.5, 1.5, (B, nc, 1)), r.uniform(0.3, 1.0, (B, nc, 1))
        rad = (d["l_n"] * d["mu"])[:, :, 0]
        active = r.permuted(np.tile(np.arange(nc) % 2 == 0, (B, 1)), axis=1)
        nrm = rad * np.where(active, r.uniform(1 + m, 3.0, (B, nc)), r.uniform(0.1, 1 - m, (B, nc)))
        phi = r.uniform(0.0, 2 * np.pi, (B, nc))
        z = np.stack([nrm * np.cos(phi), nrm * np.sin(phi)], axis=2).reshape(B, n)
        ex = (d["l_n"][:, :, 0], d["mu"][:, :, 0])
    else:
        if kind == "qp":
            lo, w = np.zeros((B, n)), np.ones((B, n))
            hi = np.full((B, n), R.INF)
            ex = ()
        else:
            d["l_min"], d["l_max"] = -r.uniform(0.3, 1.0, (B, n, 1)), r.uniform(0.3, 1.0, (B, n, 1))
            ex = (d["l_min"][:, :, 0], d["l_max"][:, :, 0])
            if kind == "sbox":
                d["v"] = r.choice([-1.0, 1.0], (B, n, 1)) * r.uniform(0.2, 1.0, (B, n, 1))
                ex += (d["v"][:, :, 0],)
            lo, hi = (np.stack(a) for a in zip(*(R.effective_bounds(kind, tuple(e[b] for e in ex), n) for b in range(B))))
            w = hi - lo
        active = r.permuted(np.tile(np.arange(n) % 2 == 0, (B, 1)), axis=1)
        below = r.random((B, n)) < 0.5 if kind != "qp" else np.ones((B, n), dtype=bool)
        out = r.uniform(m, 1.0, (B, n)) * w
        inside = lo + r.uniform(m, 1 - m, (B, n)) * w if kind != "qp" else r.uniform(m, 1.0, (B, n))
        z = np.where(active, np.where(below, lo - out, np.where(np.isfinite(hi), hi, 0.0) + out), inside)
    x = np.stack([R.project(kind, z[b], tuple(e[b] for e in ex), n) for b in range(B)])
    d["q"] = np.ascontiguousarray((x - z - np.einsum("bij,bj->bi", P, x))[:, :, None])
    x0 = PC.oracle_forward(kind, d, PC.EPS_START, PC.MAX_ITER)
    P, q, ex = PC.flat(d, kind)
    xp = R.polish_batch(kind, P, q, ex, np.ascontiguousarray(x0[:, :, 0]), PC.MAX_STEPS)[0]
    return d, P, q, ex, xp


def agreement(kind, ref, got, rows):
    """Largest over `rows` of max |newton - oracle| / max |oracle|, both maxima over all of a problem's gradients.  ref: the
    oracle's outputs by name (test_bwd_systems_hostcore._oracle_backward), got: newton_reference.backward_batch's."""
    names = ["grad_P", "grad_q"] + (["g0", "g1"] if kind != "qp" else [])
    worst = 0.0
    for b in rows:
        diff = max(float(np.abs(got[i][b] - ref[nm][b]).max()) for i, nm in enumerate(names))
        den = max(float(np.abs(ref[nm][b]).max()) for nm in names)
        worst = max(worst, diff / den if den > 0 else diff)   # (a QP with every coordinate on its bound: all zeros)
    return worst


def same_bits(a, b):
    return PC.same_bits(a, b)
