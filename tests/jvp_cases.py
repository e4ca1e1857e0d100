"""Inputs and host-side yardsticks of the forward-mode (JVP) tests -- tests/test_jvp_*.py on the CPU, tests/test_gpu_jvp.py on
the device.  Not a test file.  Problems: make_problem's families with every P re-conditioned by warm_cases.well_conditioned
(condition number <= 4), solved by the oracle at eps = 1e-10; the derivative threshold is epsilon = 1e-10.  The yardstick of
the kernels is the host core (tests/hostcore/jvp_check.cpp: the product's own bwd_systems.h helpers on one CPU thread), itself
held bit-equal to the numpy restatement tests/jvp_reference.py."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np

import jvp_reference as R
from conftest import make_problem
from warm_cases import well_conditioned

HERE = os.path.dirname(os.path.abspath(__file__))
D = ctypes.POINTER(ctypes.c_double)
I = ctypes.POINTER(ctypes.c_int)
EPS_FWD, MAX_ITER, EPSILON = 1e-10, 100000, 1e-10
EXTRAS = {"qp": (), "qcqp": ("l_n", "mu"), "box": ("l_min", "l_max"), "sbox": ("l_min", "l_max", "v")}


def _p(a):
    return None if a is None else a.ctypes.data_as(D)


@functools.lru_cache(maxsize=None)
def hostcore():
    src = os.path.join(HERE, "hostcore", "jvp_check.cpp")
    so = os.path.join(HERE, "hostcore", "libjvpcheck.so")
    deps = [src, os.path.join(HERE, "hostcore", "bwd_systems_check.cpp")]
    deps += [os.path.join(HERE, "..", "diffqcqp_amd", "csrc", f) for f in ("bwd_systems.h", "kkt_core.h", "sbox_bounds.h", "common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fvisibility=hidden",
                               "-o", so + ".tmp", src])
        os.replace(so + ".tmp", so)
    return ctypes.CDLL(so)


def seed_of(kind, N, structure):
    return 52000 + 1000 * R.KIND[kind] + 10 * N + (structure == "diag")


@functools.lru_cache(maxsize=None)
def problem(kind, N, B, structure="dense"):
    """-> (d: make_problem's dict as read-only numpy arrays, P well conditioned; x: the oracle's solution (B,N,1))."""
    from oracle import oracle as O
    O.build()
    t = make_problem(kind, B, N, seed_of(kind, N, structure), structure)
    t["P"] = well_conditioned(t["P"])
    d = {k: np.ascontiguousarray(v.numpy()) for k, v in t.items()}
    if kind == "qp":
        x, _ = O.qp_fwd_batch(d["P"], d["q"], EPS_FWD, MAX_ITER)
    elif kind == "qcqp":
        x, _ = O.qcqp_fwd_batch(d["P"], d["q"], d["l_n"], d["mu"], EPS_FWD, MAX_ITER)
    else:
        x, _ = O.boxqp_fwd_batch(d["P"], d["q"], d["l_min"], d["l_max"], EPS_FWD, MAX_ITER, v=d.get("v"))
    for a in list(d.values()) + [x]:
        a.setflags(write=False)
    return d, x


def host_jvp(kind, d, x, tangents, epsilon=EPSILON):
    """The host core over a batch.  tangents: (dP (B,N,N), dq (B,N)[, da, db]), None entries = NULL -> (dx (B,N), steps)."""
    lib = hostcore()
    P, q, ex = R.flat(d, kind)
    B, N = q.shape
    xx = np.ascontiguousarray(x.reshape(B, N))
    tangents = tuple(tangents) + (None,) * (4 - len(tangents))
    tangents = [None if t is None else np.ascontiguousarray(t, dtype=np.float64) for t in tangents]
    ex = [np.ascontiguousarray(e) for e in ex] + [None] * (3 - len(ex))
    dx = np.zeros((B, N))
    steps = np.zeros((B, 2 if kind in ("box", "sbox") else 1), dtype=np.int32)
    row = lambda a, b: None if a is None else _p(a[b])   # noqa: E731
    for b in range(B):
        lib.jvp_check(R.KIND[kind], N, _p(np.ascontiguousarray(P[b])), _p(q[b]), row(ex[0], b), row(ex[1], b), row(ex[2], b),
                      _p(xx[b]), row(tangents[0], b), row(tangents[1], b), row(tangents[2], b), row(tangents[3], b),
                      ctypes.c_double(epsilon), _p(dx[b]), steps[b].ctypes.data_as(I))
    return dx, steps


# ---- the adjoint identity <g, dx> = sum <grad, tangent> ----------------------------------------------------------------------
# Backward and JVP return Tikhonov iterates of A^T b = rhs and A w = s (mu_ir = 1e-7, 1 or 3 bodies): regularised by A A^T and
# by A^T A, truncated alike, so the identity holds to the refinement's accuracy only.  ADJOINT_GAP_CPU: the largest relative gap
# of the numpy restatement's two modes on ADJOINT_BATCHES, as measured, to two digits (tests/test_jvp_reference.py measures it
# again and holds the record to exactly those digits); the GPU tests allow 10 x the record.  The gap is normalised by the sum
# of the absolute terms, so it cannot exceed 1: at 10 x the QCQP's and the signed box QP's bars catch a wrong sign or a
# misplaced row, not a small error -- what pins the values is the bit-equality with the host core.  QP: the system is symmetric, the gap is rounding.  QCQP: the
# cone rows put singular values of 1e-3 .. 1e-2 into A, where one body of the refinement is off by percents -- in each mode.
ADJOINT_BATCHES = ((8, 37, "dense"), (8, 67, "diag"), (3, 37, "dense"), (4, 37, "dense"))
ADJOINT_GAP_CPU = {"qp": 3.9e-16, "qcqp": 0.054, "box": 2.6e-4, "sbox": 0.060}


def adjoint_inputs(kind, N, B, structure):
    """-> (tangents as jvp_reference.random_tangents, g (B,N)) of a batch: seeded, shared by the CPU and GPU tests."""
    seed = 99 + seed_of(kind, N, structure)
    return R.random_tangents(kind, B, N, seed, diag=structure == "diag"), np.random.default_rng(seed + 1).standard_normal((B, N))


def adjoint_gap(g, dx, grads, tangents):
    """Largest over the batch of |<g, dx> - sum <grad, tangent>| / sum |terms|; every array (B, ...); exactly rounded sums."""
    worst = 0.0
    for b in range(g.shape[0]):
        lhs = (g[b] * dx[b]).ravel()
        rhs = np.concatenate([(a[b] * t[b]).ravel() for a, t in zip(grads, tangents)])
        scale = math.fsum(np.abs(lhs)) + math.fsum(np.abs(rhs))
        if scale > 0:   # (a QP with every coordinate at its bound: both sides are exact zeros)
            worst = max(worst, abs(math.fsum(lhs) - math.fsum(rhs)) / scale)
    return worst


def restatement_gap(kind, d, x, tan, g, rows=None):
    """adjoint_gap of the numpy restatement's two modes on a batch (rows: the problems to take, default all)."""
    P, q, ex = R.flat(d, kind)
    rows = range(q.shape[0]) if rows is None else list(rows)
    dx, grads = [], []
    for b in rows:
        exb = tuple(e[b] for e in ex)
        bw = R.derivative(kind, P[b], q[b], exb, x[b, :, 0], EPSILON, "bwd", g=g[b])
        dx.append(R.derivative(kind, P[b], q[b], exb, x[b, :, 0], EPSILON, "jvp", tangents=tuple(t[b] for t in tan))["dx"])
        grads.append([bw["grad_P"], bw["grad_q"]] + ([bw["g0"], bw["g1"]] if kind != "qp" else []))
    return adjoint_gap(g[rows], np.stack(dx), [np.stack(c) for c in zip(*grads)], [t[rows] for t in tan])


def adjoint_gap_cpu(kind, N, B, structure):
    if kind == "qcqp" and N % 2:
        N += 1
    d, x = problem(kind, N, B, structure)
    tan, g = adjoint_inputs(kind, N, B, structure)
    return restatement_gap(kind, d, x, tan, g)


# ---- non-default epsilon -------------------------------------------------------------------------------------------------------
# epsilon sets the active sets of the differentiated system.  On problem()'s x (the oracle at eps = 1e-10) no coordinate lies
# between 1e-10 and 1e-3 of its bound, and every epsilon selects the same sets.  loose_problem() takes the same inputs with the
# oracle's forward stopped at eps = 1e-4 -- and, because the oracle returns the PROJECTED iterate, whose active coordinates lie
# on their bounds to the last bit at any tolerance (measured: 0 to 4 % of a batch moved by the forward's tolerance alone),
# pulls that x into the feasible set's interior by a seeded u in [0.5, 2] x 1e-4 per coordinate / contact (pull_inside): what
# an interior-point or an unprojected iterate of that accuracy looks like.  Near-active coordinates then sit around 1e-4 off
# their bounds and EPSILONS select different sets -- tests/test_jvp_reference.py holds that to account on the numpy restatement
# (at least MIN_MOVED of every batch changes dx between the first and the last epsilon); the GPU test compares with the host core.
EPSILONS = (1e-10, 1e-6, 1e-3)
EPS_LOOSE = 1e-4
MIN_MOVED = 0.10


def pull_inside(kind, d, x, seed):
    """x (B,N,1) moved off the boundary of the feasible set by u ~ U(0.5e-4, 2e-4): x + u (QP: x >= 0); into [lo + u, hi - u]
    (box kinds, the signed box QP's effective bounds; a coordinate whose interval is shorter than 2 u stays); a contact within
    u of its disc's rim scaled to radius r - u (QCQP, r = l_n mu > u)."""
    B, N = x.shape[:2]
    xs = np.array(x.reshape(B, N))
    _, _, ex = R.flat(d, kind)
    if kind == "qp":
        return (xs + np.random.default_rng(seed).uniform(0.5e-4, 2e-4, (B, N)))[:, :, None]
    if kind == "qcqp":
        u = np.random.default_rng(seed).uniform(0.5e-4, 2e-4, (B, N // 2))
        r = ex[0] * ex[1]
        nrm = np.sqrt(xs[:, 0::2] ** 2 + xs[:, 1::2] ** 2)
        near = (nrm > r - u) & (r > u)
        f = np.where(near, (r - u) / np.where(near, nrm, 1.0), 1.0)
        xs[:, 0::2] *= f
        xs[:, 1::2] *= f
        return xs[:, :, None]
    u = np.random.default_rng(seed).uniform(0.5e-4, 2e-4, (B, N))
    lo, hi = ex[0], ex[1]
    if kind == "sbox":
        eb = [R.effective_bounds(lo[b], hi[b], ex[2][b]) for b in range(B)]
        lo, hi = np.stack([e[0] for e in eb]), np.stack([e[1] for e in eb])
    room = hi - lo > 2 * u
    return np.where(room, np.minimum(np.maximum(xs, lo + u), hi - u), xs)[:, :, None]
# one row per family: (kind, N, B, structure) -- JvpDiag, JvpTeam, JvpAny (the box kinds' first N beyond the team kernel)
EPSILON_ROWS = [(k, 8, 67, "diag") for k in EXTRAS] + [(k, 8, 37, "dense") for k in EXTRAS] + \
               [("box", 22, 5, "dense"), ("sbox", 22, 5, "dense")]


@functools.lru_cache(maxsize=None)
def loose_problem(kind, N, B, structure="dense"):
    """problem()'s inputs, x from the oracle's forward at EPS_LOOSE, pulled inside."""
    from oracle import oracle as O
    d, _ = problem(kind, N, B, structure)
    if kind == "qp":
        x, _ = O.qp_fwd_batch(d["P"], d["q"], EPS_LOOSE, MAX_ITER)
    elif kind == "qcqp":
        x, _ = O.qcqp_fwd_batch(d["P"], d["q"], d["l_n"], d["mu"], EPS_LOOSE, MAX_ITER)
    else:
        x, _ = O.boxqp_fwd_batch(d["P"], d["q"], d["l_min"], d["l_max"], EPS_LOOSE, MAX_ITER, v=d.get("v"))
    x = np.ascontiguousarray(pull_inside(kind, d, x, 7 + seed_of(kind, N, structure)))
    x.setflags(write=False)
    return d, x


def epsilon_tangents(kind, N, B, structure):
    return R.random_tangents(kind, B, N, 61 + seed_of(kind, N, structure), diag=structure == "diag")


def moved_by_epsilon(kind, N, B, structure):
    """The share of loose_problem's batch whose dx, in the numpy restatement, differs between EPSILONS[0] and EPSILONS[-1]."""
    d, x = loose_problem(kind, N, B, structure)
    P, q, ex = R.flat(d, kind)
    tan = epsilon_tangents(kind, N, B, structure)
    a = R.jvp_batch(kind, P, q, ex, x[:, :, 0], tan, EPSILONS[0])[0]
    b = R.jvp_batch(kind, P, q, ex, x[:, :, 0], tan, EPSILONS[-1])[0]
    return float((a != b).any(axis=1).mean())


# ---- the reference's ill-conditioned inputs ------------------------------------------------------------------------------------
# tests/golden: the reference's hard-coded matrices (ref_*: singular, cond ~1e22, a zero-radius contact, rank 3 of 8), seeded
# rank-deficient batches (rd_*: P = S S^T of rank N / 2, duplicated Jacobian rows) and the figure workload
# (conditioning/qp_ill_n8: a diagonal P from 4e-18 to 2.4e17, a third of its x NaN).  Each with the fixture's own x.
GOLDEN = os.path.join(HERE, "golden")


def fixture_names():
    import glob
    pats = ("rd_*.npz", "ref_m2_*.npz", "ref_g2_*.npz", "ref_g4_*.npz", "ref_gblock_*.npz")
    names = sorted(os.path.basename(p)[:-4] for pat in pats for p in glob.glob(os.path.join(GOLDEN, pat)))
    return names + ["conditioning/qp_ill_n8"]


def fixture_family(name):
    """'rd_duprows_qcqp_n32' -> 'rd_duprows_qcqp': the key of FIXTURE_GAP_CPU."""
    base = os.path.basename(name)
    parts = base.split("_")
    return "_".join(parts[:3]) if parts[0] == "rd" else ("qp_ill" if parts[1] == "ill" else "_".join(parts[:3]))


@functools.lru_cache(maxsize=None)
def fixture(name):
    """-> (kind, d, x (B,N,1), tangents, g (B,N), P is diagonal), read-only; tangents and g seeded by the name."""
    import zlib
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        kind = "qcqp" if "l_n" in z.files else "qp"
        d = {k: np.ascontiguousarray(z[k], dtype=np.float64) for k in ("P", "q") + EXTRAS[kind]}
        x = np.ascontiguousarray(z["x"], dtype=np.float64)
    B, N = d["q"].shape[:2]
    diagonal = bool((d["P"] == d["P"] * np.eye(N)).all())
    seed = zlib.crc32(name.encode()) % 100000
    tan = R.random_tangents(kind, B, N, seed)
    g = np.random.default_rng(seed + 1).standard_normal((B, N))
    for a in list(d.values()) + [x, g] + list(tan):
        a.setflags(write=False)
    return kind, d, x, tan, g, diagonal


def finite_rows(x):
    return np.flatnonzero(np.isfinite(x.reshape(x.shape[0], -1)).all(axis=1))


def fixture_gap_cpu(name):
    """restatement_gap on a fixture's problems with a finite x."""
    kind, d, x, tan, g, _ = fixture(name)
    return restatement_gap(kind, d, x, tan, g, finite_rows(x))


# The largest adjoint gap of the numpy restatement's two modes per fixture family (the largest over the family's files, on the
# problems whose x is finite), as measured, to two digits: tests/test_jvp_reference.py measures it again and holds the record
# to those digits; tests/test_gpu_jvp_conditioning.py allows 10 x the record.  On these singular systems the two Tikhonov
# iterates (regularised by A A^T and by A^T A, 1 to 10 bodies) need not agree at all: where the restatement's own gap exceeds
# ADJOINT_GAP_TELLS the normalised gap (which cannot exceed 1) tells nothing, and the GPU test makes no adjoint check for that
# family -- rd_lowrank_qp 0.31, ref_m2_qp 0.16, qp_ill 0.49.  The bit-equality with the host core holds for every fixture.
FIXTURE_GAP_CPU = {"rd_duprows_qcqp": 0.013, "rd_duprows_qp": 3.7e-05, "rd_lowrank_qcqp": 0.0086, "rd_lowrank_qp": 0.31,
                   "ref_g2_qcqp": 0.0019, "ref_g2_qp": 4.8e-12, "ref_g4_qcqp": 0.042, "ref_g4_qp": 4.2e-08, "ref_gblock_qcqp": 0.039,
                   "ref_gblock_qp": 1.1e-16, "ref_m2_qcqp": 2.3e-09, "ref_m2_qp": 0.16, "qp_ill": 0.49}
ADJOINT_GAP_TELLS = 0.1
