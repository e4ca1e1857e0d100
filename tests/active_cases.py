"""Inputs and host-side yardsticks of the active-set tests (dqq_newton_active_f64) -- tests/test_active_*.py on the CPU,
tests/test_gpu_active*.py on the device.  Not a test file.  Problems: newton_cases' (polish_cases' frozen batches at a polished
x, and the built agreement batches), inf_bounds_cases' one-sided batches, and built problems that reach what those do not.  The
yardstick of the kernels is the host program tests/hostcore/active_core_check.cpp (csrc/active_core.h on one CPU thread, the
flag an argument), itself held bit-equal to the numpy restatement tests/active_reference.py."""
import functools
import os
import subprocess
import tempfile

import numpy as np

import active_reference as AR
import jac_reference as JR
import newton_cases as NC
import polish_cases as PC
import polish_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = NC.KINDS
BATCHES = NC.BATCHES

# (kind, N) of tests/test_gpu_active.py, at diag_b(N) / 37 problems; the sizes and ragged_b are polish_cases'
DIAG_ROWS = [(k, N) for k in KINDS for N in PC.DIAG_N_FIRST + PC.DIAG_N_MORE]
TEAM_ROWS = [(k, N + 1 if k == "qcqp" and N % 2 else N) for k in KINDS for N in (3, 8, 20, 64, PC.TEAM_N16)]   # (a QCQP has an even N)
ANY_ROWS = [(k, 66 if k == "qcqp" else 65) for k in KINDS]
ENTRIES = ("active",)
TEAM_B = 37   # ragged against every tile: 128/N problems per wave (DQQ_P_DIAG), 64/T teams per wave, four waves per workgroup


def diag_b(N):
    return TEAM_B if N in PC.DIAG_N_FIRST else PC.ragged_b(N)


BOX_LIKE = ("qp", "box", "sbox")
STATES = {"qp": (0, 3), "qcqp": (0, 1), "box": (0, 1, 2), "sbox": (0, 1, 2, 3)}   # what every batch must contain
NAMES = ("state", "mult", "margin", "where", "status")

# The property the margin is for, on the numpy restatement (predicted_residual below): the largest natural residual of x + dx at
# q + dq, relative to the check's scale, over BATCHES (newton_cases.B_CPU problems each) per box-like kind, with dq scaled so that
# max |dz| is half the margin -- as measured, to two digits.  x itself carries the polish's residual (polish_cases.RESIDUAL_CPU,
# 2.8e-16) and dx one elimination's rounding (jac_cases.SOLVE_GAP_CPU, below 1e-15), so rounding level it is.  The tests allow
# BAR x the record, the project's convention between hosts (jac_cases.BAR).
PREDICT_CPU = {"qp": 4.7e-16, "box": 2.3e-16, "sbox": 2.1e-16}
BAR = 16


def elements(kind, N):
    return AR.elements(kind, N)


@functools.lru_cache(maxsize=None)
def hostcore(sanitized=False):
    """The host program's path, built on demand.  sanitized: with -fsanitize=address,undefined -- for CPU tests only."""
    src = os.path.join(HERE, "hostcore", "active_core_check.cpp")
    exe = os.path.join(HERE, "hostcore", "active_core_check_san" if sanitized else "active_core_check")
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else ["-O2"]
    deps = [src] + [os.path.join(HERE, "..", "diffqcqp_amd", "csrc", f)
                    for f in ("active_core.h", "newton_core.h", "polish_core.h", "check_core.h", "sbox_bounds.h", "common.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(p) > os.path.getmtime(exe) for p in deps):
        subprocess.check_call(["g++"] + extra + ["-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", exe + ".tmp", src])
        os.replace(exe + ".tmp", exe)
    return exe


def host_active(kind, P, q, ex, x, diag=False, flag=False, mask=15, sanitized=False):
    """The host core over a batch.  kind: any of polish_reference.KIND.  P (B,N,N), or (B,N) with diag; q, x (B,N); ex each (B,.).
    mask: bit i asks for output i of (state, mult, margin, where); one not asked for comes back as its fill (-7 / 7.0).
    -> (state (B,ne) int32, mult (B,ne), margin (B), where (B) int32, status (B) int32)"""
    B, N = x.shape
    k = R.KIND[kind]
    ne = elements(kind, N)
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in [P, q] + list(ex) + [x]]
    assert arrays[0].shape == ((B, N) if diag else (B, N, N)) and len(ex) == (0, 2, 2, 3)[k]
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        with open(fin, "wb") as f:
            f.write(np.array([k, B, N, int(diag), int(flag), int(k == 3), mask, 0], dtype=np.int32).tobytes())
            for a in arrays:
                f.write(a.tobytes())
        subprocess.check_call([hostcore(sanitized), fin, fout])
        raw = open(fout, "rb").read()
    ints = np.frombuffer(raw, dtype=np.int32, count=B * ne + 2 * B)
    dbl = np.frombuffer(raw, dtype=np.float64, offset=4 * (B * ne + 2 * B))
    assert dbl.size == B * ne + B
    return (ints[:B * ne].reshape(B, ne).copy(), dbl[:B * ne].reshape(B, ne).copy(), dbl[B * ne:].copy(),
            ints[B * ne:B * ne + B].copy(), ints[B * ne + B:].copy())


def same_outputs(got, want):
    """All five outputs equal as bit patterns (but for the payload of a NaN) -> the name of the first that differs, or None."""
    for name, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        if g.dtype.kind == "i":
            if g.shape != w.shape or not np.array_equal(g, w):
                return name
        elif not PC.same_bits(g, w):
            return name
    return None


def random_problem(kind, B, N, structure, seed=0):
    """A seeded batch of any size with every quantity of order 1, for the bit comparisons of the device tests (no solver runs):
    P with its spectrum within [0.5, 2.5] (diag: a diagonal on [0.5, 2]); box bounds l_min in [-0.6, -0.1], l_max in [0.1, 0.6],
    v of either sign and one in eight a zero; radii l_n mu with l_n in [0.2, 0.8], mu in [0.3, 1.0] and one l_n in sixteen a
    zero; x = PI(t) for a uniform t on [-1, 1] -- feasible, not a solution: z falls on either side of every bound.
    -> (P (B,N,N), q (B,N), ex, x (B,N))"""
    r = np.random.default_rng(61000 + 1000 * R.KIND[kind] + 10 * N + (structure == "diag") + 7 * seed)
    if structure == "diag":
        P = np.stack([np.diag(v) for v in r.uniform(0.5, 2.0, (B, N))])
    else:
        A = r.uniform(-1.0, 1.0, (B, N, N))
        G = A @ A.transpose(0, 2, 1)
        P = 0.5 * np.eye(N) + 2.0 * G / np.linalg.norm(G, 2, axis=(1, 2))[:, None, None]
        P = 0.5 * (P + P.transpose(0, 2, 1))
    q = r.uniform(-1.0, 1.0, (B, N))
    if kind == "qp":
        ex = ()
    elif kind == "qcqp":
        ln = np.where(r.random((B, N // 2)) < 1.0 / 16, 0.0, r.uniform(0.2, 0.8, (B, N // 2)))
        ex = (ln, r.uniform(0.3, 1.0, (B, N // 2)))
    else:
        ex = (-r.uniform(0.1, 0.6, (B, N)), r.uniform(0.1, 0.6, (B, N)))
        if kind == "sbox":
            v = r.choice([-1.0, 1.0], (B, N)) * r.uniform(0.2, 1.0, (B, N))
            ex += (np.where(r.random((B, N)) < 0.125, 0.0, v),)
    t = r.uniform(-1.0, 1.0, (B, N))
    x = np.stack([R.project(kind, t[b], tuple(e[b] for e in ex), N) for b in range(B)])
    return tuple(np.ascontiguousarray(a) for a in (P, q)) + (tuple(np.ascontiguousarray(e) for e in ex), np.ascontiguousarray(x))


def zero_disc_problem(structure="dense", N=8):
    """One built QCQP problem for the state the batches cannot hold: contact 0 has l_n = 0, so rad = 0 and any z off the origin
    is outside a disc of radius <= 0 (state 3, mult = |z|); contact 1 has l_n = 0 too and z = 0 exactly (inside: n2 = 0 is not
    > 0).  The others are ordinary.  -> (P (1,N,N), q (1,N), (l_n, mu), x (1,N)), x = PI(z) and q = x - z - P x."""
    r = np.random.default_rng(4100 + (structure == "diag"))
    nc = N // 2
    d = r.uniform(0.5, 2.0, N)
    P = np.diag(d)
    if structure != "diag":
        A = r.uniform(-1.0, 1.0, (N, N))
        P = P + 0.1 * (A @ A.T)
    ln, mu = r.uniform(0.5, 1.5, nc), r.uniform(0.3, 1.0, nc)
    ln[0] = ln[1] = 0.0
    z = r.uniform(-1.0, 1.0, N)
    z[2:4] = 0.0
    x = R.project("qcqp", z, (ln, mu), N)
    s = np.zeros(N)
    for j in range(N):          # the row sums as evaluate forms them: where x - z is 0, s + q is 0 exactly and z comes out as 0
        s = s + P[:, j] * x[j]
    q = (x - z) - s
    return P[None], q[None], (ln[None], mu[None]), x[None]


def two_chunk_problem(kind, N=258):
    """One problem whose rows need more than one chunk of 256 and whose nearest element lies in the second chunk: P diagonal
    plus a weak coupling, z built an element at a time -- every element's distance to its bounds (disc boundary) at least 0.1
    but the last one's, 0.01.  -> (P (1,N,N), q (1,N), ex, x (1,N), where expected)"""
    r = np.random.default_rng(5200 + R.KIND[kind])
    P = np.diag(r.uniform(0.5, 2.0, N))
    P[np.arange(N - 1), np.arange(1, N)] = 0.01
    P[np.arange(1, N), np.arange(N - 1)] = 0.01
    ne = elements(kind, N)
    if kind == "qcqp":
        ln, mu = r.uniform(0.5, 1.5, ne), r.uniform(0.5, 1.0, ne)
        rad = ln * mu
        off = np.where(np.arange(ne) % 2 == 0, r.uniform(0.1, 0.5, ne), -r.uniform(0.1, 0.2, ne))
        off[ne - 1] = 0.01
        phi = r.uniform(0.0, 2 * np.pi, ne)
        nrm = rad + off
        z = np.stack([nrm * np.cos(phi), nrm * np.sin(phi)], axis=1).reshape(N)
        ex = (ln, mu)
    else:
        lo, hi = -r.uniform(0.5, 1.0, N), r.uniform(0.5, 1.0, N)
        ex = () if kind == "qp" else ((lo, hi) if kind == "box" else (lo, hi, r.choice([-1.0, 1.0], N)))
        elo, ehi = R.effective_bounds(kind, ex, N)
        pick = np.arange(N) % 3
        dist = r.uniform(0.1, 0.2, N)
        dist[N - 1] = 0.01
        z = np.where(pick == 0, elo + dist, np.where(pick == 1, elo - dist, np.where(np.isfinite(ehi), ehi, 0.0) + dist))
    x = R.project(kind, z, ex, N)
    q = x - z - P @ x
    return P[None], q[None], tuple(e[None] for e in ex), x[None], ne - 1


def predicted_residual(kind, P, q, ex, x, seed, active=AR.active_batch, jacobian=None, flag=False):
    """The property test's figures on a batch of a box-like kind.  Per problem: draw dq, take dx = Jq dq and
    dz = dx - P dx - dq, scale dq so that max |dz| is half the margin, and evaluate the state and the natural residual of
    x + dx at q + dq.  active / jacobian: the functions under test (the restatement's by default; a device test passes its own).
    -> (state before (B,ne), state after (B,ne), residual / scale (B), margin (B))"""
    assert kind in BOX_LIKE
    B, n = x.shape
    st0, _, margin, _, status = active(kind, P, q, ex, x)
    assert not status.any() and (margin > 0.0).all() and np.isfinite(margin).all()
    Jq = jacobian(kind, P, q, ex, x) if jacobian is not None else JR.jacobians_batch(kind, P, q, ex, x, (True, False, False))[0]
    dq = np.random.default_rng(seed).standard_normal((B, n))
    dx = np.einsum("bij,bj->bi", Jq, dq)
    dz = dx - np.einsum("bij,bj->bi", P, dx) - dq
    s = 0.5 * margin / np.abs(dz).max(axis=1)
    dq, dx = dq * s[:, None], dx * s[:, None]
    x1, q1 = x + dx, q + dq
    st1 = active(kind, P, q1, ex, x1)[0]
    resid = np.array([R.evaluate(kind, P[b], q1[b], tuple(np.asarray(e[b], dtype=np.float64).reshape(-1) for e in ex), x1[b])[2]
                      for b in range(B)])
    return st0, st1, resid / R.scale(P, q1, x1), margin
