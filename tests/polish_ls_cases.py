"""Inputs and host-side yardsticks of the damped polish's tests -- tests/test_polish_ls_*.py on the CPU, tests/test_gpu_polish_ls.py
on the device.  Not a test file.  Problems: the recipe of tests/golden/make_polish_ls_golden.py at any (kind, N, B), cold starts
x = PI(0), where full Newton steps are mostly rejected and neighbouring problems accept at different step lengths.  The yardstick
of the kernels is the host core (tests/hostcore/polish_ls_core_check.cpp: polish_core.h's polish_problem_ls on one CPU thread, a
stand-alone program), itself held bit-equal to the numpy restatement tests/polish_ls_reference.py.  Two builds of that program: a
plain one, the yardstick of the device tests, and one with the address and undefined-behaviour sanitizers that only the CPU test
tests/test_polish_ls_hostcore.py runs."""
import functools
import os
import subprocess
import tempfile

import numpy as np

import polish_cases as PC
import polish_ls_reference as L
import polish_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ("qp", "qcqp", "box", "sbox")
MAX_STEPS = 12       # of the device tests: enough for most cold starts, a handful of launches' worth of work

# (kind, N) of the device tests of the damped and of the smoothed families (tests/test_gpu_polish_ls.py, test_gpu_smooth.py); the
# sizes and ragged_b are polish_cases'.  diag_bs(N): the batches of a diagonal row, the properties of the entry run on the second.
DIAG_ROWS = [(k, N) for k in KINDS for N in PC.DIAG_N_FIRST + PC.DIAG_N_MORE]
TEAM_ROWS = [(k, N) for k in KINDS for N in ((4 if k == "qcqp" else 3), 8, PC.TEAM_N16, 20, 64)]   # (a QCQP has an even N)
ANY_ROWS = [(k, 66 if k == "qcqp" else 65) for k in KINDS]
ENTRIES = ("polish_ls",)
TEAM_BS = (1, 9, 67)
ANY_B = 3
DIAG_MATRIX_N = (8, 64) + PC.DIAG_N_MORE      # a diagonal P given as (B,N,N) against DQQ_P_DIAG, at diag_bs(N)[1] problems


def team_layout(N):
    """The layout a team row runs at: DQQ_P_DENSE at N = 8, where DQQ_P_AUTO would be the same route, DQQ_P_AUTO elsewhere."""
    return PC.DENSE if N == 8 else PC.AUTO


def diag_bs(N):
    return (1, 37, 2051) if N in PC.DIAG_N_FIRST else (1, PC.ragged_b(N))


def same_bits(a, b):
    """Equal as bit patterns but for the payload of a NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=True)) and bool(
        np.array_equal(np.signbit(a[~np.isnan(a)]), np.signbit(b[~np.isnan(b)])))


@functools.lru_cache(maxsize=None)
def problem(kind, N, B, structure="dense", seed=0):
    """-> (P (B,N,N), q (B,N), ex each (B,.), x (B,N): the cold start), read-only.  dense: condition number 60; diag:
    P = diag(exp(U(-3, 3)))."""
    r = np.random.default_rng(9000 + 1000 * R.KIND[kind] + 10 * N + (structure == "diag") + 7919 * seed)
    if structure == "diag":
        P = np.zeros((B, N, N))
        P[:, np.arange(N), np.arange(N)] = np.exp(r.uniform(-3.0, 3.0, (B, N)))
    else:
        Q, _ = np.linalg.qr(r.standard_normal((B, N, N)))
        M = (Q * np.exp(r.uniform(0.0, np.log(60.0), (B, 1, N)))) @ Q.transpose(0, 2, 1)
        P = np.ascontiguousarray(0.5 * (M + M.transpose(0, 2, 1)))
    q = r.uniform(-1.0, 1.0, (B, N))
    if kind == "qp":
        ex = ()
    elif kind == "qcqp":
        ex = (r.uniform(0.1, 1.0, (B, N // 2)), r.uniform(0.1, 1.0, (B, N // 2)))
    else:
        ex = (-r.uniform(0.01, 1.0, (B, N)), r.uniform(0.01, 1.0, (B, N)))
        if kind == "sbox":
            ex = ex + (r.standard_normal((B, N)),)
    if kind == "qcqp":
        x = np.zeros((B, N))
    else:
        lo, hi = zip(*(R.effective_bounds(kind, tuple(e[b] for e in ex), N) for b in range(B)))
        x = np.where(np.array(lo) > 0.0, np.array(lo), np.where(np.array(hi) < 0.0, np.array(hi), 0.0))
    for a in (P, q, x) + ex:
        a.setflags(write=False)
    return P, q, ex, x


def one_sided(ex, seed=3):
    """The box extras with about a third of the bounds on each side moved to infinity."""
    r = np.random.default_rng(seed)
    lo, hi = np.array(ex[0]), np.array(ex[1])
    lo[r.random(lo.shape) < 0.33] = -np.inf
    hi[r.random(hi.shape) < 0.33] = np.inf
    return (lo, hi) + tuple(ex[2:])


def compact(P):
    """(B,N,N) -> the diagonals (B,N)."""
    return np.ascontiguousarray(np.diagonal(P, axis1=1, axis2=2))


@functools.lru_cache(maxsize=None)
def hostcore(sanitized=False):
    """The host program's path, built on demand.  sanitized: the build with -fsanitize=address,undefined -- for CPU tests only;
    a test marked gpu uses the plain build."""
    src = os.path.join(HERE, "hostcore", "polish_ls_core_check.cpp")
    exe = os.path.join(HERE, "hostcore", "polish_ls_core_check_san" if sanitized else "polish_ls_core_check")
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else ["-O2"]
    deps = [src] + [os.path.join(HERE, "..", "diffqcqp_amd", "csrc", f)
                    for f in ("polish_core.h", "check_core.h", "sbox_bounds.h", "common.h", "route.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(p) > os.path.getmtime(exe) for p in deps):
        subprocess.check_call(["g++"] + extra + ["-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", exe + ".tmp", src])
        os.replace(exe + ".tmp", exe)
    return exe


def host_polish_ls(kind, P, q, ex, x, max_steps=MAX_STEPS, max_halvings=0, reg=0.0, diag=False, in_place=False, inf_ok=False,
                   sanitized=False):
    """The host core over a batch.  P (B,N,N), or (B,N) with diag; q, x (B,N); ex each (B,.) -> x_out, resid, steps, status,
    halvings.  sanitized: run the sanitizer build (hostcore)."""
    B, N = x.shape
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in (P, q) + tuple(ex) + (x,)]
    assert arrays[0].shape == ((B, N) if diag else (B, N, N))
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        with open(fin, "wb") as f:
            f.write(np.array([R.KIND[kind], B, N, int(diag), max_steps, int(in_place), max_halvings, int(inf_ok)], dtype=np.int32).tobytes())
            f.write(np.array([reg], dtype=np.float64).tobytes())
            for a in arrays:
                f.write(a.tobytes())
        subprocess.check_call([hostcore(sanitized), fin, fout])
        raw = open(fout, "rb").read()
    nd = B * N + 2 * B
    dbl = np.frombuffer(raw[: 8 * nd], dtype=np.float64)
    ints = np.frombuffer(raw[8 * nd:], dtype=np.int32)
    assert ints.size == 3 * B
    return (dbl[: B * N].reshape(B, N).copy(), dbl[B * N:].reshape(B, 2).copy(), ints[:B].copy(), ints[B:2 * B].copy(),
            ints[2 * B:].copy())


@functools.lru_cache(maxsize=None)
def frozen_host(name, kind, max_halvings, max_steps=L.MAX_STEPS):
    """The host core's result on a frozen cold-start row of tests/golden/polish_ls."""
    P, q, ex, x = L.frozen(name, kind)
    return host_polish_ls(kind, P, q, ex, x, max_steps, max_halvings)
