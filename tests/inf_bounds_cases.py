"""Inputs and host-side yardsticks of the one-sided-box tests (DQQ_F_INFINITE_BOUNDS) -- tests/test_inf_bounds_*.py on the CPU,
tests/test_gpu_inf_bounds*.py on the device.  Not a test file.  The yardstick of the kernels is the host program
tests/hostcore/inf_bounds_check.cpp (csrc/polish_core.h and csrc/newton_core.h on one CPU thread, the flag an argument), itself
held bit-equal to the numpy restatement tests/inf_bounds_reference.py."""
import functools
import os
import subprocess
import tempfile

import numpy as np

import polish_reference as R
from polish_cases import AUTO, DENSE, DIAG

HERE = os.path.dirname(os.path.abspath(__file__))
INF = float("inf")
KINDS = ("box", "sbox")
F_INFINITE_BOUNDS = 0x800
HUGE = 1e300          # the finite stand-in of the large-finite equivalence
MAX_STEPS = 8
# (layout, structure, N, B) of tests/test_gpu_inf_bounds.py: DQQ_P_DIAG; the LDS teams at an odd N (T = 8, idle lanes), N = 8 and
# N = 20 (T = 32); the any-N form; then DQQ_P_DIAG's other compiled N (diag_tile.h) at 9 (128/N) + 1 problems -- a last wave with
# one valid problem -- and the teams of 16
ROWS = [(DIAG, "diag", 2, 37), (DIAG, "diag", 8, 37), (DENSE, "dense", 3, 37), (AUTO, "dense", 8, 37), (DENSE, "dense", 20, 37),
        (DENSE, "dense", 65, 5), (DIAG, "diag", 4, 289), (DIAG, "diag", 16, 73), (DIAG, "diag", 32, 37), (DENSE, "dense", 12, 37)]
ENTRIES = ("polish", "bwd", "jvp", "jac")     # what gpu_all of the device test runs on every row, under the flag
DIAG_MATRIX = [(8, 37), (4, 289), (16, 73), (32, 37)]     # (N, B): a diagonal P given as (B,N,N) against DQQ_P_DIAG


def problem(kind, B, N, structure, seed=0, bad_row=None):
    """A seeded batch with every quantity of order 1 -> (P (B,N,N), q, ex, x, gx (B,N), tangents (dP (B,N,N), dq, da, db)).
    P: spectrum within [0.5, 2.5] (diag: a diagonal on [0.5, 2]).  Bounds: finite l_min in [-0.6, -0.1], l_max in [0.1, 0.6], then
    per coordinate one of finite/finite, -inf/finite, finite/+inf, -inf/+inf, each a quarter of a problem's coordinates (rounded),
    in an order shuffled per problem.  sbox: v of either sign, one coordinate in eight a zero.  x: uniform on [-0.5, 0.5] -- not a
    solution: the polish has work to do, the derivatives are taken where they are asked for.  dP is diagonal with "diag".
    bad_row: that problem gets l_min = +inf at coordinate 0 (status 2 with or without the flag)."""
    r = np.random.default_rng(97000 + 1000 * R.KIND[kind] + 10 * N + (structure == "diag") + 7 * seed)
    if structure == "diag":
        P = np.stack([np.diag(v) for v in r.uniform(0.5, 2.0, (B, N))])
        dP = np.stack([np.diag(v) for v in r.standard_normal((B, N))])
    else:
        A = r.uniform(-1.0, 1.0, (B, N, N))
        G = A @ A.transpose(0, 2, 1)
        P = 0.5 * np.eye(N) + 2.0 * G / np.linalg.norm(G, 2, axis=(1, 2))[:, None, None]
        P = 0.5 * (P + P.transpose(0, 2, 1))
        dP = r.standard_normal((B, N, N))
    q = r.uniform(-1.0, 1.0, (B, N))
    lo, hi = -r.uniform(0.1, 0.6, (B, N)), r.uniform(0.1, 0.6, (B, N))
    combo = r.permuted((np.arange(N)[None, :] + np.arange(B)[:, None]) % 4, axis=1)   # (N < 4: the four take turns over the batch)
    lo = np.where((combo == 1) | (combo == 3), -INF, lo)
    hi = np.where((combo == 2) | (combo == 3), INF, hi)
    ex = (lo, hi)
    if kind == "sbox":
        v = r.choice([-1.0, 1.0], (B, N)) * r.uniform(0.2, 1.0, (B, N))
        ex += (np.where(r.random((B, N)) < 0.125, 0.0, v),)
    x = r.uniform(-0.5, 0.5, (B, N))
    gx = r.standard_normal((B, N))
    tangents = (dP, r.standard_normal((B, N)), r.standard_normal((B, N)), r.standard_normal((B, N)))
    if bad_row is not None:
        ex[0][bad_row, 0] = INF
    return tuple(np.ascontiguousarray(a) for a in (P, q)) + (tuple(np.ascontiguousarray(e) for e in ex),) + (x, gx, tangents)


def large_finite(ex):
    """ex with every infinite bound replaced by -HUGE / +HUGE (v is left alone)."""
    lo, hi = ex[0], ex[1]
    return (np.where(lo == -INF, -HUGE, lo), np.where(hi == INF, HUGE, hi)) + tuple(ex[2:])


def compact(P):
    return np.ascontiguousarray(np.diagonal(P, axis1=1, axis2=2))


def compact_jac(J):
    """The DQQ_P_DIAG form of a box kind's Jacobian (B,N,N): its diagonal."""
    return compact(J)


@functools.lru_cache(maxsize=None)
def hostcore(sanitized=False):
    """The host program's path, built on demand.  sanitized: with -fsanitize=address,undefined -- for CPU tests only."""
    src = os.path.join(HERE, "hostcore", "inf_bounds_check.cpp")
    exe = os.path.join(HERE, "hostcore", "inf_bounds_check_san" if sanitized else "inf_bounds_check")
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else ["-O2"]
    deps = [src] + [os.path.join(HERE, "..", "diffqcqp_amd", "csrc", f)
                    for f in ("newton_core.h", "polish_core.h", "check_core.h", "sbox_bounds.h", "common.h", "route.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(p) > os.path.getmtime(exe) for p in deps):
        subprocess.check_call(["g++"] + extra + ["-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", exe + ".tmp", src])
        os.replace(exe + ".tmp", exe)
    return exe


def host_all(kind, P, q, ex, x, gx, tangents=None, diag=False, flag=True, max_steps=MAX_STEPS, sanitized=False):
    """The four host cores over a batch.  kind: any of polish_reference.KIND.  P (B,N,N), or (B,N) with diag (dP alike); q, x, gx
    (B,N); ex each (B,.); tangents (dP, dq, da, db) or None (all NULL).  -> dict: x_out, resid (B,2), dx, gP (as P), gq, ga, gb,
    Jq, Ja, Jb (as include/diffqcqp_hip.h shapes them; the QP has no ga, gb, Ja, Jb), steps, st_polish, st_jvp, st_bwd, st_jac."""
    B, N = x.shape
    k = R.KIND[kind]
    ne = 0 if k == 0 else (N // 2 if k == 1 else N)
    arrays = [P, q] + list(ex) + [x, gx] + (list(tangents) if tangents is not None else [])
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in arrays]
    assert arrays[0].shape == ((B, N) if diag else (B, N, N)) and len(ex) == (0, 2, 2, 3)[k]
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        with open(fin, "wb") as f:
            f.write(np.array([k, B, N, int(diag), max_steps, int(flag), int(k == 3), int(tangents is not None)], dtype=np.int32).tobytes())
            for a in arrays:
                f.write(a.tobytes())
        subprocess.check_call([hostcore(sanitized), fin, fout])
        raw = open(fout, "rb").read()
    pshape = (B, N) if diag else (B, N, N)
    jq = ((B, N, 2) if k == 1 else (B, N)) if diag else (B, N, N)
    je = (B, N) if diag else (B, N, ne)
    shapes = [("x_out", (B, N)), ("resid", (B, 2)), ("dx", (B, N)), ("gP", pshape), ("gq", (B, N))]
    shapes += [("ga", (B, ne)), ("gb", (B, ne))] if ne else []
    shapes += [("Jq", jq)] + ([("Ja", je), ("Jb", je)] if ne else [])
    out, off = {}, 0
    for name, shp in shapes:
        cnt = int(np.prod(shp))
        out[name] = np.frombuffer(raw, dtype=np.float64, count=cnt, offset=off).reshape(shp).copy()
        off += 8 * cnt
    ints = np.frombuffer(raw, dtype=np.int32, offset=off)
    assert ints.size == 5 * B
    for i, name in enumerate(("steps", "st_polish", "st_jvp", "st_bwd", "st_jac")):
        out[name] = ints[i * B:(i + 1) * B].copy()
    return out


def same_bits(a, b):
    """Equal as bit patterns but for the payload of a NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=True)) and bool(
        np.array_equal(np.signbit(a[~np.isnan(a)]), np.signbit(b[~np.isnan(b)])))


FLOAT_KEYS = ("x_out", "resid", "dx", "gP", "gq", "ga", "gb", "Jq", "Ja", "Jb")
INT_KEYS = ("steps", "st_polish", "st_jvp", "st_bwd", "st_jac")
