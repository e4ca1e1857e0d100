"""numpy restatement of the solution check's DEFINITIONS (include/diffqcqp_hip.h, dqq_check_f64), written from the definitions
and not from the kernel: plain numpy sums in numpy's order.  Shared by tests/test_check_hostcore.py and tests/test_gpu_check.py,
with the batch generator, the derived tolerance and the loader of the host-compiled core.

Tolerance (derived, not tuned): a sum of m terms carries at most m 2^-53 relative error on the sum of absolute values, so
per problem   bound = 4 (N + 2) 2^-52 (max|P||x| + max|q| + max|x|)   for resid[0], [1], [3], and N * bound * max|x| for the
objective."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KINDS = ("qp", "qcqp", "box", "sbox")
KIND_ID = {"qp": 0, "qcqp": 1, "box": 2, "sbox": 3}
AUTO, DENSE, DIAG = 0, 1, 2
D = ctypes.POINTER(ctypes.c_double)


def project(kind, t, extras):
    """Euclidean projection of t (B,N) onto the kind's feasible set."""
    if kind == "qp":
        return np.maximum(t, 0.0)
    if kind in ("box", "sbox"):
        t = np.minimum(np.maximum(t, extras[0]), extras[1])
        if kind == "sbox":
            sg = np.sign(extras[2])
            t = sg * np.minimum(sg * t, 0.0)
        return t
    r = extras[0] * extras[1]                       # (B,N/2)
    a, b = t[:, 0::2], t[:, 1::2]
    n2 = a * a + b * b
    with np.errstate(all="ignore"):
        sc = np.where(n2 > r * np.abs(r), r / np.sqrt(n2), 1.0)
    out = np.empty_like(t)
    out[:, 0::2], out[:, 1::2] = a * sc, b * sc
    return out


def reference(kind, P, q, extras, x, iters=None, max_iter=None, diag=False):
    """-> (status (B) int, resid (B,4)).  P (B,N,N), or (B,N) with diag; q, x (B,N); extras: tuple of (B,N) / (B,N/2) arrays."""
    with np.errstate(all="ignore"):
        if diag:
            Px, aPx = P * x, np.abs(P) * np.abs(x)
        else:
            Px, aPx = np.einsum("bij,bj->bi", P, x), np.einsum("bij,bj->bi", np.abs(P), np.abs(x))
        g = Px + q
        B = x.shape[0]
        resid = np.empty((B, 4))
        resid[:, 0] = np.abs(x - project(kind, x - g, extras)).max(axis=1)
        resid[:, 1] = np.abs(x - project(kind, x, extras)).max(axis=1)
        resid[:, 2] = 0.5 * (x * Px).sum(axis=1) + (q * x).sum(axis=1)
        resid[:, 3] = np.maximum(aPx.max(axis=1), np.abs(q).max(axis=1))
    status = np.zeros(B, dtype=np.int32)
    if iters is not None:
        status[np.asarray(iters) >= max_iter] = 1
    status[~(np.isfinite(x).all(axis=1) & np.isfinite(resid).all(axis=1))] = 2
    return status, resid


def bounds(P, q, x, diag=False):
    """-> (bound (B) for resid[0], [1], [3]; bound (B) for the objective), from the inputs (module docstring)."""
    N = x.shape[1]
    with np.errstate(all="ignore"):
        aPx = np.abs(P) * np.abs(x) if diag else np.einsum("bij,bj->bi", np.abs(P), np.abs(x))
        xm = np.abs(x).max(axis=1)
        b = 4.0 * (N + 2) * 2.0 ** -52 * (aPx.max(axis=1) + np.abs(q).max(axis=1) + xm)
    return b, N * b * xm


def assert_close(resid, ref, P, q, x, diag=False, what=""):
    """resid against the numpy evaluation within the derived bounds; a non-finite reference entry must be non-finite."""
    b, bo = bounds(P, q, x, diag)
    for k in range(4):
        tol = bo if k == 2 else b
        fin = np.isfinite(ref[:, k])
        assert not np.isfinite(resid[~fin, k]).any(), "%s resid[%d]: finite where the definition is not" % (what, k)
        err = np.abs(resid[fin, k] - ref[fin, k])
        bad = err > tol[fin]
        assert not bad.any(), "%s resid[%d]: error %.3e over the derived bound %.3e" % (
            what, k, err[bad].max(), tol[fin][bad].min())


def make_batch(kind, B, N, seed, diag=False):
    """A seeded batch with an x that is neither optimal nor feasible: (P, q, extras, x) as float64 numpy arrays, P (B,N,N) or
    (B,N)."""
    r = np.random.default_rng(seed)
    if diag:
        P = r.uniform(0.1, 1.1, (B, N))
    else:
        S = r.uniform(-1.0, 1.0, (B, N, N))
        P = S @ S.transpose(0, 2, 1) / N + 0.1 * np.eye(N)
        P += 0.01 * r.uniform(-1.0, 1.0, (B, N, N))   # not symmetric: g = P x + q reads rows
    q = r.uniform(-1.0, 1.0, (B, N))
    x = r.uniform(-1.0, 1.0, (B, N))
    if kind == "qp":
        extras = ()
    elif kind == "qcqp":
        extras = (r.uniform(0.0, 1.0, (B, N // 2)), r.uniform(0.0, 1.0, (B, N // 2)))
    else:
        extras = (-0.6 * r.uniform(0.5, 1.5, (B, N)), 0.6 * r.uniform(0.5, 1.5, (B, N)))
        if kind == "sbox":
            v = r.uniform(-1.0, 1.0, (B, N))
            v[:, 0] = 0.0                                # sign(0) = 0 pins a coordinate to 0
            extras += (v,)
    return P, q, extras, x


def hostcore():
    """The host-compiled core (tests/hostcore/check_core_check.cpp over diffqcqp_amd/csrc/check_core.h and route.cpp)."""
    src = os.path.join(HERE, "hostcore", "check_core_check.cpp")
    so = os.path.join(HERE, "hostcore", "libcheckcore.so")
    csrc = os.path.join(ROOT, "diffqcqp_amd", "csrc")
    deps = [src, os.path.join(ROOT, "include", "diffqcqp_hip.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fvisibility=hidden",
                               "-o", so + ".tmp", src])
        os.replace(so + ".tmp", so)
    lib = ctypes.CDLL(so)
    lib.hostcheck.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, D, D, D, D, D, D, ctypes.c_int, ctypes.c_int,
                              ctypes.c_int, D]
    lib.hostcheck_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    return lib


def host_check(lib, kind, P, q, extras, x, iters=None, max_iter=0, diag=False):
    """The host core over a batch -> (status, resid), the arithmetic the device runs, one problem at a time."""
    B, N = x.shape
    P, q, x = (np.ascontiguousarray(a, dtype=np.float64) for a in (P, q, x))
    ex = [np.ascontiguousarray(e, dtype=np.float64) for e in extras] + [None] * (3 - len(extras))
    status, resid = np.empty(B, dtype=np.int32), np.empty((B, 4))
    p = lambda a, b: None if a is None else a[b].ctypes.data_as(D)
    for b in range(B):
        status[b] = lib.hostcheck(KIND_ID[kind], int(diag), N, p(P, b), p(q, b), p(ex[0], b), p(ex[1], b), p(ex[2], b),
                                  p(x, b), int(iters is not None), 0 if iters is None else int(iters[b]), int(max_iter),
                                  resid[b].ctypes.data_as(D))
    return status, resid


def same_bits(a, b):
    """Bit for bit, except that any NaN equals any NaN: which NaN an invalid operation produces (sign, payload) is the
    processor's choice, not the arithmetic's."""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | nan).all())
