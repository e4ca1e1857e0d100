"""Inputs and host-side yardsticks of the polish path's tests -- tests/test_path_*.py on the CPU, tests/test_gpu_path*.py on the
device.  Not a test file.  Problems: tests/polish_ls_cases.py's recipe (cold starts x = PI(0)) and the batches frozen under
tests/golden/smooth.  The yardstick of the kernels is the host core (tests/hostcore/path_core_check.cpp: path_core.h's
polish_problem_path on one CPU thread, a stand-alone program), itself held bit-equal to the numpy restatement
tests/path_reference.py.  Two builds of that program: a plain one, the yardstick of the device tests, and one with the address
and undefined-behaviour sanitizers that only the CPU test tests/test_path_hostcore.py runs."""
import functools
import os
import subprocess
import tempfile

import numpy as np

import path_reference as PR
import polish_cases as PC
import polish_reference as R
import smooth_cases as SC

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = SC.KINDS
KAPPAS, STEPS, MAX_HALVINGS = PR.KAPPAS, PR.STEPS, PR.MAX_HALVINGS
# the schedules of the device tests: the default one; a short one that is not monotone, has a stage without budget and the hard
# stage in the middle; the longest one the entry takes
SHORT = ((1e-2, 0.0, 1e-1, 1e-3), (3, 2, 0, 3))
LONG = ((1.0, 1e-1, 3e-2, 1e-2, 1e-3, 1e-4, 0.0, 0.0), (1, 1, 1, 1, 1, 1, 1, 2))

# (kind, N, layout, structure, B) of tests/test_gpu_path.py: the compact diagonal at every compiled N (polish_cases has the sizes
# and ragged_b), then (B,N,N) at every team width and on scratch
DENSE, DIAG = PC.DENSE, PC.DIAG
ENTRIES = ("polish_path",)
ROWS = ([(k, N, DIAG, "diag", 70) for k in KINDS for N in PC.DIAG_N_FIRST] + [(k, N, DENSE, "dense", 37) for k in KINDS for N in (8, 20, 64, 66)] +
        [(k, N, DIAG, "diag", PC.ragged_b(N)) for k in KINDS for N in PC.DIAG_N_MORE] + [(k, PC.TEAM_N16, DENSE, "dense", 37) for k in KINDS])
DIAG_MATRIX_N, diag_bs = SC.DIAG_MATRIX_N, SC.diag_bs

same_bits = SC.same_bits
compact = SC.compact
problem = SC.problem
frozen = SC.frozen


def equal(got, ref):
    """Every output of a path call, bit for bit."""
    assert len(got) == len(ref) == 7
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype and same_bits(g, r), (g, r)


@functools.lru_cache(maxsize=None)
def hostcore(sanitized=False):
    """The host program's path, built on demand.  sanitized: the build with -fsanitize=address,undefined -- for CPU tests only;
    a test marked gpu uses the plain build."""
    src = os.path.join(HERE, "hostcore", "path_core_check.cpp")
    exe = os.path.join(HERE, "hostcore", "path_core_check_san" if sanitized else "path_core_check")
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else ["-O2"]
    deps = [src] + [os.path.join(HERE, "..", "diffqcqp_amd", "csrc", f)
                    for f in ("path_core.h", "smooth_core.h", "newton_core.h", "polish_core.h", "check_core.h", "sbox_bounds.h", "common.h",
                              "route.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(p) > os.path.getmtime(exe) for p in deps):
        subprocess.check_call(["g++"] + extra + ["-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", exe + ".tmp", src])
        os.replace(exe + ".tmp", exe)
    return exe


def host_path(kind, P, q, ex, x, kappas=KAPPAS, stage_steps=STEPS, max_halvings=MAX_HALVINGS, reg=0.0, diag=False, in_place=False,
              sanitized=False):
    """The host core over a batch.  P (B,N,N), or (B,N) with diag; q, x (B,N); ex each (B,.) -> x_out (B,N), resid (B,2), steps,
    status, halvings (B) int32, stage_resid (B,S,2), stage_steps (B,S) int32"""
    B, N = x.shape
    S = len(kappas)
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in (P, q) + tuple(ex) + (x,)]
    assert arrays[0].shape == ((B, N) if diag else (B, N, N)) and len(stage_steps) == S
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        with open(fin, "wb") as f:
            f.write(np.array([R.KIND[kind], B, N, int(diag), int(in_place), max_halvings, S], dtype=np.int32).tobytes())
            f.write(np.array([reg], dtype=np.float64).tobytes())
            f.write(np.array(kappas, dtype=np.float64).tobytes())
            f.write(np.array(stage_steps, dtype=np.int32).tobytes())
            for a in arrays:
                f.write(a.tobytes())
        subprocess.check_call([hostcore(sanitized), fin, fout])
        raw = open(fout, "rb").read()
    nd = B * N + 2 * B + 2 * B * S
    dbl, ints = np.frombuffer(raw[: 8 * nd], dtype=np.float64), np.frombuffer(raw[8 * nd:], dtype=np.int32)
    assert ints.size == 3 * B + B * S
    return (dbl[: B * N].reshape(B, N).copy(), dbl[B * N:B * N + 2 * B].reshape(B, 2).copy(), ints[:B].copy(), ints[B:2 * B].copy(),
            ints[2 * B:3 * B].copy(), dbl[B * N + 2 * B:].reshape(B, S, 2).copy(), ints[3 * B:].reshape(B, S).copy())


def chain(call, x, kappas, stage_steps):
    """The explicit chain over any single-stage polish: call(x, kappa, max_steps) -> (x_out, resid, steps, status, halvings), arrays
    of numpy.  -> the path's seven outputs, assembled as the entry's header states them."""
    B = x.shape[0]
    S = len(kappas)
    sres, sst = np.empty((B, S, 2)), np.empty((B, S), dtype=np.int32)
    steps, halvings, status0, cur = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), None, x
    for s in range(S):
        cur, rs, st, status, hv = call(cur, kappas[s], stage_steps[s])
        sres[:, s], sst[:, s] = rs, st
        steps, halvings = steps + st, halvings + hv
        status0 = status if s == 0 else status0
    status = np.where(status0 == 2, 2, np.where(steps > 0, 0, 1)).astype(np.int32)
    return cur, np.stack([sres[:, 0, 0], sres[:, -1, 1]], axis=1), steps, status, halvings, sres, sst
