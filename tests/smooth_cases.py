"""Inputs and host-side yardsticks of the smoothed Newton family's tests -- tests/test_smooth_*.py on the CPU,
tests/test_gpu_smooth.py on the device.  Not a test file.  Problems: tests/polish_ls_cases.py's recipe (cold starts x = PI(0)).
The yardstick of the kernels is the host core (tests/hostcore/smooth_core_check.cpp: smooth_core.h's *_problem_smooth functions on
one CPU thread, a stand-alone program), itself held bit-equal to the numpy restatement tests/smooth_reference.py.  Two builds of
that program: a plain one, the yardstick of the device tests, and one with the address and undefined-behaviour sanitizers that
only the CPU test tests/test_smooth_hostcore.py runs.

The three measured tolerances: each is the worst value the numpy restatement reaches on the batches frozen under
tests/golden/smooth (N = 8, 32 problems, every kind that the quantity exists for, kappa in KAPPAS; `measured` below), as
`python tests/golden/make_smooth_golden.py` prints them; the tests hold to 10 x the record, the margin DESIGN 4.11 uses for AGREE_CPU."""
import functools
import os
import subprocess
import tempfile

import numpy as np

import polish_ls_cases as C
import polish_reference as R
import smooth_reference as S

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = C.KINDS
KAPPAS = (1e-4, 1e-2)
MAX_STEPS = 12           # of the device tests
SOLVE_STEPS, SOLVE_HALVINGS = 60, 8      # "the smoothed point" of the property tests
MARGIN = 10.0

# the batches the records below are taken on, frozen under tests/golden/smooth (tests/golden/make_smooth_golden.py): (kind, structure)
GOLDEN = os.path.join(HERE, "golden", "smooth")
N, B = 8, 32
ROWS = [(k, "dense") for k in C.KINDS] + [("qp", "diag")]
CONVERGED = 1e-13        # r (hard or smoothed) of a point that counts as a solution on these batches (|x|, |g| are O(1))

# the records, per kappa in KAPPAS' order (python tests/golden/make_smooth_golden.py prints them), on the frozen batches, at the
# smoothed point reached from the frozen hard solution xh -- what qcqp-level callers do: solve, then the smoothed polish
#   central path: max |x_i g_i - kappa^2| / kappa^2 over the two QP batches
#   adjoint gap:  max |<grad_x, dx> - <grads, tangents>| / (|<grad_x, dx>| + |<grads, tangents>| + tiny) over the dense batches
#   finite differences: max |dx_jvp - dx_fd|_inf / (|dx_jvp|_inf + 1) over the dense batches, central differences of the smoothed
#                 polish's own solution at step FD_STEP; every base and moved point must have converged (fd_gap asserts it), and
#                 no problem is left out
CENTRAL_PATH = {1e-4: 9.55e-07, 1e-2: 1.25e-10}
ADJOINT_GAP = {1e-4: 1.78e-13, 1e-2: 5.63e-13}
FINITE_DIFF = {1e-4: 1.65e-09, 1e-2: 2.3e-09}
FD_STEP = {1e-4: 1e-7, 1e-2: 1e-6}

same_bits = C.same_bits
compact = C.compact
problem = C.problem
# the device tables: the damped polish's (tests/polish_ls_cases.py)
DIAG_ROWS, TEAM_ROWS, ANY_ROWS, TEAM_BS, ANY_B = C.DIAG_ROWS, C.TEAM_ROWS, C.ANY_ROWS, C.TEAM_BS, C.ANY_B
DIAG_MATRIX_N, diag_bs, team_layout = C.DIAG_MATRIX_N, C.diag_bs, C.team_layout
ENTRIES = ("polish_smooth", "bwd_smooth", "jvp_smooth")     # family_checks of the device test runs all three on every row
# (entry, the parent entry whose geometry it launches with, kind, N) of tests/test_gpu_smooth_trips.py
TRIP_ROWS = [(e, p, k, N) for e, p, kinds in (("polish", "polish_ls", ("qp", "qcqp", "box", "sbox", "qp", "sbox")),
                                              ("bwd", "bwd", ("qcqp", "box", "sbox", "qp", "qcqp", "box")),
                                              ("jvp", "jvp", ("box", "sbox", "qp", "qcqp", "box", "qcqp")))
             for k, N in zip(kinds, (6, 20, 34, 64, 66, 12))]
_EXTRAS = {"qp": (), "qcqp": ("l_n", "mu"), "box": ("l_min", "l_max"), "sbox": ("l_min", "l_max", "v")}


def golden_path(kind, structure):
    return os.path.join(GOLDEN, "%s_%s_n%d.npz" % (kind, structure, N))


@functools.lru_cache(maxsize=None)
def frozen(kind, structure="dense"):
    """-> (P (B,N,N), q, ex, x: the cold start, xh: the hard solution, (dP, dq, da, db, gx)) of a frozen row, read-only."""
    with np.load(golden_path(kind, structure)) as z:
        get = lambda k: np.ascontiguousarray(z[k]) if k in z.files else None     # noqa: E731
        out = (get("P"), get("q"), tuple(get(k) for k in _EXTRAS[kind]), get("x"), get("xh"),
               (get("dP"), get("dq"), get("da"), get("db"), get("gx")))
    for a in (out[0], out[1], out[3], out[4]) + out[2] + out[5]:
        if a is not None:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def hostcore(sanitized=False):
    """The host program's path, built on demand.  sanitized: the build with -fsanitize=address,undefined -- for CPU tests only;
    a test marked gpu uses the plain build."""
    src = os.path.join(HERE, "hostcore", "smooth_core_check.cpp")
    exe = os.path.join(HERE, "hostcore", "smooth_core_check_san" if sanitized else "smooth_core_check")
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else ["-O2"]
    deps = [src] + [os.path.join(HERE, "..", "diffqcqp_amd", "csrc", f)
                    for f in ("smooth_core.h", "newton_core.h", "polish_core.h", "check_core.h", "sbox_bounds.h", "common.h", "route.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(p) > os.path.getmtime(exe) for p in deps):
        subprocess.check_call(["g++"] + extra + ["-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", exe + ".tmp", src])
        os.replace(exe + ".tmp", exe)
    return exe


def _run(mode, kind, P, q, ex, x, more, max_steps, in_place, max_halvings, given, reg, kappa, diag, sanitized):
    B, N = x.shape
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in (P, q) + tuple(ex) + (x,) + tuple(more)]
    assert arrays[0].shape == ((B, N) if diag else (B, N, N))
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        with open(fin, "wb") as f:
            f.write(np.array([mode, R.KIND[kind], B, N, int(diag), max_steps, int(in_place), max_halvings, given], dtype=np.int32).tobytes())
            f.write(np.array([reg, kappa], dtype=np.float64).tobytes())
            for a in arrays:
                f.write(a.tobytes())
        subprocess.check_call([hostcore(sanitized), fin, fout])
        return open(fout, "rb").read()


def host_polish(kind, P, q, ex, x, max_steps=MAX_STEPS, max_halvings=8, reg=0.0, kappa=0.0, diag=False, in_place=False, sanitized=False):
    """-> x_out (B,N), resid (B,2), steps, status, halvings (B) int32"""
    B, N = x.shape
    raw = _run(0, kind, P, q, ex, x, (), max_steps, in_place, max_halvings, 0, reg, kappa, diag, sanitized)
    nd = B * N + 2 * B
    dbl, ints = np.frombuffer(raw[: 8 * nd], dtype=np.float64), np.frombuffer(raw[8 * nd:], dtype=np.int32)
    assert ints.size == 3 * B
    return (dbl[: B * N].reshape(B, N).copy(), dbl[B * N:].reshape(B, 2).copy(), ints[:B].copy(), ints[B:2 * B].copy(), ints[2 * B:].copy())


def host_backward(kind, P, q, ex, x, gx, reg=0.0, kappa=0.0, diag=False, sanitized=False):
    """-> grad_P (as P), grad_q (B,N), grad_a, grad_b ((B,.) or None for the QP), status (B) int32"""
    B, N = x.shape
    raw = _run(1, kind, P, q, ex, x, (gx,), 0, False, 0, 0, reg, kappa, diag, sanitized)
    npp = B * N if diag else B * N * N
    ne = 0 if kind == "qp" else (B * N // 2 if kind == "qcqp" else B * N)
    nd = npp + B * N + 2 * ne
    dbl, ints = np.frombuffer(raw[: 8 * nd], dtype=np.float64), np.frombuffer(raw[8 * nd:], dtype=np.int32)
    assert ints.size == B
    gP = dbl[:npp].reshape((B, N) if diag else (B, N, N)).copy()
    gq = dbl[npp:npp + B * N].reshape(B, N).copy()
    ga = gb = None
    if ne:
        ga = dbl[npp + B * N:npp + B * N + ne].reshape(B, -1).copy()
        gb = dbl[npp + B * N + ne:].reshape(B, -1).copy()
    return gP, gq, ga, gb, ints.copy()


def host_jvp(kind, P, q, ex, x, dP=None, dq=None, da=None, db=None, reg=0.0, kappa=0.0, diag=False, sanitized=False):
    """-> dx (B,N), status (B) int32"""
    B, N = x.shape
    tang = (dP, dq, da, db)
    given = sum(1 << i for i, t in enumerate(tang) if t is not None)
    raw = _run(2, kind, P, q, ex, x, tuple(t for t in tang if t is not None), 0, False, 0, given, reg, kappa, diag, sanitized)
    dbl, ints = np.frombuffer(raw[: 8 * B * N], dtype=np.float64), np.frombuffer(raw[8 * B * N:], dtype=np.int32)
    assert ints.size == B
    return dbl.reshape(B, N).copy(), ints.copy()


@functools.lru_cache(maxsize=None)
def tangents(kind, N, B, structure="dense", seed=0):
    """-> (dP (B,N,N): symmetric, diagonal for a diagonal structure; dq (B,N); da, db (B,.) or None; grad_x (B,N)), read-only."""
    r = np.random.default_rng(4000 + 100 * R.KIND[kind] + N + 7919 * seed + (structure == "diag"))
    dP = r.standard_normal((B, N, N))
    dP = 0.5 * (dP + dP.transpose(0, 2, 1))
    if structure == "diag":
        dP = dP * np.eye(N)
    dq = r.standard_normal((B, N))
    ne = 0 if kind == "qp" else (N // 2 if kind == "qcqp" else N)
    da = r.standard_normal((B, ne)) if ne else None
    db = r.standard_normal((B, ne)) if ne else None
    gx = r.standard_normal((B, N))
    for a in (dP, dq, da, db, gx):
        if a is not None:
            a.setflags(write=False)
    return np.ascontiguousarray(dP), dq, da, db, gx


def smoothed_point(kind, P, q, ex, x, kappa):
    """The restatement's smoothed polish from x (a hard solution, or a smoothed point of a problem next to this one), run long:
    (x_kappa, resid, steps, status, halvings)."""
    return S.polish_batch(kind, P, q, ex, x, SOLVE_STEPS, SOLVE_HALVINGS, 0.0, kappa)


def converged_point(kind, P, q, ex, x, kappa):
    """smoothed_point's x_kappa, every problem of which must be a solution of the smoothed equation."""
    out = smoothed_point(kind, P, q, ex, x, kappa)
    assert (out[1][:, 1] <= CONVERGED).all(), "%s kappa %g: the smoothed polish left r_kappa = %.3g" % (kind, kappa, out[1][:, 1].max())
    return out[0]


def g_of(P, q, x):
    s = np.zeros(x.shape)
    for j in range(x.shape[1]):          # in index order, elementwise: the same bits on every host
        s = s + P[:, :, j] * x[:, j:j + 1]
    return s + q


def adjoint_gap(kind, P, q, ex, x, tang, kappa, reg=0.0):
    dP, dq, da, db, gx = tang
    dx, s1 = S.jvp_batch(kind, P, q, ex, x, dP, dq, da, db, reg, kappa)
    gP, gq, ga, gb, s2 = S.backward_batch(kind, P, q, ex, x, gx, reg, kappa)
    assert not s1.any() and not s2.any()
    lhs = (gx * dx).sum(axis=1)
    rhs = (gP * dP).sum(axis=(1, 2)) + (gq * dq).sum(axis=1)
    if ga is not None:
        rhs = rhs + (ga * da).sum(axis=1) + (gb * db).sum(axis=1)
    return float((np.abs(lhs - rhs) / (np.abs(lhs) + np.abs(rhs) + 1e-300)).max())


def fd_gap(kind, P, q, ex, xh, tang, kappa):
    """The smoothed JVP at the smoothed point against central differences of the smoothed polish's own solution, every problem
    of the batch (the map is smooth: nothing is set aside).  The base point is reached from the hard solution xh, the moved
    points from the base point; all three must have converged."""
    dP, dq, da, db, _ = tang
    h = FD_STEP[kappa]
    xs = converged_point(kind, P, q, ex, xh, kappa)
    dx, st = S.jvp_batch(kind, P, q, ex, xs, dP, dq, da, db, 0.0, kappa)
    assert not st.any()

    def moved(sign):
        e2 = tuple(e + sign * h * t if i < 2 else e for i, (e, t) in enumerate(zip(ex, (da, db, None))))
        return converged_point(kind, P + sign * h * dP, q + sign * h * dq, e2, xs, kappa)

    fd = (moved(1.0) - moved(-1.0)) / (2.0 * h)
    return float((np.abs(dx - fd).max(axis=1) / (np.abs(dx).max(axis=1) + 1.0)).max())


def central_path_gap(P, q, xh, kappa):
    xs = converged_point("qp", P, q, (), xh, kappa)
    return float((np.abs(xs * g_of(P, q, xs) - kappa * kappa) / (kappa * kappa)).max())


def measured():
    """-> {name: {kappa: worst value}} on the frozen batches."""
    out = {"CENTRAL_PATH": {}, "ADJOINT_GAP": {}, "FINITE_DIFF": {}}
    for kappa in KAPPAS:
        cp, ag, fd = 0.0, 0.0, 0.0
        for kind, structure in ROWS:
            P, q, ex, _, xh, tang = frozen(kind, structure)
            if kind == "qp":
                cp = max(cp, central_path_gap(P, q, xh, kappa))
            if structure == "dense":
                ag = max(ag, adjoint_gap(kind, P, q, ex, converged_point(kind, P, q, ex, xh, kappa), tang, kappa))
                fd = max(fd, fd_gap(kind, P, q, ex, xh, tang, kappa))
        out["CENTRAL_PATH"][kappa], out["ADJOINT_GAP"][kappa], out["FINITE_DIFF"][kappa] = cp, ag, fd
    return out


if __name__ == "__main__":
    for name, vals in measured().items():
        print(name, "= {%s}" % ", ".join("%g: %.3g" % kv for kv in vals.items()))
