"""Inputs and host-side yardsticks of the smoothed Newton Jacobians' tests -- tests/test_jac_smooth_*.py on the CPU,
tests/test_gpu_jac_smooth*.py on the device.  Not a test file.  Problems: tests/smooth_cases.py's (polish_ls_cases' recipe, and
the batches frozen under tests/golden/smooth).  The yardstick of the kernels is the host core
(tests/hostcore/jac_smooth_core_check.cpp: csrc/smooth_core.h's newton_jac_problem_smooth on one CPU thread, loaded through
ctypes), itself held bit-equal to the numpy restatement tests/jac_smooth_reference.py.

The two measured tolerances, at kappa = KAPPA on the dense batches frozen under tests/golden/smooth (N = 8, 32 problems,
every kind), as `python tests/golden/make_jac_smooth_golden.py` prints them; the tests hold to MARGIN x the record."""
import ctypes
import functools
import os
import subprocess

import numpy as np

import jac_smooth_reference as JS
import polish_reference as R
import smooth_cases as SC
import smooth_reference as S

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "diffqcqp_amd", "csrc")
KINDS = SC.KINDS
KAPPAS = (0.0, 1e-4, 1e-2, 1.0)       # of the bit-equality tests on the CPU
REGS = (0.0, 1e-3)
KAPPA = 1e-2                          # of the measured tolerances and of the device rows
REG = 1e-3
MARGIN = SC.MARGIN
AUTO, DENSE, DIAG = 0, 1, 2

# the records (python tests/golden/make_jac_smooth_golden.py prints them), over the dense frozen batches, at the smoothed point
# reached from the frozen hard solution:
#   finite differences: max over problems and columns of |J[:, j] - fd_j|_inf / (|J[:, j]|_inf + 1), fd_j the central difference of the
#                 smoothed polish's own solution in the j-th entry of q / a / b at step SC.FD_STEP; every base and moved point must
#                 have converged (r_kappa <= SC.CONVERGED), and no problem is left out
#   adjoint gap:  max |vjp - backward|_inf / (|backward|_inf + 1) per gradient (P, q, a, b) and problem, ops.newton_jacobian_vjp of the
#                 restated Jacobians against smooth_reference.backward for the frozen cotangent gx
FINITE_DIFF = 1.63e-09
ADJOINT_GAP = 1.04e-15

# (kind, N, B) of tests/test_gpu_jac_smooth.py: every compiled size of the three families (a QCQP has an even N); B of 37 and 67 so
# that tiles and teams are ragged
DIAG_ROWS = [(k, N, 37 if N in (8, 32) else 67) for k in KINDS for N in (2, 4, 8, 16, 32, 64)]
TEAM_ROWS = [(k, N + (N % 2 if k == "qcqp" else 0), 67 if N in (8, 33) else 37) for k in KINDS for N in (3, 8, 12, 20, 33, 64)]
ANY_ROWS = [(k, 66, 37) for k in KINDS]
ENTRIES = ("jac_smooth",)
_D = ctypes.POINTER(ctypes.c_double)
_I = ctypes.POINTER(ctypes.c_int)

same_bits = SC.same_bits
compact = SC.compact
problem = SC.problem

_DEPS = ("smooth_core.h", "newton_core.h", "polish_core.h", "check_core.h", "sbox_bounds.h", "common.h")
_SRC = os.path.join(HERE, "hostcore", "jac_smooth_core_check.cpp")


def _stale(out, deps):
    return not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in deps)


@functools.lru_cache(maxsize=None)
def hostcore():
    """The host core as a shared library, built on demand (plain: the yardstick of the device tests too)."""
    so = os.path.join(HERE, "hostcore", "libjacsmoothcheck.so")
    if _stale(so, [_SRC] + [os.path.join(CSRC, f) for f in _DEPS]):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fvisibility=hidden",
                               "-Wno-unknown-pragmas", "-o", so + ".tmp", _SRC])
        os.replace(so + ".tmp", so)
    lib = ctypes.CDLL(so)
    lib.jac_smooth_batch.argtypes = [ctypes.c_int] * 4 + [_D] * 9 + [_I, ctypes.c_double, ctypes.c_double]
    lib.jvp_smooth_unit_batch.argtypes = [ctypes.c_int] * 4 + [_D] * 6 + [ctypes.c_int, _D, _D, _I, ctypes.c_double, ctypes.c_double]
    return lib


@functools.lru_cache(maxsize=None)
def hostcore_program(sanitized=False):
    """The same file as a stand-alone program; sanitized: with the address and undefined-behaviour sanitizers -- CPU tests only."""
    exe = os.path.join(HERE, "hostcore", "jac_smooth_core_check_san" if sanitized else "jac_smooth_core_check")
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else ["-O2"]
    if _stale(exe, [_SRC] + [os.path.join(CSRC, f) for f in _DEPS]):
        subprocess.check_call(["g++"] + extra + ["-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-DJAC_SMOOTH_CHECK_MAIN",
                                                 "-o", exe + ".tmp", _SRC])
        os.replace(exe + ".tmp", exe)
    return exe


def _p(a):
    return None if a is None else a.ctypes.data_as(_D)


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def extra_cols(kind, N):
    return JS.extra_cols(kind, N)


def out_shapes(kind, B, N, diag):
    """Shapes of (Jq, Ja, Jb) as include/diffqcqp_hip.h has them (Ja, Jb None for the QP)."""
    ne = extra_cols(kind, N)
    s = (((B, N, 2) if kind == "qcqp" else (B, N), (B, N), (B, N)) if diag else ((B, N, N), (B, N, ne), (B, N, ne)))
    return s if kind != "qp" else (s[0], None, None)


def host_jac(kind, P, q, ex, x, need=(True, True, True), diag=False, status=True, reg=0.0, kappa=0.0):
    """P (B,N,N), or (B,N) with diag; q, x (B,N); ex each (B,.) -> (Jq, Ja, Jb: None where not needed or the QP has none,
    status (B) int32)."""
    B, N = x.shape
    P, q, x = _c(P), _c(q), _c(x)
    assert P.shape == ((B, N) if diag else (B, N, N))
    ex = [_c(e) for e in ex] + [None] * (3 - len(ex))
    need = tuple(need) + (True,) * (3 - len(need))
    J = [np.full(s, 7.0) if s is not None and nd else None for s, nd in zip(out_shapes(kind, B, N, diag), need)]
    st = np.full(B, -1, dtype=np.int32)
    rc = hostcore().jac_smooth_batch(R.KIND[kind], B, N, int(diag), _p(P), _p(q), _p(ex[0]), _p(ex[1]), _p(ex[2]), _p(x), _p(J[0]),
                                     _p(J[1]), _p(J[2]), st.ctypes.data_as(_I) if status else None, reg, kappa)
    assert rc == 0
    return J[0], J[1], J[2], st


def subsets(kind):
    """Every non-empty subset of the outputs the kind has, as `need`."""
    n = 1 if kind == "qp" else 3
    return [tuple(bool(m >> i & 1) for i in range(3)) for m in range(1, 1 << n)]


def unit_tangents(kind, B, N, which, j):
    """smooth_reference.jvp_batch's (dP, dq, da, db) for the unit tangent e_j of input `which` (0 q, 1 a, 2 b)."""
    e = np.zeros((B, N if which == 0 else extra_cols(kind, N)))
    e[:, j] = 1.0
    t = [None, None, None, None]
    t[1 + which] = e
    return tuple(t)


def with_bad_rows(kind, P, q, ex, x, nan_at, inf_at):
    """Copies with a NaN in q of problem nan_at and an infinity in problem inf_at (an infinite bound / friction coefficient; the QP:
    in x)."""
    P, q, x = P.copy(), q.copy(), x.copy()
    ex = tuple(e.copy() for e in ex)
    q[nan_at, 1] = np.nan
    if kind == "qp":
        x[inf_at, 0] = np.inf
    else:
        ex[1][inf_at, 0] = np.inf
    return P, q, ex, x


# ---- the route plan, compiled for the host -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def route_lib():
    src = os.path.join(HERE, "hostcore", "jac_smooth_route_check.cpp")
    so = os.path.join(HERE, "hostcore", "libjacsmoothroute.so")
    if _stale(so, [src] + [os.path.join(CSRC, f) for f in ("route.cpp", "route.h", "tuning.h", "report.h", "worklist.h", "common.h")]):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-o", so + ".tmp", src])
        os.replace(so + ".tmp", so)
    lib = ctypes.CDLL(so)
    lib.jac_smooth_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_double, ctypes.c_double, _I]
    lib.jac_reg_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_double, _I]
    return lib


def plan(kind, N, B, p_layout, reg=0.0, kappa=KAPPA):
    """plan_newton_jac_smooth -> (err, family, route, scratch, reg, smooth, inf_bounds); kind: a name or a number"""
    out = (ctypes.c_int * 7)()
    route_lib().jac_smooth_plan(R.KIND.get(kind, kind), N, B, p_layout, reg, kappa, out)
    return tuple(out)


def plan_reg(kind, N, B, p_layout, reg=0.0):
    out = (ctypes.c_int * 7)()
    route_lib().jac_reg_plan(R.KIND.get(kind, kind), N, B, p_layout, reg, out)
    return tuple(out)


def family_ids():
    out = (ctypes.c_int * 64)()
    n = route_lib().jac_smooth_family_ids(out)
    return list(out[:n])


def team_width(N):
    return 8 if N <= 8 else 16 if N <= 16 else 32 if N <= 32 else 64 if N <= 64 else 256


def cell(kind, N, B, p_layout, reg=0.0, kappa=KAPPA):
    """-> (kind, form, size) of the NewtonJacSmooth kernel the call launches, from the plan -- None if it launches another family"""
    err, family, route, _, _, smooth, _ = plan(kind, N, B, p_layout, reg, kappa)
    first = family_ids()[-3]
    if err != 0 or not smooth or not first <= family < first + 3:
        return None
    form = ("diag", "team", "any")[family - first]
    assert route == family - first + 1
    return (kind, form, N if form == "diag" else team_width(N) if form == "team" else 0)


def device_rows():
    """(kind, N, B, layout) of every bit-equality row of tests/test_gpu_jac_smooth.py."""
    return ([(k, N, B, DIAG) for k, N, B in DIAG_ROWS] + [(k, N, B, DENSE if N == 8 else AUTO) for k, N, B in TEAM_ROWS] +
            [(k, N, B, DENSE) for k, N, B in ANY_ROWS])


# ---- the measured tolerances -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def smoothed_frozen(kind, kappa=KAPPA):
    """-> (P, q, ex, x_kappa, gx) of the dense frozen batch, x_kappa the restatement's converged smoothed point from the hard solution"""
    P, q, ex, _, xh, tang = SC.frozen(kind, "dense")
    xs = SC.converged_point(kind, P, q, ex, xh, kappa)
    xs.setflags(write=False)
    return P, q, ex, xs, tang[4]


@functools.lru_cache(maxsize=None)
def frozen_jacobians(kind, kappa=KAPPA):
    P, q, ex, xs, _ = smoothed_frozen(kind, kappa)
    out = JS.jacobians_batch(kind, P, q, ex, xs, (True, True, True), 0.0, kappa)
    assert not out[3].any()
    return out


@functools.lru_cache(maxsize=None)
def fd_columns(kind, kappa=KAPPA):
    """Central differences of the smoothed polish's own solution, column by column: (FDq (B,N,N), FDa, FDb (B,N,ne) or None)."""
    P, q, ex, xs, _ = smoothed_frozen(kind, kappa)
    B, N = xs.shape
    h = SC.FD_STEP[kappa]
    out = []
    for which in range(1 if kind == "qp" else 3):
        w = N if which == 0 else extra_cols(kind, N)
        fd = np.empty((B, N, w))
        for j in range(w):
            def moved(sign):
                if which == 0:
                    qm = q.copy()
                    qm[:, j] += sign * h
                    return SC.converged_point(kind, P, qm, ex, xs, kappa)
                em = [e.copy() for e in ex]
                em[which - 1][:, j] += sign * h
                return SC.converged_point(kind, P, q, tuple(em), xs, kappa)
            fd[:, :, j] = (moved(1.0) - moved(-1.0)) / (2.0 * h)
        out.append(fd)
    return tuple(out) + (None,) * (3 - len(out))


def fd_gap(kind, kappa=KAPPA):
    J, fd = frozen_jacobians(kind, kappa), fd_columns(kind, kappa)
    worst = 0.0
    for w in range(3):
        if fd[w] is not None:
            worst = max(worst, float((np.abs(J[w] - fd[w]).max(axis=1) / (np.abs(J[w]).max(axis=1) + 1.0)).max()))
    return worst


def rel_gap(got, ref):
    """max over problems of |got - ref|_inf / (|ref|_inf + 1); arrays (B, ...)"""
    B = ref.shape[0]
    return float((np.abs(got - ref).reshape(B, -1).max(axis=1) / (np.abs(ref).reshape(B, -1).max(axis=1) + 1.0)).max())


def adjoint_gap(kind, kappa=KAPPA):
    """ops.newton_jacobian_vjp (torch, on the CPU) of the restated Jacobians against the restated smoothed backward."""
    import torch
    from diffqcqp_amd import ops
    P, q, ex, xs, gx = smoothed_frozen(kind, kappa)
    J = frozen_jacobians(kind, kappa)
    ref = S.backward_batch(kind, P, q, ex, xs, gx, 0.0, kappa)
    assert not ref[4].any()
    Jt = tuple(None if j is None else torch.from_numpy(j) for j in J[:3])
    got = ops.newton_jacobian_vjp(kind, Jt, torch.from_numpy(xs.copy()).unsqueeze(-1), torch.from_numpy(gx.copy())[None, :, :, None], compact=False)
    worst = 0.0
    for g, r in zip(got, ref[:4]):
        if r is not None:
            worst = max(worst, rel_gap(g[0].numpy().reshape(r.shape), r))
    return worst


def measured():
    return {"FINITE_DIFF": max(fd_gap(k) for k in KINDS), "ADJOINT_GAP": max(adjoint_gap(k) for k in KINDS)}
