"""The damped polish (dqq_polish_ls_f64) restated in numpy: the step rule of diffqcqp_amd/csrc/polish_core.h's polish_problem_ls
a second time, over the element functions of tests/polish_reference.py (g, z, F, r, D, M, the elimination, PI).  Not a test
file.

Per problem: d from M d = -F as in polish_reference.polish (reg on the diagonal of P where M is formed); trial points
x_k = PI(x + t_k d) with t_k = 2^-k, k = 0 .. max_halvings, the product and the sum rounded one by one; the first k with
r(x_k) < r is accepted (a NaN is not); if none is, x is kept and the loop ends.  An accepted k counts one step and k halvings.
max_halvings = 0 is polish_reference.polish.  Also here: the cold-start batches frozen under tests/golden/polish_ls (written by
tests/golden/make_polish_ls_golden.py) and the counts the restatement reaches on them."""
import os

import numpy as np

import polish_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "polish_ls")
MAX_STEPS = 60                      # of the cold-start rows
BAR = 64 * 2.8e-16                  # polish_cases.BAR: r <= BAR * scale is "machine-precision KKT"
B_COLD = 30

# (name, kind, N): dense P with condition number 60, and the reference's figure family as a box problem (P diagonal)
ROWS = [("%s_k60_n%d" % (k, N), k, N) for k in ("qp", "qcqp", "box", "sbox") for N in (8, 20)] + [
    ("box_figure_n8", "box", 8), ("box_figure_n20", "box", 20)]
# problems of B_COLD that reach the bar from x = PI(0) in MAX_STEPS accepted steps: (max_halvings = 0, max_halvings = 8), as
# the restatement counts them on the frozen files (tests/test_polish_ls_reference.py counts them again)
COUNTS = {
    "qp_k60_n8": (19, 30),
    "qp_k60_n20": (9, 30),
    "qcqp_k60_n8": (1, 30),
    "qcqp_k60_n20": (0, 30),
    "box_k60_n8": (3, 30),
    "box_k60_n20": (0, 29),
    "sbox_k60_n8": (3, 28),
    "sbox_k60_n20": (0, 29),
    "box_figure_n8": (1, 13),
    "box_figure_n20": (0, 11),
}


def _with_reg(P, reg):
    if reg == 0.0:
        return P
    Pr = P.copy()
    i = np.arange(P.shape[0])
    Pr[i, i] = P[i, i] + reg
    return Pr


def polish_ls(kind, P, q, ex, x, max_steps=8, max_halvings=0, reg=0.0):
    """One problem.  -> (x_out, (r_before, r_after), steps, status, halvings)"""
    with np.errstate(all="ignore"):
        n = x.shape[0]
        ex = tuple(np.asarray(e, dtype=np.float64).reshape(-1) for e in ex)
        bad = not (np.isfinite(P).all() and np.isfinite(q).all() and np.isfinite(x).all() and all(np.isfinite(e).all() for e in ex))
        xc = x.copy()
        z, F, r0 = R.evaluate(kind, P, q, ex, xc)
        r, steps, halvings = r0, 0, 0
        if bad or not np.isfinite(r0):
            return xc, (r0, r0), 0, 2, 0
        Pm = _with_reg(P, reg)
        while steps < max_steps and r != 0.0:
            d = R.solve(R.newton_matrix(kind, Pm, R.jacobian(kind, z, ex, n)), -F)
            if d is None:
                break
            t, found = 1.0, None
            for k in range(max_halvings + 1):
                s = t * d
                xn = R.project(kind, xc + s, ex, n)
                zn, Fn, rn = R.evaluate(kind, P, q, ex, xn)
                if rn < r:
                    found = k
                    break
                t = 0.5 * t
            if found is None:
                break
            xc, z, F, r = xn, zn, Fn, rn
            steps += 1
            halvings += found
        return xc, (r0, r), steps, 0 if steps > 0 else 1, halvings


def polish_ls_batch(kind, P, q, ex, x, max_steps=8, max_halvings=0, reg=0.0):
    """P (B,n,n), q (B,n), ex each (B,.), x (B,n) -> x_out (B,n), resid (B,2), steps, status, halvings (B) int32"""
    B, n = x.shape
    xo, rs = np.empty((B, n)), np.empty((B, 2))
    st, ss, hs = np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32)
    for b in range(B):
        xo[b], rs[b], st[b], ss[b], hs[b] = polish_ls(kind, P[b], q[b], tuple(e[b] for e in ex), x[b], max_steps, max_halvings, reg)
    return xo, rs, st, ss, hs


def cold_start(kind, ex, B, n):
    """x = PI(0) per problem."""
    return np.stack([R.project(kind, np.zeros(n), tuple(e[b] for e in ex), n) for b in range(B)])


def golden_path(name):
    return os.path.join(GOLDEN, name + ".npz")


def frozen(name, kind):
    """-> (P (B,n,n), q (B,n), ex each (B,.), x (B,n): the cold start) of a frozen row; a diagonal P is stored as (B,n)."""
    with np.load(golden_path(name)) as z:
        P, q = np.ascontiguousarray(z["P"]), np.ascontiguousarray(z["q"])
        ex = tuple(np.ascontiguousarray(z[k]) for k in {"qp": (), "qcqp": ("l_n", "mu"), "box": ("l_min", "l_max"),
                                                        "sbox": ("l_min", "l_max", "v")}[kind])
    if P.ndim == 2:
        P = np.ascontiguousarray(np.stack([np.diag(v) for v in P]))
    B, n = q.shape
    return P, q, ex, cold_start(kind, ex, B, n)


def converged(P, q, out):
    """Per problem: status 0 and r_after within the bar of the problem's scale at x_out."""
    return (out[3] == 0) & (out[1][:, 1] <= BAR * R.scale(P, q, out[0]))
