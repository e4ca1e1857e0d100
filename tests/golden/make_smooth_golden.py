"""Writes tests/golden/smooth/*.npz: the batches on which the three tolerances of the smoothed Newton family are measured
(tests/smooth_cases.py: ROWS, CENTRAL_PATH, ADJOINT_GAP, FINITE_DIFF), frozen because the QR and the matrix products of the problem
recipe differ in their last bits from host to host while the restatement on given inputs is elementwise IEEE arithmetic.  Per row
32 problems at N = 8 of tests/polish_ls_cases.py's recipe (dense: condition number 60; diag: P = diag(exp(U(-3, 3)))), with
  x      the cold start PI(0)
  xh     the hard solution: the restatement's smoothed polish continued over kappa = 1e-1, 1e-2, 1e-3, 1e-4 and finished with
         the hard damped polish (every problem must reach r <= 1e-13 at every stage: the script stops otherwise)
  dP, dq, da, db, gx   the tangents and the cotangent of tests/smooth_cases.py's `tangents`
Prints the records to put into tests/smooth_cases.py.
usage (from tests/): python golden/make_smooth_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import smooth_cases as SC        # noqa: E402
import smooth_reference as S     # noqa: E402

EXTRAS = {"qp": (), "qcqp": ("l_n", "mu"), "box": ("l_min", "l_max"), "sbox": ("l_min", "l_max", "v")}


def hard_solution(kind, P, q, ex, x):
    cur = x
    for kappa in (1e-1, 1e-2, 1e-3, 1e-4, 0.0):
        out = S.polish_batch(kind, P, q, ex, cur, SC.SOLVE_STEPS, SC.SOLVE_HALVINGS, 0.0, kappa)
        assert (out[1][:, 1] <= SC.CONVERGED).all(), (kind, kappa, out[1][:, 1].max())
        cur = out[0]
    return cur


def main():
    os.makedirs(SC.GOLDEN, exist_ok=True)
    for kind, structure in SC.ROWS:
        P, q, ex, x = SC.problem(kind, SC.N, SC.B, structure)
        dP, dq, da, db, gx = SC.tangents(kind, SC.N, SC.B, structure)
        d = dict(P=P, q=q, x=x, xh=hard_solution(kind, P, q, ex, x), dP=dP, dq=dq, gx=gx)
        d.update(dict(zip(EXTRAS[kind], ex)))
        if da is not None:
            d.update(da=da, db=db)
        np.savez(SC.golden_path(kind, structure), **d)
    SC.frozen.cache_clear()
    for name, vals in SC.measured().items():
        print(name, "= {%s}" % ", ".join("%g: %.3g" % kv for kv in vals.items()))


if __name__ == "__main__":
    main()
