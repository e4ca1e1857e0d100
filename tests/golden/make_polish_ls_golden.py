"""Writes tests/golden/polish_ls/*.npz: the cold-start batches on which the damped polish's numpy restatement is counted
(tests/polish_ls_reference.py: ROWS, COUNTS), frozen because QR and the matrix products below differ in their last bits from host
to host while the restatement on given inputs is elementwise IEEE arithmetic.  Per row B_COLD problems:
  dense rows    P = Q diag(exp(U(0, ln 60))) Q', Q from the QR of a normal matrix, symmetrised
  figure rows   P = diag(exp(U(-10, 10))), stored as its diagonal (the reference's figure family, here with a box)
  q ~ U(-1, 1);  l_min = -U(.01, 1), l_max = +U(.01, 1);  l_n, mu ~ U(.1, 1);  v ~ N(0, 1)
one numpy.random.default_rng(SEED) through all rows in ROWS' order.  Prints the counts to put into COUNTS.
usage (from tests/): python golden/make_polish_ls_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import polish_ls_reference as L   # noqa: E402

SEED = 1
KAPPA = 60.0


def extras(r, kind, B, n):
    if kind == "qcqp":
        return {"l_n": r.uniform(0.1, 1.0, (B, n // 2)), "mu": r.uniform(0.1, 1.0, (B, n // 2))}
    if kind == "qp":
        return {}
    d = {"l_min": -r.uniform(0.01, 1.0, (B, n)), "l_max": r.uniform(0.01, 1.0, (B, n))}
    if kind == "sbox":
        d["v"] = r.standard_normal((B, n))
    return d


def main():
    os.makedirs(L.GOLDEN, exist_ok=True)
    r = np.random.default_rng(SEED)
    for name, kind, n in L.ROWS:
        B = L.B_COLD
        if "figure" in name:
            P = np.exp(r.uniform(-10.0, 10.0, (B, n)))
        else:
            P = np.empty((B, n, n))
            for b in range(B):
                Q, _ = np.linalg.qr(r.standard_normal((n, n)))
                M = (Q * np.exp(r.uniform(0.0, np.log(KAPPA), n))[None, :]) @ Q.T
                P[b] = 0.5 * (M + M.T)
        q = r.uniform(-1.0, 1.0, (B, n))
        np.savez(L.golden_path(name), P=P, q=q, **extras(r, kind, B, n))
        Pf, qf, ex, x = L.frozen(name, kind)
        print('    "%s": (%d, %d),' % (name, *(int(L.converged(Pf, qf, L.polish_ls_batch(kind, Pf, qf, ex, x, L.MAX_STEPS, h)).sum())
                                             for h in (0, 8))))


if __name__ == "__main__":
    main()
