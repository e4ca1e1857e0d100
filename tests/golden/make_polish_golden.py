"""Writes tests/golden/polish/*.npz: the batches on which the polish's numpy restatement is measured (tests/polish_cases.py:
RESIDUAL_CPU) -- polish_cases.problem / figure_workload as one host computed them, frozen.  Those builders go through
torch.linalg.eigh, a matrix product and the oracle's compiled forward, whose last bits differ from host to host; a residual
of a few ulps, taken as the maximum over several hundred problems, moves in its first digit with them.  The restatement itself is
elementwise IEEE arithmetic: on frozen inputs its measurement is the same everywhere.  A diagonal P is stored as its diagonal.
usage (from tests/): python golden/make_polish_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import polish_cases as C   # noqa: E402


def main():
    os.makedirs(C.GOLDEN, exist_ok=True)
    for kind, N, structure in C.BATCHES:
        d, x = C.problem(kind, N, C.B_CPU, structure)
        out = {k: v for k, v in d.items()}
        if structure == "diag":
            out["P"] = C.compact(d["P"])
        np.savez(C.golden_path(kind, N, structure), x=x, **out)
    d, x = C.figure_workload()
    np.savez(C.golden_path("qp", 8, "figure"), x=x, P=C.compact(d["P"]), q=d["q"])


if __name__ == "__main__":
    main()
