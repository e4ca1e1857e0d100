"""Prints the two records of the smoothed Newton Jacobians' tests (tests/jac_smooth_cases.py: FINITE_DIFF, ADJOINT_GAP), measured
with the numpy restatement (tests/jac_smooth_reference.py) on the dense batches frozen under tests/golden/smooth
(tests/golden/make_smooth_golden.py wrote them; this script writes no file): every column of Jq, Ja, Jb at kappa = 1e-2 against
central differences of the smoothed polish's own solution, and ops.newton_jacobian_vjp of the restated Jacobians against the
restated smoothed backward.
usage (from tests/): python golden/make_jac_smooth_golden.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import jac_smooth_cases as C     # noqa: E402


def main():
    for kind in C.KINDS:
        print("%-5s finite differences %.3g   adjoint gap %.3g" % (kind, C.fd_gap(kind), C.adjoint_gap(kind)))
    for name, val in C.measured().items():
        print(name, "= %.3g" % val)


if __name__ == "__main__":
    main()
