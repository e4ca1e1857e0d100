"""CPU check of the forward-mode helpers of diffqcqp_amd/csrc/bwd_systems.h (transposed accessors, R^T, rhs^T) plus the
refinement, run on one thread by tests/hostcore/jvp_check.cpp, against the numpy restatement tests/jvp_reference.py -- at the
bar the backward's host core is held to against the oracle (tests/test_bwd_systems_hostcore.py): bit-equal.  The host build is
a test artefact; the product never calls it."""
import numpy as np
import pytest

import jvp_cases as C
import jvp_reference as R

CASES = [("qp", 5), ("qp", 8), ("qcqp", 4), ("qcqp", 6), ("box", 3), ("box", 4), ("sbox", 3), ("sbox", 4)]
B = 32


@pytest.mark.parametrize("structure", ["dense", "diag"])
@pytest.mark.parametrize("kind,N", CASES)
def test_host_core_is_the_numpy_restatement_bit_for_bit(oracle, kind, N, structure):
    d, x = C.problem(kind, N, B, structure)
    P, q, ex = R.flat(d, kind)
    tan = R.random_tangents(kind, B, N, 11)
    ref_dx, ref_steps = R.jvp_batch(kind, P, q, ex, x[:, :, 0], tan)
    dx, steps = C.host_jvp(kind, d, x, tan)
    assert np.array_equal(dx, ref_dx) and np.array_equal(steps, ref_steps.reshape(steps.shape))
    assert np.abs(dx).max() > 1e-3      # (not a comparison of zeros)
    # a NULL tangent is a zero tangent, bit for bit; each tangent alone
    for i in range(len(tan)):
        only = tuple(t if j == i else None for j, t in enumerate(tan))
        zeros = tuple(t if j == i else np.zeros_like(t) for j, t in enumerate(tan))
        a, _ = C.host_jvp(kind, d, x, only)
        b, _ = C.host_jvp(kind, d, x, zeros)
        assert np.array_equal(a, b) and np.array_equal(a, R.jvp_batch(kind, P, q, ex, x[:, :, 0], only)[0]), i
    assert not C.host_jvp(kind, d, x, (None,) * len(tan))[0].any()
