"""CPU checks of the numpy restatement of the Newton Jacobians (tests/jac_reference.py), which every other Jacobian test stands
on: every column against newton_reference's JVP of the unit tangent, Jq against numpy's own solve, and Jq against
newton_reference's backward through the adjoint identity -- the last two measured and held to the records in tests/jac_cases.py."""
import numpy as np
import pytest

import jac_cases as C
import jac_reference as JR
import newton_cases as NC
import newton_reference as NR


@pytest.mark.parametrize("kind,N,structure", C.BATCHES)
def test_every_column_is_the_jvp_of_its_unit_tangent(kind, N, structure):
    P, q, ex, x = NC.problem(kind, N, structure)
    B = x.shape[0]
    J = JR.jacobians_batch(kind, P, q, ex, x)
    assert not J[3].any()
    for which in range(1 if kind == "qp" else 3):
        for j in range(J[which].shape[2]):
            dx, st = NR.jvp_batch(kind, P, q, ex, x, *C.unit_tangents(kind, B, N, which, j))
            assert not st.any() and np.array_equal(J[which][:, :, j], dx, equal_nan=True), (which, j)
    if kind == "qp":
        assert J[1] is None and J[2] is None


@pytest.mark.parametrize("kind", C.KINDS)
def test_bad_problems_are_nan_where_the_jvp_is(kind):
    N = 8
    P, q, ex, x = NC.problem(kind, N, "dense")
    P, q, x = P.copy(), q.copy(), x.copy()
    ex = tuple(e.copy() for e in ex)
    P[3, 0, :] = 0.0                        # status 1: a zero row at a free coordinate (tests/test_newton_hostcore.py)
    x[3, 0], q[3, 0] = 0.01, -0.01
    if kind == "qcqp":
        P[3, 1, :] = 0.0
        P[3, 1, 1] = 1.0
        x[3, 1], q[3, 1] = 0.0, 0.0
        ex[0][3, 0], ex[1][3, 0] = 1.0, 1.0
    elif kind != "qp":
        ex[0][3, 0], ex[1][3, 0] = -1.0, 1.0
        if kind == "sbox":
            ex[2][3, 0] = -1.0
    q[7, 1] = np.nan
    if kind != "qp":
        ex[1][11, 0] = np.inf
    B = x.shape[0]
    J = JR.jacobians_batch(kind, P, q, ex, x)
    want = np.zeros(B, dtype=np.int32)
    want[3], want[7] = 1, 2
    if kind != "qp":
        want[11] = 2
    assert np.array_equal(J[3], want)
    for which in range(1 if kind == "qp" else 3):
        assert np.isnan(J[which][want != 0]).all() and np.isfinite(J[which][want == 0]).all()
        for j in (0, J[which].shape[2] - 1):
            dx, st = NR.jvp_batch(kind, P, q, ex, x, *C.unit_tangents(kind, B, N, which, j))
            assert np.array_equal(st, want) and np.array_equal(J[which][:, :, j], dx, equal_nan=True)


@pytest.mark.parametrize("kind", C.KINDS)
def test_each_output_alone_has_the_same_bits(kind):
    P, q, ex, x = NC.problem(kind, 8, "dense")
    full = JR.jacobians_batch(kind, P, q, ex, x)
    for which in range(1 if kind == "qp" else 3):
        one = JR.jacobians_batch(kind, P, q, ex, x, tuple(i == which for i in range(3)))
        assert C.same_bits(one[which], full[which]) and all(one[i] is None for i in range(3) if i != which)


@pytest.mark.parametrize("kind", C.KINDS)
def test_jq_agrees_with_numpys_solve_as_recorded(kind):
    gaps = [C.solve_gap(k, N, s) for k, N, s in C.BATCHES if k == kind]
    print("%s: max |Jq + solve(M, D)| / scale %s (record %.2g)" % (kind, ["%.3g" % g for g in gaps], C.SOLVE_GAP_CPU[kind]))
    assert max(gaps) <= C.BAR * C.SOLVE_GAP_CPU[kind]


@pytest.mark.parametrize("kind", C.KINDS)
def test_jq_is_the_backwards_transpose_as_recorded(kind):
    gaps = [C.adjoint_gap(k, N, s) for k, N, s in C.BATCHES if k == kind]
    print("%s: |g'(Jq t) - grad_q't| / scale %s (record %.2g)" % (kind, ["%.3g" % g for g in gaps], C.JAC_ADJOINT_CPU[kind]))
    assert max(gaps) <= C.BAR * C.JAC_ADJOINT_CPU[kind]
