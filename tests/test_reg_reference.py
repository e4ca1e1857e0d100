"""CPU checks of the proximal weight on the numpy restatement (tests/reg_reference.py): what the weight is for, on batches whose
free block is singular (tests/reg_cases.py), and what it costs on positive definite ones.  Every bar is derived, not measured; the
records of reg_cases.py are measured again here and held to their two digits."""
import numpy as np
import pytest

import jvp_cases as JC
import newton_cases as NC
import newton_reference as NR
import polish_cases as PC
import polish_reference as R
import reg_cases as C
import reg_reference as RR
from test_bwd_systems_hostcore import _oracle_backward

NAMES = {"qp": (), "qcqp": ("l_n", "mu"), "box": ("l_min", "l_max"), "sbox": ("l_min", "l_max", "v")}


@pytest.mark.parametrize("kind,N,mode", C.CPU_BATCHES)
def test_free_block_is_singular_and_x_solves(kind, N, mode):
    d = C.batch(kind, N, mode)
    for b in range(C.B):
        rank, size = C.free_rank(d, b)
        assert rank < size, (b, rank, size)
        assert np.linalg.eigvalsh(d["P"][b]).min() > -1e-12                      # positive semidefinite
        r = R.evaluate(kind, d["P"][b], d["q"][b], tuple(e[b] for e in d["ex"]), d["x"][b])[2]
        assert r <= 1e-13
    elements = N // 2 if kind == "qcqp" else N                 # contacts or coordinates
    active = elements // (4 if mode == "lowrank" else 2)      # a quarter or half of them
    per_element = 2 if kind == "qcqp" else 1                  # coordinates of an element
    assert d["free"].sum() == C.B * (elements - active) * per_element


@pytest.mark.parametrize("kind,N,mode", C.CPU_BATCHES)
def test_the_gap_and_its_closing(kind, N, mode):
    """reg = 0: status 1 or numbers beyond 1e8, per batch as recorded.  reg = 1e-7: status 0 and finite, every output of every
    mode; the two modes adjoint within the record."""
    d = C.batch(kind, N, mode)
    P, q, ex, x = d["P"], d["q"], d["ex"], d["x"]
    tan, g = C.inputs(kind, N, C.B)
    dx0, s0 = RR.jvp_batch(kind, P, q, ex, x, *tan, reg=0.0)
    one = s0 == 1
    huge = (s0 == 0) & (np.abs(np.nan_to_num(dx0)).max(axis=1) > 1e8)
    assert (one | huge).all()
    assert ("status1" if one.all() else "huge" if huge.all() else "mixed") == C.GAP_AT_ZERO[(kind, N, mode)]
    assert np.isnan(dx0[one]).all()
    dx, sj = RR.jvp_batch(kind, P, q, ex, x, *tan, reg=C.REG)
    grads = RR.backward_batch(kind, P, q, ex, x, g, reg=C.REG)
    assert not sj.any() and not grads[4].any()
    assert np.isfinite(dx).all() and all(np.isfinite(a).all() for a in grads[:4] if a is not None)
    gap = JC.adjoint_gap(g, dx, [grads[0], grads[1]] + ([grads[2], grads[3]] if kind != "qp" else []), tan)
    print("adjoint gap", kind, N, mode, gap)
    assert gap <= C.ADJOINT_GAP_CPU[kind] * 1.05
    if N == 8:
        J = RR.jacobian_batch(kind, P, q, ex, x, reg=C.REG)
        assert not J[3].any() and all(np.isfinite(a).all() for a in J[:3] if a is not None)


def test_adjoint_record():
    worst = dict.fromkeys(C.KINDS, 0.0)
    for kind, N, mode in C.CPU_BATCHES:
        d = C.batch(kind, N, mode)
        tan, g = C.inputs(kind, N, C.B)
        dx, _ = RR.jvp_batch(kind, d["P"], d["q"], d["ex"], d["x"], *tan, reg=C.REG)
        gr = RR.backward_batch(kind, d["P"], d["q"], d["ex"], d["x"], g, reg=C.REG)
        worst[kind] = max(worst[kind], JC.adjoint_gap(g, dx, [gr[0], gr[1]] + ([gr[2], gr[3]] if kind != "qp" else []), tan))
    assert {k: C.two_digits(v) for k, v in worst.items()} == C.ADJOINT_GAP_CPU


@pytest.mark.parametrize("kind,N,mode", C.CPU_BATCHES)
def test_tangents_in_the_range(kind, N, mode):
    """dq_F = P_FF s (zero elsewhere) has a solution of the unregularised system, and M_reg dx = rhs leaves
    |M dx - rhs| = reg |D dx| <= 8 reg |dx| per problem (max norms; D's entries are at most 1, a contact's row has two)."""
    d = C.batch(kind, N, mode)
    r = np.random.default_rng(5)
    for b in range(C.B):
        P, q, x = d["P"][b], d["q"][b], d["x"][b]
        ex = tuple(e[b] for e in d["ex"])
        f = np.nonzero(d["free"][b])[0]
        dq = np.zeros(N)
        dq[f] = P[np.ix_(f, f)] @ r.standard_normal(f.size)
        dx, st = RR.jvp(kind, P, q, ex, x, dq=dq, reg=C.REG)
        assert st == 0
        z, D, M = RR.setup(kind, P, q, ex, x, 0.0)
        rhs = RR.jvp_rhs(kind, z, D, ex, x, None, dq, None, None)
        assert np.abs(M @ dx - rhs).max() <= 8 * C.REG * np.abs(dx).max() + 64 * 2.3e-16 * np.abs(M).sum(axis=1).max() * np.abs(dx).max()


@pytest.mark.parametrize("kind,structure", NC.AGREE_BATCHES)
def test_positive_definite_bias(kind, structure):
    """On newton_cases' positive definite batches: dx_reg - dx_0 = -reg M_reg^-1 D dx_0, so |dx_reg - dx_0| <= 8 reg |M^-1| |dx_0|
    in the max norm (|M_reg^-1| <= 2 |M^-1| for reg |M^-1| <= 1/2; rounding takes the rest)."""
    _, P, q, ex, x = NC.agree_problem(kind, structure)
    tan, _ = C.inputs(kind, NC.AGREE_N, x.shape[0])
    dx0, s0 = NR.jvp_batch(kind, P, q, ex, x, *tan)
    dxr, sr = RR.jvp_batch(kind, P, q, ex, x, *tan, reg=C.REG)
    assert not s0.any() and not sr.any()
    for b in range(x.shape[0]):
        _, _, M = RR.setup(kind, P[b], q[b], tuple(e[b] for e in ex), x[b], 0.0)
        inv = np.abs(np.linalg.inv(M)).sum(axis=1).max()
        assert np.abs(dxr[b] - dx0[b]).max() <= 8 * C.REG * inv * np.abs(dx0[b]).max()


def test_reg_zero_is_the_parent():
    for kind, structure in NC.AGREE_BATCHES[:4]:
        _, P, q, ex, x = NC.agree_problem(kind, structure)
        tan, g = C.inputs(kind, NC.AGREE_N, x.shape[0])
        assert C.same_bits(RR.jvp_batch(kind, P, q, ex, x, *tan)[0], NR.jvp_batch(kind, P, q, ex, x, *tan)[0])
        for a, b in zip(RR.backward_batch(kind, P, q, ex, x, g), NR.backward_batch(kind, P, q, ex, x, g)):
            assert C.same_bits(a, b)
        assert C.same_bits(RR.polish_batch(kind, P, q, ex, x)[0], R.polish_batch(kind, P, q, ex, x)[0])
    P = np.array([[-0.0, 0.0], [0.0, 1.0]])
    assert np.signbit(RR.p_reg(P, 0.0)[0, 0]) and not np.signbit(RR.p_reg(P, 1e-7)[0, 0])


@pytest.mark.parametrize("kind", C.KINDS)
def test_polish_from_the_forward(kind):
    """From the oracle's forward at eps = 1e-3: r after <= r before everywhere, and the recorded number of problems reaches
    64 x 2.8e-16 of the check's scale within 8 and within 32 steps."""
    reached = [0, 0]
    for N, mode in C.POLISH_BATCHES:
        d = C.batch(kind, N, mode)
        P, q, ex = d["P"], d["q"], d["ex"]
        dd = {"P": np.ascontiguousarray(P), "q": np.ascontiguousarray(q[:, :, None])}
        dd.update({nm: np.ascontiguousarray(e[:, :, None]) for nm, e in zip(NAMES[kind], ex)})
        x0 = np.ascontiguousarray(PC.oracle_forward(kind, dd, PC.EPS_START, PC.MAX_ITER)[:, :, 0])
        scale = R.scale(P, q, x0)
        for i, steps in enumerate((8, 32)):
            _, rs, st, ss = RR.polish_batch(kind, P, q, ex, x0, steps, reg=C.REG)
            assert (rs[:, 1] <= rs[:, 0]).all() and (ss < 2).all()
            reached[i] += int((rs[:, 1] <= C.POLISH_BAR * scale).sum())
    print("polish reached", kind, reached)
    assert tuple(reached) == C.POLISH_REACHED[kind]


@pytest.mark.parametrize("kind", C.KINDS)
def test_agreement_with_the_oracles_backward_on_rank_deficient_inputs(oracle, kind):
    """The oracle's backward (Tikhonov weight 1e-7) against the Newton backward at reg = 1e-7 on the singular margin batches:
    the largest relative difference per kind, for a seeded cotangent and for one in the range of the free block, held to the
    records (measurements of two different regularisations, not bars)."""
    worst = {"any": 0.0, "range": 0.0}
    for N, mode in C.AGREE_BATCHES:
        d = C.batch(kind, N, mode)
        P, q, ex, x = d["P"], d["q"], d["ex"], d["x"]
        g = C.inputs(kind, N, C.B)[1]
        for which, gx in (("any", g), ("range", C.range_cotangent(d, g))):
            dd = {"P": np.ascontiguousarray(P), "q": np.ascontiguousarray(q[:, :, None]), "grad_x": np.ascontiguousarray(gx[:, :, None])}
            dd.update({nm: np.array(e[:, :, None]) for nm, e in zip(NAMES[kind], ex)})
            ref = _oracle_backward(oracle, kind, dd, np.ascontiguousarray(x[:, :, None]), 1e-10)
            got = RR.backward_batch(kind, P, q, ex, x, gx, reg=C.REG)
            assert not got[4].any()
            a = NC.agreement(kind, ref, got, range(C.B))
            print("agreement", kind, N, mode, which, "%.3g" % a)
            worst[which] = max(worst[which], a)
    assert C.two_digits(worst["any"]) == C.AGREE_REG_CPU[kind]
    assert C.two_digits(worst["range"]) == C.AGREE_REG_RANGE_CPU[kind]
