"""CPU tests of the oracle (oracle/diffqcqp_oracle.c).

The reference has no test with an expected value, so the oracle is
pinned by properties and by the reference's own two checking methods: KKT
residuals (Solver.cpp:825,867 printouts) and finite differences
(test_script.py:34-43, Solver.cpp:830-851).  PARITY UNPINNED by reference outputs.
"""
import glob
import os

import numpy as np
import pytest
import torch

from conftest import make_problem

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# ref_*.npz / rd_*.npz (the reference's own matrices, rank-deficient P) have their own tests with scale-relative tolerances
GENERIC_FIXTURES = sorted(p for p in glob.glob(os.path.join(GOLDEN, "*.npz"))
                          if not os.path.basename(p).startswith(("ref_", "rd_")))


def test_seed5_inputs_match_the_constants_in_the_reference_comments():
    """test_script.py:23-29 inputs reproduce the four-digit constants left in comments at
    test_script.py:153-154 and Solver.cpp:783,796 (0.4979/0.3295/0.2432, -0.3661/-0.9514) -- INPUTS only: the reference
    holds no expected solution or gradient for them."""
    d = np.load(os.path.join(GOLDEN, "qp_seed5.npz"))
    P, q = d["P"][0], d["q"][0, :, 0]
    assert np.allclose(P, [[0.4979, 0.3295], [0.3295, 0.2432]], atol=5e-5)
    assert np.allclose(q, [-0.3661, -0.9514], atol=5e-5)
    torch.manual_seed(5)
    S = torch.rand(1, 2, 2, dtype=torch.float64) + 0.01
    assert np.array_equal(torch.bmm(S, S.transpose(1, 2)).numpy(), d["P"])


def test_seed5_solution_and_fd_gradient(oracle):
    """The FD check of test_script.py:23-43: analytic dP of x[1] vs central differences.  (The expected x, the 123
    iterations and grad_P[1,1] = -16.0827925 are SURVEY.md section 4's values, computed by the survey session's separate numpy
    restatement of Solver.cpp -- two readings of the source agreeing, not a reference output.)"""
    d = np.load(os.path.join(GOLDEN, "qp_seed5.npz"))
    P, q = d["P"][0], d["q"][0, :, 0]
    x, it = oracle.solveQP(P, q, np.zeros(2), 1e-12, 1e-7, 10000, True, return_iters=True)
    assert it == 123
    assert x[0] == 0.0 and abs(x[1] - 3.91173314626397) < 1e-9
    bl = oracle.solveDerivativesQP(P, q, x, np.array([0.0, 1.0]))
    grad_P = -np.outer(bl, x)
    fd = np.zeros((2, 2))
    for i in range(2):
        for j in range(2):
            e = np.zeros((2, 2))
            e[i, j] = 1e-8
            fd[i, j] = (oracle.solveQP(P + e, q, None, 1e-12, 1e-7, 10000)[1]
                        - oracle.solveQP(P - e, q, None, 1e-12, 1e-7, 10000)[1]) / 2e-8
    assert abs(grad_P[1, 1] + 16.0827925) < 1e-6
    assert np.allclose(grad_P, fd, atol=1e-4)


def test_readme_example_is_degenerate(oracle):
    """README.md:35-38: q >= 0 => x == 0 after ONE iteration, all gradients 0."""
    d = np.load(os.path.join(GOLDEN, "qp_readme.npz"))
    x, it = oracle.qp_fwd_batch(d["P"], d["q"], 1e-7, 1000)
    assert np.all(x == 0.0) and np.all(it == 1)
    gP, gq, _ = oracle.qp_bwd_batch(d["P"], d["q"], x, d["grad_x"])
    assert np.all(gP == 0.0) and np.all(gq == 0.0)


def test_diag_qp_closed_form_and_backward_identity(oracle):
    """x* = max(-q/p, 0) within the solver's accuracy; dl_i = p g/(p^2+1e-7) on the inactive set."""
    d = make_problem("qp", 512, 8, 11)
    P, q, g = d["P"].numpy(), d["q"].numpy(), d["grad_x"].numpy()
    p = np.diagonal(P, axis1=1, axis2=2)
    x, it = oracle.qp_fwd_batch(P, q, 1e-7, 1000)
    cf = np.maximum(-q[:, :, 0] / p, 0)
    err = np.abs(x[:, :, 0] - cf)
    assert np.median(err.max(1)) < 1e-6 and err.max() < 1e-3
    assert it.max() < 60
    gP, gq, steps = oracle.qp_bwd_batch(P, q, x, g)
    assert np.all(steps == 1)
    xx = x[:, :, 0]
    active = (xx <= 1e-10) & (-(p * xx + q[:, :, 0]) < -1e-10)
    dl = np.where(active, 0.0, p * g[:, :, 0] / (p * p + 1e-7))
    assert np.abs(-gq[:, :, 0] - dl).max() < 1e-13
    assert np.allclose(gP, -dl[:, :, None] * xx[:, None, :], atol=1e-15)


@pytest.mark.parametrize("structure,N", [("diag", 8), ("dense", 8), ("dense", 16)])
def test_qp_kkt(oracle, structure, N):
    """KKT of min 1/2 x'Px+q'x, x>=0: x>=0, Px+q>=0, x.(Px+q)=0 (to solver accuracy)."""
    d = make_problem("qp", 64, N, 21, structure)
    P, q = d["P"].numpy(), d["q"].numpy()
    x, _ = oracle.qp_fwd_batch(P, q, 1e-10, 100000)
    r = np.einsum("bij,bj->bi", P, x[:, :, 0]) + q[:, :, 0]
    assert x.min() >= 0.0
    assert r.min() > -1e-5
    assert np.abs(x[:, :, 0] * r).max() < 1e-5


@pytest.mark.parametrize("structure", ["diag", "dense"])
def test_qcqp_kkt(oracle, structure):
    """Feasibility + stationarity Px+q+2 gamma_i x_(i) = 0 with the recovered duals gamma >= 0."""
    N = 8
    d = make_problem("qcqp", 64, N, 22, structure)
    P, q, ln, mu = d["P"].numpy(), d["q"].numpy(), d["l_n"].numpy(), d["mu"].numpy()
    x, _ = oracle.qcqp_fwd_batch(P, q, ln, mu, 1e-10, 100000)
    r = (ln * mu)[:, :, 0]
    nrm = np.sqrt(x[:, 0::2, 0] ** 2 + x[:, 1::2, 0] ** 2)
    assert (nrm - r).max() < 1e-9
    for b in range(8):
        _, _, _, _, gam = oracle.solveDerivativesQCQP(P[b], q[b], ln[b], mu[b], x[b], np.zeros(N), return_steps=True)
        assert gam.min() > -1e-6
        stat = P[b] @ x[b, :, 0] + q[b, :, 0] + 2 * np.repeat(gam, 2) * x[b, :, 0]
        assert np.abs(stat).max() < 1e-4


def _fd(fun, arr, h):
    out = np.zeros_like(arr)
    it = np.nditer(arr, flags=["multi_index"])
    for _ in it:
        i = it.multi_index
        a, b = arr.copy(), arr.copy()
        a[i] += h
        b[i] -= h
        out[i] = (fun(a) - fun(b)) / (2 * h)
    return out


def test_qp_dense_fd_gradients(oracle):
    d = make_problem("qp", 4, 4, 31, "dense")
    for b in range(4):
        P, q, g = d["P"][b].numpy(), d["q"][b, :, 0].numpy(), d["grad_x"][b, :, 0].numpy()
        x = oracle.solveQP(P, q, None, 1e-13, 1e-7, 100000)
        bl = oracle.solveDerivativesQP(P, q, x, g)
        fq = _fd(lambda qq: g @ oracle.solveQP(P, qq, None, 1e-13, 1e-7, 100000), q, 1e-6)
        assert np.allclose(-bl, fq, atol=2e-4, rtol=1e-3)
        # The factorisation reads only the lower triangle of P (Eigen LLT, Solver.cpp:76), so P is
        # perturbed symmetrically and compared with grad_P[i,j] + grad_P[j,i].
        gP = -np.outer(bl, x)
        for i in range(4):
            for j in range(i + 1):
                e = np.zeros((4, 4))
                e[i, j] = e[j, i] = 1e-6
                fd = (g @ oracle.solveQP(P + e, q, None, 1e-13, 1e-7, 100000)
                      - g @ oracle.solveQP(P - e, q, None, 1e-13, 1e-7, 100000)) / 2e-6
                an = gP[i, i] if i == j else gP[i, j] + gP[j, i]
                assert abs(fd - an) < 2e-4 + 1e-3 * abs(an), (i, j, fd, an)


def test_qcqp_fd_gradients(oracle):
    """QCQP backward.  The reference solves the differentiated KKT system A^T b = [0; g] only in the
    Tikhonov sense, b = (A A^T + 1e-7 I)^-1 A [0; g] iterated 1 or 3 times (Solver.cpp:15-44), which is
    visibly inexact once cond(A)^2 * 1e-7 is not small.  So the check is split:
      (1) the restated KKT matrix is right: an EXACT solve with it matches finite differences;
      (2) the oracle output equals that (iterated) Tikhonov solution, and E1/E2 scale dgamma."""
    d = make_problem("qcqp", 4, 4, 32, "dense")
    n, nc = 4, 2
    for b in range(4):
        P, q, g = d["P"][b].numpy(), d["q"][b, :, 0].numpy(), d["grad_x"][b, :, 0].numpy()
        ln, mu = d["l_n"][b, :, 0].numpy() * 0.3, d["mu"][b, :, 0].numpy()
        sol = lambda PP, qq, ll, mm: oracle.solveQCQP(PP, qq, ll, mm, None, 1e-13, 1e-7, 100000)
        x = sol(P, q, ln, mu)
        E1, E2, blg, steps, gam = oracle.solveDerivativesQCQP(P, q, ln, mu, x, g, return_steps=True)
        r = ln * mu
        S = np.array([x[2 * i] ** 2 + x[2 * i + 1] ** 2 - r[i] ** 2 for i in range(nc)])
        act = [i for i in range(nc) if S[i] > -1e-10 and r[i] > 1e-10]
        na = len(act)
        A = np.zeros((n + na, n + na))
        for k, c in enumerate(act):
            A[k, k] = S[c]
            A[k, na + 2 * c: na + 2 * c + 2] = gam[c] * 2 * x[2 * c: 2 * c + 2]
            A[na + 2 * c: na + 2 * c + 2, k] = 2 * x[2 * c: 2 * c + 2]
        A[na:, na:] = P + np.diag(2 * np.repeat(gam, 2))
        rhs = np.concatenate([np.zeros(na), g])
        # (1) exact solve vs finite differences
        bex = np.linalg.solve(A.T, rhs)
        dgam_ex = np.zeros(nc)
        dgam_ex[act] = bex[:na]
        assert np.allclose(-bex[na:], _fd(lambda qq: g @ sol(P, qq, ln, mu), q, 1e-6), atol=2e-5, rtol=2e-3)
        assert np.allclose(np.diag(E2) * dgam_ex, _fd(lambda ll: g @ sol(P, q, ll, mu), ln, 1e-6), atol=2e-5, rtol=2e-3)
        assert np.allclose(np.diag(E1) * dgam_ex, _fd(lambda mm: g @ sol(P, q, ln, mm), mu, 1e-6), atol=2e-5, rtol=2e-3)
        # (2) the oracle is the iterated Tikhonov solve
        K = A @ A.T + 1e-7 * np.eye(n + na)
        xs = np.zeros(n + na)
        for _ in range(steps):
            xs = np.linalg.solve(K, 1e-7 * xs + A @ rhs)
        ref = np.zeros(nc + n)
        ref[act] = xs[:na]
        ref[nc:] = xs[na:]
        assert np.allclose(blg, ref, rtol=1e-6, atol=1e-12)
        assert np.allclose(np.diag(E1), 2 * gam * ln * ln * mu) and np.allclose(np.diag(E2), 2 * gam * ln * mu * mu)


# ---------------------------------------------------------------- box QP / signed box QP
def test_box_diag_closed_form(oracle):
    """Diagonal P: x* = clamp(-q/p, l_min, l_max); signed box additionally v o x <= 0 (Solver.cpp:396-398).

    Reference quirk (Solver.cpp:226): the loop stops on the DUAL residual rho*|l_2 - l_2_pred| alone, so when
    the over-relaxed iterate is clamped to the same bounds on every coordinate in two consecutive iterations it
    stops there (iteration 2) whatever the primal residual is.  Such returns have no interior coordinate; every
    other problem must match the closed form."""
    d = make_problem("sbox", 64, 8, 71)
    P, q = d["P"].numpy(), d["q"].numpy()
    lo, hi, v = d["l_min"].numpy(), d["l_max"].numpy(), d["v"].numpy()
    p = np.diagonal(P, axis1=1, axis2=2)[..., None]
    x, it = oracle.boxqp_fwd_batch(P, q, lo, hi, 1e-9, 10000)
    ref = np.clip(-q / p, lo, hi)
    interior = ((x > lo) & (x < hi)).any(axis=(1, 2))
    assert interior.mean() > 0.8 and it.max() < 10000
    assert np.abs(x - ref)[interior].max() < 1e-6
    early = ~interior & (np.abs(x - ref).max(axis=(1, 2)) > 1e-6)
    assert (it[early] <= 2).all()           # the quirk, and nothing else, explains a wrong return
    xs, its = oracle.boxqp_fwd_batch(P, q, lo, hi, 1e-9, 10000, v=v)
    sg = np.sign(v)
    refs = sg * np.minimum(sg * ref, 0.0)  # the feasible set is a box with one side moved to 0
    lo_s, hi_s = np.where(sg < 0, np.maximum(lo, 0.0), lo), np.where(sg > 0, np.minimum(hi, 0.0), hi)
    interior_s = ((xs > lo_s) & (xs < hi_s)).any(axis=(1, 2))
    assert np.abs(xs - refs)[interior_s].max() < 1e-6 and its.max() < 10000
    assert (sg * xs <= 0).all() and (xs >= lo).all() and (xs <= hi).all()


def test_box_matches_qp_when_bounds_are_zero_and_infinity(oracle):
    """l_min = 0, l_max = +huge reduces solveBoxQP to solveQP (same loop, Solver.cpp:198-261 vs :61-123)."""
    d = make_problem("qp", 16, 8, 72, "dense")
    P, q = d["P"].numpy(), d["q"].numpy()
    x0, it0 = oracle.qp_fwd_batch(P, q, 1e-7, 1000)
    x1, it1 = oracle.boxqp_fwd_batch(P, q, np.zeros_like(q), np.full_like(q, 1e300), 1e-7, 1000)
    assert np.array_equal(x0, x1) and np.array_equal(it0, it1)


def test_box_kkt_and_fd_gradients(oracle):
    """KKT of the recovered duals and finite differences of every input.  Settles the sign the reference
    leaves open (qcqp.py:93 vs Solver.cpp:837): grad_l_min = -dgamma_lo*gamma_lo, grad_l_max = +dgamma_hi*gamma_hi."""
    rng = np.random.default_rng(0)
    n = 6
    S = rng.random((n, n))
    P = S @ S.T / n + 0.1 * np.eye(n)
    q = rng.uniform(-1, 1, n)
    lo = -(rng.random(n) * 0.5 + 0.05)
    hi = rng.random(n) * 0.5 + 0.05
    g = rng.standard_normal(n)

    def sol(P=P, q=q, lo=lo, hi=hi):
        return oracle.solveBoxQP(P, q, lo, hi, np.zeros(n), 1e-12, 1e-7, 100000)

    x = sol()
    blg, gam, st = oracle.solveDerivativesBoxQP(P, q, lo, hi, x, g, return_steps=True)
    assert (gam >= -1e-9).all() and 0 < (gam > 1e-6).sum() < n
    assert np.abs(P @ x + q - gam[:n] + gam[n:]).max() < 1e-6
    dg, dl = blg[:2 * n], blg[2 * n:]
    h = 1e-6
    E = np.eye(n)
    fd = lambda f: np.array([g @ (f(+h * E[i]) - f(-h * E[i])) / (2 * h) for i in range(n)])
    assert np.allclose(-dl, fd(lambda e: sol(q=q + e)), atol=2e-5)
    assert np.allclose(-(dg[:n] * gam[:n]), fd(lambda e: sol(lo=lo + e)), atol=2e-5)
    assert np.allclose(+(dg[n:] * gam[n:]), fd(lambda e: sol(hi=hi + e)), atol=2e-5)
    gP = -np.outer(dl, x)
    for (i, j) in [(0, 0), (1, 4), (4, 1), (5, 5)]:
        D = np.zeros((n, n)); D[i, j] = D[j, i] = h  # LLT reads the lower triangle only: perturb symmetrically
        num = g @ (sol(P=P + D) - sol(P=P - D)) / (2 * h)
        ana = gP[i, j] + (gP[j, i] if i != j else 0.0)
        assert abs(num - ana) < 5e-5
    # batched assembly agrees with the single-problem composition
    out = oracle.boxqp_bwd_batch(P[None], q[None, :, None], lo[None, :, None], hi[None, :, None], x[None, :, None],
                                 g[None, :, None])
    assert np.array_equal(out[0][0], gP) and np.array_equal(out[1][0, :, 0], -dl)
    assert np.array_equal(out[2][0, :, 0], -(dg[:n] * gam[:n])) and np.array_equal(out[3][0, :, 0], dg[n:] * gam[n:])
    assert np.array_equal(out[4][0], gam) and out[5][0].tolist() == st.tolist()


def test_box_both_bounds_active(oracle):
    """l_min == l_max pins a coordinate: both multipliers enter the system (a 3x3 block per coordinate)."""
    d = make_problem("box", 8, 4, 73)
    P, q = d["P"].numpy(), d["q"].numpy()
    lo, hi = d["l_min"].numpy().copy(), d["l_max"].numpy().copy()
    hi[:, 1] = lo[:, 1]
    x, _ = oracle.boxqp_fwd_batch(P, q, lo, hi, 1e-9, 10000)
    assert np.abs(x[:, 1] - lo[:, 1]).max() < 1e-12
    out = oracle.boxqp_bwd_batch(P, q, lo, hi, x, d["grad_x"].numpy())
    assert all(np.isfinite(o).all() for o in out[:5])
    assert np.abs(out[1][:, 1]).max() < 1e-5  # a pinned coordinate does not move with q


def test_warm_start_is_dead(oracle):
    """Solver.cpp:70 then :80 -- the argument cannot change the result."""
    d = make_problem("qp", 1, 8, 41, "dense")
    P, q = d["P"][0].numpy(), d["q"][0].numpy()
    a = oracle.solveQP(P, q, np.zeros(8), 1e-8, 1e-7, 1000)
    b = oracle.solveQP(P, q, np.random.default_rng(0).normal(size=8), 1e-8, 1e-7, 1000)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("path", GENERIC_FIXTURES, ids=os.path.basename)
def test_oracle_reproduces_golden(oracle, path):
    """The committed fixtures are what the oracle computes (here and on the GPU box's host)."""
    d = np.load(path)
    eps, mi = float(d["eps"]), int(d["max_iter"])
    if "l_min" in d.files:  # box QP (with v: signed box QP, forward only)
        v = d["v"] if "v" in d.files else None
        x, it = oracle.boxqp_fwd_batch(d["P"], d["q"], d["l_min"], d["l_max"], eps, mi, v=v)
        assert np.array_equal(it, d["iters"]) and np.allclose(x, d["x"], rtol=0, atol=1e-11)
        if v is None:
            gP, gq, glo, ghi, gam, st = oracle.boxqp_bwd_batch(d["P"], d["q"], d["l_min"], d["l_max"], d["x"], d["grad_x"])
            assert np.array_equal(st, d["ir_steps"])
            for a, n in ((gP, "grad_P"), (gq, "grad_q"), (glo, "grad_l_min"), (ghi, "grad_l_max"), (gam, "gamma")):
                assert np.allclose(a, d[n], rtol=1e-9, atol=1e-12), n
        return
    if "l_n" in d.files:
        x, it = oracle.qcqp_fwd_batch(d["P"], d["q"], d["l_n"], d["mu"], eps, mi)
        gP, gq, gl, gm, st = oracle.qcqp_bwd_batch(d["P"], d["q"], d["l_n"], d["mu"], d["x"], d["grad_x"])
        assert np.allclose(gl, d["grad_l_n"], rtol=1e-9, atol=1e-12) and np.allclose(gm, d["grad_mu"], rtol=1e-9, atol=1e-12)
    else:
        x, it = oracle.qp_fwd_batch(d["P"], d["q"], eps, mi)
        gP, gq, st = oracle.qp_bwd_batch(d["P"], d["q"], d["x"], d["grad_x"])
    # libm pow() may differ by an ulp between hosts; everything else is IEEE-exact
    assert np.array_equal(it, d["iters"])
    assert np.allclose(x, d["x"], rtol=0, atol=1e-11)
    assert np.array_equal(st, d["ir_steps"])
    assert np.allclose(gP, d["grad_P"], rtol=1e-9, atol=1e-12) and np.allclose(gq, d["grad_q"], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "ref_*.npz")) +
                                        glob.glob(os.path.join(GOLDEN, "rd_*.npz"))), ids=os.path.basename)
def test_oracle_reproduces_reference_inputs(oracle, path):
    """ref_*.npz: the matrices the reference hard-codes in Solver::test() (Solver.cpp:697-923; inputs only -- the
    reference holds no expected values); rd_*.npz: seeded rank-deficient dense P.  Solutions reach 1.6e7, so the
    forward tolerance is relative to the solution's scale; the backward runs on the fixture's x (IEEE-exact)."""
    d = np.load(path)
    eps, mi = float(d["eps"]), int(d["max_iter"])
    if "l_n" in d.files:
        x, it = oracle.qcqp_fwd_batch(d["P"], d["q"], d["l_n"], d["mu"], eps, mi)
        gP, gq, gl, gm, st = oracle.qcqp_bwd_batch(d["P"], d["q"], d["l_n"], d["mu"], d["x"], d["grad_x"])
        assert np.allclose(gl, d["grad_l_n"], rtol=1e-9, atol=1e-12) and np.allclose(gm, d["grad_mu"], rtol=1e-9, atol=1e-12)
    else:
        x, it = oracle.qp_fwd_batch(d["P"], d["q"], eps, mi)
        gP, gq, st = oracle.qp_bwd_batch(d["P"], d["q"], d["x"], d["grad_x"])
    assert np.array_equal(it, d["iters"])
    assert np.abs(x - d["x"]).max() <= 1e-9 * max(1.0, np.abs(d["x"]).max())
    assert np.array_equal(st, d["ir_steps"])
    assert np.allclose(gP, d["grad_P"], rtol=1e-9, atol=1e-12) and np.allclose(gq, d["grad_q"], rtol=1e-9, atol=1e-12)


def test_conditioning_fixture_is_what_the_oracle_computes(oracle):
    """golden/conditioning/qp_ill_n8.npz (the reference's ill-conditioned QP workload, test_script.py:140-157) is regenerated
    here by make_golden.py's own recipe and compared bit for bit, NaN for NaN: inputs, x, iteration counts, refinement
    steps and gradients.  What the fixture records is the reference's behaviour on it: a third of the problems end in NaN
    (llt() of a shifted diagonal that lost positivity), the loop stops in the iteration after, a few hit max_iter."""
    import sys
    sys.path.insert(0, GOLDEN)
    d = np.load(os.path.join(GOLDEN, "conditioning", "qp_ill_n8.npz"))
    default = torch.get_default_dtype()
    try:
        import make_golden  # (sets float64 as torch's default dtype, as the generator runs)
        torch.set_default_dtype(torch.float64)
        new = make_golden.conditioning_cases()["qp_ill_n8"]
    finally:
        torch.set_default_dtype(default)
    assert sorted(new) == sorted(d.files)
    for k in d.files:
        assert np.array_equal(np.asarray(new[k]), d[k], equal_nan=True), k
    nan = np.isnan(d["x"]).any(axis=(1, 2))
    assert np.isnan(d["x"][nan]).all() and 15 <= nan.sum() <= 30          # NaN problems are all-NaN; 23 of 64
    assert (d["iters"][nan] < 20000).all() and (d["iters"] == 1000000).sum() >= 1
    assert np.isfinite(d["grad_q"]).all()                                    # grad_q does not depend on x's NaN
    assert np.isfinite(d["grad_P"][~nan]).all()


def test_reference_inputs_are_the_literals_and_behave_as_their_structure_says(oracle):
    """What can be said about the reference's own matrices without the reference: the literals have the structure
    SURVEY 8(c)(v) describes, and the oracle's answers satisfy the optimality conditions the structure implies."""
    import sys
    sys.path.insert(0, GOLDEN)
    import reference_inputs as R
    P, q, l_n = R.m2_singular()
    assert np.linalg.matrix_rank(P) == 2 and np.count_nonzero(P) == 2                  # singular
    x = oracle.solveQP(P, q, None, 1e-10, 1e-7, 1000)
    assert abs(x[0] - 8000 / 0.0005) <= 1e-6 * 1.6e7 and np.all(x[1:] == 0)            # -q0/p0 = 1.6e7; x >= 0
    x1 = oracle.solveQP(P, q, None, 1e-10, 1e-7, 1)                                     # Solver.cpp:729: one iteration
    assert 0 < x1[0] < x[0]
    xq = oracle.solveQCQP(P, q, l_n, np.ones(2), None, 1e-10, 1e-7, 1000)
    assert abs(np.hypot(xq[0], xq[1]) - 1e4) <= 1e-6 * 1e4                              # on the 1e4 friction disk
    P4, q4, l4 = R.g4_delassus()
    assert np.allclose(P4, P4.T) and np.linalg.matrix_rank(P4) == 3
    assert np.array_equal(P4[0], P4[4]) and np.array_equal(P4[1], P4[3]) and np.array_equal(P4[2], P4[6])
    assert np.array_equal(P4[5], P4[7])
    x4 = oracle.solveQCQP(P4, q4, l4, np.ones(4), None, 1e-10, 1e-7, 1000)
    assert np.all(np.hypot(x4[0::2], x4[1::2]) <= l4 * (1 + 1e-9))                      # feasible
    assert np.allclose(np.hypot(x4[0::2], x4[1::2]), l4, rtol=1e-6)                     # every contact slides
    P2, q2 = R.g2_product()
    assert np.allclose(P2, P2.T) and np.linalg.cond(P2) > 1e20
    Pb, qb, radii = R.g_blockdiag()
    xb = oracle.solveQCQP(Pb, qb, radii[0], np.ones(2), None, 1e-10, 1e-7, 100000)
    assert xb[2] == 0 and xb[3] == 0                                                    # the zero-radius contact
    assert abs(np.hypot(xb[0], xb[1]) - radii[0][0]) <= 1e-9


def test_oracle_openmp_matches_serial(oracle):
    d = make_problem("qcqp", 257, 8, 51)
    a = oracle.qcqp_fwd_batch(d["P"].numpy(), d["q"].numpy(), d["l_n"].numpy(), d["mu"].numpy(), 1e-7, 1000, nthreads=1)
    b = oracle.qcqp_fwd_batch(d["P"].numpy(), d["q"].numpy(), d["l_n"].numpy(), d["mu"].numpy(), 1e-7, 1000, nthreads=4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("kind", ["qp", "qcqp", "box", "sbox"])
def test_batch_functions_are_the_single_problem_functions_at_any_parameters(oracle, kind):
    """The batch API passes eps, mu_prox, max_iter, adaptive and the backward's epsilon through: each batch call equals, bit
    for bit, a loop over the single-problem function of the reference's pybind11 signature (iterations, refinement steps,
    and the duals gamma / dgamma of the QCQP and box backward included)."""
    from param_cases import nudge
    from tools import oracle_params
    B, N = 24, 8
    d = {k: v.numpy() for k, v in make_problem(kind, B, N, 5600 + len(kind), "mixed").items()}
    P, q, g = d["P"], d["q"], d["grad_x"]
    for eps, mu_prox, max_iter, adaptive in ((1e-7, 1e-10, 1000, True), (1e-5, 1e-3, 300, False), (1e-10, 1e-2, 4000, True),
                                             (1e-7, 1e-7, 0, False), (1e-7, 1e-5, 1, True)):
        if kind == "qp":
            x, it = oracle.qp_fwd_batch(P, q, eps, max_iter, mu_prox=mu_prox, adaptive=adaptive)
            one = [oracle.solveQP(P[b], q[b], None, eps, mu_prox, max_iter, adaptive, return_iters=True) for b in range(B)]
        elif kind == "qcqp":
            x, it = oracle.qcqp_fwd_batch(P, q, d["l_n"], d["mu"], eps, max_iter, mu_prox=mu_prox, adaptive=adaptive)
            one = [oracle.solveQCQP(P[b], q[b], d["l_n"][b], d["mu"][b], None, eps, mu_prox, max_iter, adaptive,
                                    return_iters=True) for b in range(B)]
        elif kind == "box":
            x, it = oracle.boxqp_fwd_batch(P, q, d["l_min"], d["l_max"], eps, max_iter, mu_prox=mu_prox, adaptive=adaptive)
            one = [oracle.solveBoxQP(P[b], q[b], d["l_min"][b], d["l_max"][b], None, eps, mu_prox, max_iter, adaptive,
                                     return_iters=True) for b in range(B)]
        else:
            x, it = oracle.boxqp_fwd_batch(P, q, d["l_min"], d["l_max"], eps, max_iter, v=d["v"], mu_prox=mu_prox,
                                           adaptive=adaptive)
            one = [oracle.solveSignedBoxQP(P[b], q[b], d["l_min"][b], d["l_max"][b], d["v"][b], None, eps, mu_prox, max_iter,
                                           adaptive, return_iters=True) for b in range(B)]
        assert np.array_equal(x[:, :, 0], np.stack([o[0] for o in one])) and np.array_equal(it, [o[1] for o in one])
        xp, itp = oracle_params.fwd(oracle, kind, d, eps, max_iter, mu_prox, adaptive)   # what the fuzzers use
        assert np.array_equal(xp, x) and np.array_equal(itp, it)
        if max_iter == 0:
            assert (x == 0).all() and (it == 0).all()
    if kind == "sbox":
        return
    x = nudge(kind, d, x, 3)
    for epsilon in (1e-10, 1e-6, 1e-4, 1e-2):
        fuzz_ref = oracle_params.bwd(oracle, kind, d, x, epsilon)
        batch = {"qp": lambda: oracle.qp_bwd_batch(P, q, x, g, epsilon=epsilon),
                 "qcqp": lambda: oracle.qcqp_bwd_batch(P, q, d["l_n"], d["mu"], x, g, epsilon=epsilon),
                 "box": lambda: oracle.boxqp_bwd_batch(P, q, d["l_min"], d["l_max"], x, g, epsilon=epsilon)}[kind]()
        assert len(fuzz_ref) == len(batch) and all(np.array_equal(a, b) for a, b in zip(fuzz_ref, batch))
        if kind == "qp":
            gP, gq, st = oracle.qp_bwd_batch(P, q, x, g, epsilon=epsilon)
            for b in range(B):
                bl, s = oracle.solveDerivativesQP(P[b], q[b], x[b], g[b], epsilon, return_steps=True)
                assert np.array_equal(gq[b, :, 0], -bl) and st[b] == s
                assert np.array_equal(gP[b], -(bl[:, None] * x[b, :, 0][None, :]))
        elif kind == "qcqp":
            gP, gq, gl, gm, st, gam, dgam = oracle.qcqp_bwd_batch(P, q, d["l_n"], d["mu"], x, g, epsilon=epsilon,
                                                                  duals=True)
            assert all(np.array_equal(a, b) for a, b in zip(oracle.qcqp_bwd_batch(P, q, d["l_n"], d["mu"], x, g,
                                                                                  epsilon=epsilon), (gP, gq, gl, gm, st)))
            for b in range(B):
                E1, E2, blg, s, gm1 = oracle.solveDerivativesQCQP(P[b], q[b], d["l_n"][b], d["mu"][b], x[b], g[b], epsilon,
                                                                  return_steps=True)
                nc = N // 2
                assert np.array_equal(gq[b, :, 0], -blg[nc:]) and st[b] == s
                assert np.array_equal(gam[b, :, 0], gm1) and np.array_equal(dgam[b, :, 0], blg[:nc])
                assert np.array_equal(gl[b, :, 0], np.diag(E2) * blg[:nc]) and np.array_equal(gm[b, :, 0], np.diag(E1) * blg[:nc])
        else:
            gP, gq, glo, ghi, gam, st, dgam = oracle.boxqp_bwd_batch(P, q, d["l_min"], d["l_max"], x, g, epsilon=epsilon,
                                                                     duals=True)
            for b in range(B):
                blg, gm1, s = oracle.solveDerivativesBoxQP(P[b], q[b], d["l_min"][b], d["l_max"][b], x[b], g[b], epsilon,
                                                           return_steps=True)
                assert np.array_equal(gq[b, :, 0], -blg[2 * N:]) and np.array_equal(st[b], s)
                assert np.array_equal(gam[b], gm1) and np.array_equal(dgam[b], blg[:2 * N])
                assert np.array_equal(glo[b, :, 0], -(blg[:N] * gm1[:N])) and np.array_equal(ghi[b, :, 0], blg[N:2 * N] * gm1[N:])


def test_iteration_statistics_match_the_survey_sessions_independent_restatement(oracle):
    """SURVEY.md Appendix C lists statistics from a SECOND restatement of the reference -- a throwaway numpy script written by
    the survey session from its own reading of Solver.cpp, before this oracle existed (never product, never committed).  Its
    numbers are the only figures about this algorithm in the repository that did not come out of this oracle or the kernels
    checked against it, so they are worth a test: iteration counts depend on every detail of the loop (under-estimated
    power iteration, rho schedule, cpt logic, one- vs two-sided stop).  Different seeds, so the comparison is statistical:
    means within 3-4 standard errors of both samples, maxima of the same order."""
    import torch
    g = torch.Generator().manual_seed(20260930)
    U = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)

    def its_qp(P, q):
        return oracle.qp_fwd_batch(P.numpy(), q.numpy(), 1e-7, 1000, nthreads=8)

    # README verbatim (q >= 0): one iteration, x = 0
    P, q = torch.diag_embed(U(200, 8)), U(200, 8, 1)
    x, it = its_qp(P, q)
    assert (it == 1).all() and not x.any()
    # QP diag N = 8, p ~ U(.1, 1.1): survey 18.3 mean / p99 25 / max 31 (400 problems)
    n = 2000
    p, q = U(n, 8) + 0.1, 2 * U(n, 8, 1) - 1
    x, it = its_qp(torch.diag_embed(p), q)
    assert abs(it.mean() - 18.3) < 0.8 and 23 <= np.percentile(it, 99) <= 28 and 28 <= it.max() <= 40
    err = np.abs(x[:, :, 0] - np.maximum(-q[:, :, 0].numpy() / p.numpy(), 0)).max(axis=1)
    assert 0.5e-7 < np.median(err) < 6e-7                      # survey: median 1.7e-7
    # ... p ~ U(0, 1): survey 23.6 mean / median 21 / p90 34 / p99 64 / max 173 (heavy tail)
    p0 = U(n, 8)
    x, it0 = its_qp(torch.diag_embed(p0), q)
    # (the survey's p90 of 34 is one 400-problem sample: subsets of that size give 33 .. 44 here)
    assert abs(it0.mean() - 23.6) < 1.5 and abs(np.median(it0) - 21) <= 1 and 32 <= np.percentile(it0, 90) <= 44
    assert 55 <= np.percentile(it0, 99) <= 75 and it0.max() > 100          # survey: p99 64, max 173
    # QP diag N = 32, p ~ U(.1, 1.1): survey mean 21.6, max 25;  p ~ U(0, 1): mean 37.8
    x, it = its_qp(torch.diag_embed(U(400, 32) + 0.1), 2 * U(400, 32, 1) - 1)
    assert abs(it.mean() - 21.6) < 0.8 and it.max() <= 30
    x, it = its_qp(torch.diag_embed(U(400, 32)), 2 * U(400, 32, 1) - 1)
    assert abs(it.mean() - 37.8) < 3.0
    # QCQP diag N = 8, p ~ U(.1, 1.1), r = U * U: survey 17.6 mean / p99 27 / max 33
    p, q = U(n, 8) + 0.1, 2 * U(n, 8, 1) - 1
    ln, mu = U(n, 4, 1), U(n, 4, 1)
    x, it = oracle.qcqp_fwd_batch(torch.diag_embed(p).numpy(), q.numpy(), ln.numpy(), mu.numpy(), 1e-7, 1000, nthreads=8)
    assert abs(it.mean() - 17.6) < 0.8 and 24 <= np.percentile(it, 99) <= 31 and it.max() <= 45
    # ... its backward: the refinement loop leaves after 1 body on about half of the problems and after 3 on the rest (141 / 159)
    gx = torch.randn(n, 8, 1, generator=g, dtype=torch.float64)
    st = oracle.qcqp_bwd_batch(torch.diag_embed(p).numpy(), q.numpy(), ln.numpy(), mu.numpy(), x, gx.numpy(), nthreads=8)[-1]
    assert set(np.unique(st)) <= {1, 3} and 0.35 < (st == 1).mean() < 0.6
    # QP backward: always one body
    xq, _ = its_qp(torch.diag_embed(p), q)
    assert (oracle.qp_bwd_batch(torch.diag_embed(p).numpy(), q.numpy(), xq, gx.numpy(), nthreads=8)[-1] == 1).all()
    # dense P = S S^T / N + 0.1 I: N = 32 survey mean 63 (max 75); N = 64 mean 91 (p99 131, max 136)
    for N, mean, tol, mx in ((32, 63, 4.0, 95), (64, 91, 5.0, 170)):
        S = U(200, N, N)
        P = torch.bmm(S, S.transpose(1, 2)) / N + 0.1 * torch.eye(N, dtype=torch.float64)
        x, it = its_qp(P, 2 * U(200, N, 1) - 1)
        assert abs(it.mean() - mean) < tol and it.max() <= mx, (N, it.mean(), it.max())
    assert it.max() < 1000                                       # "no max_iter hits in any probe"
