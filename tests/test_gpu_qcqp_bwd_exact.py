"""The diagonal QCQP backward (csrc/bwd_diag.hip, kkt_core.h: QcqpContact) against the oracle's backward on identical x, bit for
bit -- grad_P, grad_q, grad_l_n, grad_mu, gamma, dgamma and ir_steps -- at the smallest shapes at which its addressing and its
per-contact KKT blocks can go wrong:
  * N = 8 (16 problems per wave tile, 12 residual entries per problem) and N = 2 (64 per tile, one contact per problem, an odd
    residual row of 3);
  * 1, T - 1, T, T + 1 and 4 T + 3 problems (T = 128 / N): a partial tile, exactly one, one and a problem, a partial workgroup;
  * routes: DQQ_P_DIAG, DQQ_P_AUTO, and DQQ_P_AUTO with the forward's pdiag / flags hand-off;
  * active and inactive contacts inside one problem (x is the oracle's forward solution; l_n is scaled so that about half of
    the contacts end on the cone's boundary), and refinement loops of different lengths inside one tile -- both asserted."""
import numpy as np
import pytest
import torch

from conftest import make_problem
from test_gpu_parity import dev, npy, ops, oracle_bwd, oracle_fwd  # noqa: F401  (ops: fixture)

pytestmark = pytest.mark.gpu

P_AUTO, P_DIAG = 0, 2   # diffqcqp_amd._capi
_cache = {}


def case(oracle, N, B):
    """Problem, the oracle's x and the oracle's backward on it: computed once per shape, shared by the routes."""
    if (N, B) not in _cache:
        d = make_problem("qcqp", B, N, seed=1000 * N + B)
        # cone radius l_n mu ~ 6 U(0,1)^2 against |unconstrained minimiser| ~ |q| / p ~ 1: about half of the contacts active
        d["l_n"] = 6.0 * d["l_n"]
        xo, _ = oracle_fwd(oracle, "qcqp", d)
        ref = oracle.qcqp_bwd_batch(d["P"].numpy(), d["q"].numpy(), d["l_n"].numpy(), d["mu"].numpy(), xo, d["grad_x"].numpy(),
                                    nthreads=8, duals=True)
        r = (d["l_n"] * d["mu"]).numpy().reshape(B, N // 2)
        S = (xo.reshape(B, N // 2, 2) ** 2).sum(-1) - r * r
        act = (S > -1e-10) & (r > 1e-10)                               # Solver.cpp:637-641
        _cache[(N, B)] = (d, xo, ref, act)
    return _cache[(N, B)]


def sizes(N):
    T = 128 // N
    return [1, T - 1, T, T + 1, 4 * T + 3]


CASES = [(N, B) for N in (8, 2) for B in sizes(N)]


@pytest.mark.parametrize("route", ["diag", "auto", "auto_handoff"])
@pytest.mark.parametrize("N, B", CASES)
def test_qcqp_diag_backward_is_bit_exact(oracle, ops, N, B, route):
    d, xo, ref, act = case(oracle, N, B)
    gP, gq, gl, gm, steps, gam, dgam = ref
    g = dev(d)
    x = torch.from_numpy(xo).cuda()
    duals = (torch.full((B, N // 2, 1), 7.0, dtype=torch.float64, device="cuda"), torch.full((B, N // 2, 1), 7.0, dtype=torch.float64, device="cuda"))
    kw = {}
    P, layout = g["P"], P_AUTO
    if route == "diag":
        P, layout = torch.diagonal(g["P"], dim1=1, dim2=2).contiguous(), P_DIAG
    elif route == "auto_handoff":
        kw["cache"] = ops.diag_cache(g["q"])
        ops.qcqp_forward(g["P"], g["q"], g["l_n"], g["mu"], 1e-7, 1000, cache=kw["cache"])
    hP, hq, hl, hm, hs = ops.qcqp_backward(P, g["q"], g["l_n"], g["mu"], x, g["grad_x"], layout=layout, return_steps=True,
                                           duals=duals, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(npy(hs), steps), "refinement step counts differ"
    want_P = np.diagonal(gP, axis1=1, axis2=2) if route == "diag" else gP
    for name, a, b in (("grad_P", hP, want_P), ("grad_q", hq, gq), ("grad_l_n", hl, gl), ("grad_mu", hm, gm),
                       ("gamma", duals[0], gam), ("dgamma", duals[1], dgam)):
        a = npy(a)
        assert a.shape == b.shape, (name, a.shape, b.shape)
        assert np.array_equal(a, b), "%s: max diff %g" % (name, np.abs(a - b).max())


@pytest.mark.parametrize("N", [8, 2])
def test_the_batches_hold_what_they_are_meant_to(oracle, N):
    T = 128 // N
    d, xo, ref, act = case(oracle, N, 4 * T + 3)
    share = act.mean()
    assert 0.25 < share < 0.75, "about half of the contacts should be active: %.2f" % share
    if N > 2:
        mixed = (act.any(1) & ~act.all(1)).mean()
        assert mixed > 0.25, "active and inactive contacts in one problem: only %.2f of the problems" % mixed
    # refinement loops of different lengths inside one wave tile, in neighbouring problems
    steps = ref[4]
    tiles = [steps[i:i + T] for i in range(0, len(steps), T)]
    assert any(len(np.unique(t)) > 1 for t in tiles), steps
    assert np.any(steps[:-1] != steps[1:])
    assert steps.min() >= 1 and steps.max() >= 3, (steps.min(), steps.max())
