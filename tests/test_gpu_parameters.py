"""Every kernel route with the solver parameters a caller can set moved off their defaults (run with -m gpu on an MI355X).

Each route family keeps its own copy of the code that reads mu_prox (initial rho, tau, the shifted diagonal, q - mu_prox l),
eps, max_iter and adaptive_rho; the backward's dual-recovery threshold epsilon is read by csrc/bwd_systems.h for every family
(written out only in dense_wave64.hip and kkt_core.h: QcqpContact::setup).  The rows of tests/param_cases.py name the
route each call takes (checked against route.cpp on the CPU by tests/test_param_cases.py); here every row is run on the
shipped build against the oracle at the same arguments, with the bar its family has at default parameters
(tests/test_gpu_parity.py):
  forward    mu_prox in {1e-10, 1e-5, 1e-2}, eps in {1e-10, 1e-5}: check_forward, min_match 0.999 (fast and N <= 16
             routes), 0.97 (fwave64), 0.9 (N = 64), 0.99 (the reference-order and global-memory kernels beyond N = 16);
             max_iter = 1: identical counts, |dx| <= 1e-9;  max_iter = 0: x = 0 and no iteration, as the reference;
             adaptive_rho = False, max_iter 4000: |dx| <= 1e-6, >= 0.9 equal counts, |dit| <= 2;
  backward   on nudged x (param_cases.nudge) at epsilon in {1e-10, 1e-6, 1e-4}: bit-exact (bdiag), 1e-9 with equal
             refinement steps (bsmall, blane, bteam, bany), REASSOC_TOL (bchol, bqcqp, bqcqpbig); the duals of the QCQP
             and box backward as the gradients they feed; every single-output request bit-identical to the full call.
Each parameter point also asserts that its inputs can tell a kernel that ignores the parameter from one that uses it
(iteration counts / gradients change against the default on a given share of the problems)."""
import numpy as np
import pytest
import torch

from conftest import make_problem
from param_cases import BWD, DIAG, FWD, nudge, row_id, row_problem, tile
from test_gpu_parity import REASSOC_TOL, X_TOL, check_backward_exact, check_backward_reassociated, check_forward, npy

pytestmark = pytest.mark.gpu
MU_PROX = (1e-10, 1e-5, 1e-2)
EPS = (1e-10, 1e-5)
EPSILON = (1e-10, 1e-6, 1e-4)
EPSILON_SHARE = {1e-6: 0.4, 1e-4: 0.6}   # least share of problems whose oracle gradients move off epsilon = 1e-10
REASSOCIATING = ("bchol", "bqcqp", "bqcqpbig")


@pytest.fixture(scope="module")
def ops():
    """The shipped library, the hint feedback off: the route of a call is then a function of its arguments alone."""
    assert torch.cuda.is_available(), "these tests need the GPU"
    from diffqcqp_amd import build, ops as _ops, _capi
    build.build()
    _capi.lib()
    was_on = _capi._feedback is not None
    _capi.enable_feedback(False)
    yield _ops
    _capi.enable_feedback(was_on)


def _dev(d, layout):
    g = {k: v.cuda() for k, v in d.items()}
    if (layout & 0xff) == DIAG:
        g["P"] = torch.diagonal(g["P"], dim1=1, dim2=2).contiguous()
    return g


def _ofwd(O, kind, d, eps, max_iter, mu_prox=1e-7, adaptive=True):
    a = {k: v.numpy() for k, v in d.items()}
    kw = dict(mu_prox=mu_prox, nthreads=8, adaptive=adaptive)
    if kind == "qp":
        return O.qp_fwd_batch(a["P"], a["q"], eps, max_iter, **kw)
    if kind == "qcqp":
        return O.qcqp_fwd_batch(a["P"], a["q"], a["l_n"], a["mu"], eps, max_iter, **kw)
    return O.boxqp_fwd_batch(a["P"], a["q"], a["l_min"], a["l_max"], eps, max_iter, v=a.get("v"), **kw)


def _hfwd(ops, kind, g, layout, eps, max_iter, mu_prox=1e-7, adaptive=True):
    kw = dict(mu_prox=mu_prox, adaptive_rho=adaptive, layout=layout, return_iters=True)
    if kind == "qp":
        return ops.qp_forward(g["P"], g["q"], eps, max_iter, **kw)
    if kind == "qcqp":
        return ops.qcqp_forward(g["P"], g["q"], g["l_n"], g["mu"], eps, max_iter, **kw)
    return ops.boxqp_forward(g["P"], g["q"], g["l_min"], g["l_max"], eps, max_iter, v=g.get("v"), **kw)


def _min_match(N, route):
    if N == 64:
        return 0.9
    if "fwave64" in route:
        return 0.97
    return 0.999 if N <= 16 else 0.99


@pytest.mark.parametrize("row", FWD, ids=row_id)
def test_forward_parameters(oracle, ops, row):
    _, kind, N, B, layout, _, route = row
    base, full = row_problem(row, make_problem)
    g = _dev(full, layout)
    nb = base["q"].shape[0]
    _, it_default = _ofwd(oracle, kind, base, 1e-7, 1000)
    lam = np.linalg.eigvalsh(base["P"].numpy()).max(axis=1)
    for mu_prox in MU_PROX:
        xo, ito = _ofwd(oracle, kind, base, 1e-7, 1000, mu_prox)
        # the point's own conditions: tau > 1, the oracle converges, and mu_prox changes its trajectories
        assert (lam >= 10 * mu_prox).all()
        assert (np.isfinite(xo).all(axis=(1, 2)) & (ito < 1000)).mean() >= 0.99
        moved = (ito != it_default).mean()
        print("%s mu_prox %g: iteration counts differ from mu_prox = 1e-7 on %.3f" % (row_id(row), mu_prox, moved))
        assert moved >= 0.5 if nb >= 100 else moved > 0
        xh, ith = _hfwd(ops, kind, g, layout, 1e-7, 1000, mu_prox)
        check_forward(xh, ith, tile(xo, B), tile(ito, B), min_match=_min_match(N, route))
    for eps in EPS:
        xo, ito = _ofwd(oracle, kind, base, eps, 1000)
        xh, ith = _hfwd(ops, kind, g, layout, eps, 1000)
        check_forward(xh, ith, tile(xo, B), tile(ito, B), min_match=_min_match(N, route))
    xo, ito = _ofwd(oracle, kind, base, 1e-7, 1)
    xh, ith = _hfwd(ops, kind, g, layout, 1e-7, 1)
    assert np.array_equal(npy(ith), tile(ito, B)) and np.abs(npy(xh) - tile(xo, B)).max() <= 1e-9
    xo, ito = _ofwd(oracle, kind, base, 1e-7, 0)
    assert (xo == 0).all() and (ito == 0).all()
    xh, ith = _hfwd(ops, kind, g, layout, 1e-7, 0)
    assert (npy(xh) == 0).all() and (npy(ith) == 0).all()
    xo, ito = _ofwd(oracle, kind, base, 1e-7, 4000, adaptive=False)
    xh, ith = _hfwd(ops, kind, g, layout, 1e-7, 4000, adaptive=False)
    xo, ito = tile(xo, B), tile(ito, B)
    assert np.abs(npy(xh) - xo).max() <= X_TOL
    assert (npy(ith) == ito).mean() >= 0.9 and np.abs(npy(ith) - ito).max() <= 2


# ---------------------------------------------------------------- backward
def _obwd(O, kind, d, x, epsilon):
    """-> (grads, steps, duals) of the oracle; duals = (gamma, dgamma) in the C ABI's layout, None for the QP."""
    a = {k: v.numpy() for k, v in d.items()}
    if kind == "qp":
        gP, gq, st = O.qp_bwd_batch(a["P"], a["q"], x, a["grad_x"], nthreads=8, epsilon=epsilon)
        return [gP, gq], st, None
    if kind == "qcqp":
        gP, gq, gl, gm, st, gam, dgam = O.qcqp_bwd_batch(a["P"], a["q"], a["l_n"], a["mu"], x, a["grad_x"], nthreads=8,
                                                          epsilon=epsilon, duals=True)
        return [gP, gq, gl, gm], st, (gam, dgam)
    gP, gq, glo, ghi, gam, st, dgam = O.boxqp_bwd_batch(a["P"], a["q"], a["l_min"], a["l_max"], x, a["grad_x"], nthreads=8,
                                                        epsilon=epsilon, duals=True)
    return [gP, gq, glo, ghi], st, (gam, dgam)


def _hbwd(ops, kind, g, x, layout, epsilon, need=None, duals=True):
    B, N = g["q"].shape[0], g["q"].shape[1]
    if kind == "qp":
        need = need or (True, True)
        gP, gq, st = ops.qp_backward(g["P"], g["q"], x, g["grad_x"], need[0], need[1], layout=layout, return_steps=True,
                                     epsilon=epsilon)
        return [gP, gq], st, None
    shape = (B, N // 2, 1) if kind == "qcqp" else (B, 2 * N)
    du = (torch.empty(shape, dtype=torch.float64, device="cuda"), torch.empty(shape, dtype=torch.float64, device="cuda")) \
        if duals else None
    fn = ops.qcqp_backward if kind == "qcqp" else ops.boxqp_backward
    aux = (g["l_n"], g["mu"]) if kind == "qcqp" else (g["l_min"], g["l_max"])
    out = fn(g["P"], g["q"], *aux, x, g["grad_x"], need=need or (True, True, True, True), layout=layout, return_steps=True,
             epsilon=epsilon, duals=du)
    return list(out[:4]), out[4], du


def _moved(ref, ref0):
    """Per problem: does any gradient but grad_P differ from the epsilon = 1e-10 one by more than 1e-6 relative?"""
    out = np.zeros(ref[1].shape[0], dtype=bool)
    for a, b in zip(ref[1:], ref0[1:]):
        a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
        out |= ~(np.abs(a - b).max(axis=1) <= 1e-6 * np.maximum(1.0, np.abs(b).max(axis=1)))
    return out


def _families(route):
    """(family of the diagonal problems, family of the others) of a backward route."""
    first = route.split(" ")[0].split("/")[0]
    if route.startswith("bdiag + "):
        return "bdiag", route.split(" + ")[1].split(" ")[0].split("/")[0]
    return first, first


def _check_rows(oracle, kind, d, x, grads, steps, duals, ref, family, sel, epsilon, min_same=0.9):
    """The bar of `family` on the problems `sel` (numpy bool mask).  min_same: the least share of equal refinement exits of a
    matrix-core kernel (check_backward_reassociated's default; tests/test_gpu_footprint.py passes 0 for its tiny batches)."""
    if not sel.any():
        return
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[sel]))
    rg, rst, rdu = ref
    if family in REASSOCIATING:
        dsel = {k: v[torch.from_numpy(sel)] for k, v in d.items()}
        check_backward_reassociated(oracle, kind, dsel, x[sel], [t(a) for a in grads], t(steps), tuple(r[sel] for r in rg) +
                                    (rst[sel],), min_same=min_same, epsilon=epsilon)
        if duals is not None:
            same = steps[sel] == rst[sel]
            tol = REASSOC_TOL[kind][2]

            def rel(a, b):
                if not b.size:
                    return 0.0
                scale = np.maximum(1.0, np.abs(b).reshape(b.shape[0], -1).max(1)).reshape((-1,) + (1,) * (b.ndim - 1))
                return float((np.abs(a - b) / scale).max())
            for a, b in zip(duals, rdu):
                assert np.isfinite(a[sel]).all() and rel(a[sel][same], b[sel][same]) <= tol
            # where the exit differs: the oracle forced to the kernel's step count, as check_backward_reassociated does
            for st in np.unique(steps[sel][~same]):
                idx = np.nonzero(sel)[0][(~same) & (steps[sel] == st)]
                oracle.set_force_ir_steps(int(st))
                try:
                    forced = _obwd(oracle, kind, {k: v[torch.from_numpy(idx)] for k, v in d.items()}, x[idx], epsilon)[2]
                finally:
                    oracle.set_force_ir_steps(0)
                for a, b in zip(duals, forced):
                    assert rel(a[idx], b) <= 10 * tol
        return
    exact = family == "bdiag"
    check_backward_exact([t(a) for a in grads], t(steps), tuple(r[sel] for r in rg) + (rst[sel],), exact=exact)
    if duals is not None:
        for a, b in zip(duals, rdu):
            if exact:
                assert np.array_equal(a[sel], b[sel])
            else:
                assert np.allclose(a[sel], b[sel], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("row", BWD, ids=row_id)
def test_backward_parameters(oracle, ops, row):
    _, kind, N, B, layout, _, route = row
    base, full = row_problem(row, make_problem)
    nb = base["q"].shape[0]
    xb = nudge(kind, {k: v.numpy() for k, v in base.items()}, _ofwd(oracle, kind, base, 1e-7, 1000)[0], 7 + N)
    x = tile(xb, B)
    g = _dev(full, layout)
    xs = torch.from_numpy(x).cuda()
    Pb = base["P"].numpy()
    diag_b = (Pb == Pb * np.eye(N)).all(axis=(1, 2))
    diag = tile(diag_b, B)
    fam_diag, fam_other = _families(route)
    ref0 = None
    for epsilon in EPSILON:
        rb = _obwd(oracle, kind, base, xb, epsilon)
        if ref0 is None:
            ref0 = rb
        else:
            moved = _moved(rb[0], ref0[0]).mean()
            print("%s epsilon %g: gradients move off epsilon = 1e-10 on %.3f" % (row_id(row), epsilon, moved))
            assert moved >= EPSILON_SHARE[epsilon] if nb >= 64 else moved > 0
        ref = ([tile(a, B) for a in rb[0]], tile(rb[1], B), None if rb[2] is None else tuple(tile(a, B) for a in rb[2]))
        grads, st, du = _hbwd(ops, kind, g, xs, layout, epsilon)
        grads = [npy(a) for a in grads]
        st = npy(st)
        du = None if du is None else tuple(npy(a) for a in du)
        if (layout & 0xff) == DIAG:   # grad_P comes back as its diagonal
            ref = ([np.ascontiguousarray(np.diagonal(ref[0][0], axis1=1, axis2=2))] + ref[0][1:],) + ref[1:]
        _check_rows(oracle, kind, full, x, grads, st, du, ref, fam_diag, diag, epsilon)
        _check_rows(oracle, kind, full, x, grads, st, du, ref, fam_other, ~diag, epsilon)
        if epsilon == 1e-6:   # partial requests: each output alone is the full call's, the others stay None
            nout = 2 if kind == "qp" else 4
            for i in range(nout):
                need = tuple(j == i for j in range(nout))
                part, pst, _ = _hbwd(ops, kind, g, xs, layout, epsilon, need=need, duals=False)
                assert all(p is None for j, p in enumerate(part) if j != i)
                assert np.array_equal(npy(part[i]), grads[i]) and np.array_equal(npy(pst), st), (row_id(row), i)


# ---------------------------------------------------------------- the Python layer passes the parameters through
@pytest.mark.parametrize("kind", ["qp", "qcqp", "box"])
def test_autograd_functions_pass_mu_prox(ops, kind):
    """QPFn2 / QCQPFn2 / BoxQPFn2.apply(..., mu_prox) (the reference's sixth / eighth argument, qcqp.py:24, 144): forward x
    and gradients are the ops calls' at that mu_prox on the same route, bit for bit."""
    from diffqcqp_amd.qcqp import BoxQPFn2, QCQPFn2, QPFn2
    d = make_problem(kind, 300, 8, 9300 + len(kind), "mixed")
    names = {"qp": ("P", "q"), "qcqp": ("P", "q", "l_n", "mu"), "box": ("P", "q", "l_min", "l_max")}[kind]
    gd = {k: v.cuda() for k, v in d.items()}
    x_default = None
    for mu_prox in (1e-7, 1e-5, 1e-2):
        t = [gd[n].clone().requires_grad_(True) for n in names]
        ws = torch.zeros_like(gd["q"])
        if kind == "qp":
            x = QPFn2.apply(*t, ws, 1e-7, 1000, mu_prox)
            xr = ops.qp_forward(gd["P"], gd["q"], 1e-7, 1000, mu_prox=mu_prox)
        elif kind == "qcqp":
            x = QCQPFn2.apply(*t, ws, 1e-7, 1000, mu_prox)
            xr = ops.qcqp_forward(gd["P"], gd["q"], gd["l_n"], gd["mu"], 1e-7, 1000, mu_prox=mu_prox)
        else:
            x = BoxQPFn2.apply(*t, ws, 1e-7, 1000, mu_prox)
            xr = ops.boxqp_forward(gd["P"], gd["q"], gd["l_min"], gd["l_max"], 1e-7, 1000, mu_prox=mu_prox)
        assert torch.equal(x.detach(), xr)
        if x_default is None:
            x_default = xr
        else:
            assert not torch.equal(xr, x_default)
        (x * gd["grad_x"]).sum().backward()
        if kind == "qp":
            ref = ops.qp_backward(gd["P"], gd["q"], xr, gd["grad_x"])
        elif kind == "qcqp":
            ref = ops.qcqp_backward(gd["P"], gd["q"], gd["l_n"], gd["mu"], xr, gd["grad_x"])
        else:
            ref = ops.boxqp_backward(gd["P"], gd["q"], gd["l_min"], gd["l_max"], xr, gd["grad_x"])
        for a, r in zip(t, ref):
            assert torch.equal(a.grad, r)


def test_module_level_api_passes_mu_prox_and_epsilon(oracle, ops):
    """diffqcqp.solveQP / solveQCQP / solveBoxQP(mu_prox=...) and solveDerivatives*(epsilon=...) against the oracle's twins
    (same bars as tests/test_gpu_parity.py:test_unbatched_twins_and_module_level_api), diagonal and dense P, nudged x."""
    from diffqcqp_amd import diffqcqp as M
    for structure in ("diag", "dense"):
        for kind in ("qp", "qcqp", "box"):
            d = {k: v.numpy() for k, v in make_problem(kind, 3, 8, 9400 + len(kind), structure).items()}
            for b in range(3):
                P, q, g = d["P"][b], d["q"][b], d["grad_x"][b, :, 0]
                for mu_prox in (1e-5, 1e-2):
                    if kind == "qp":
                        x, xo = (f(P, q, None, 1e-7, mu_prox, 1000, True) for f in (M.solveQP, oracle.solveQP))
                    elif kind == "qcqp":
                        x, xo = (f(P, q, d["l_n"][b], d["mu"][b], None, 1e-7, mu_prox, 1000, True)
                                 for f in (M.solveQCQP, oracle.solveQCQP))
                    else:
                        x, xo = (f(P, q, d["l_min"][b], d["l_max"][b], None, 1e-7, mu_prox, 1000, True)
                                 for f in (M.solveBoxQP, oracle.solveBoxQP))
                    assert np.abs(x - xo).max() < 1e-9
                xn = nudge(kind, {k: v[b:b + 1] for k, v in d.items()}, xo.reshape(1, 8, 1), 9500 + b)[0, :, 0]
                for epsilon in (1e-6, 1e-4):
                    if kind == "qp":
                        out = [M.solveDerivativesQP(P, q, xn, g, epsilon=epsilon)]
                        ref = [oracle.solveDerivativesQP(P, q, xn, g, epsilon)]
                    elif kind == "qcqp":
                        out = M.solveDerivativesQCQP(P, q, d["l_n"][b], d["mu"][b], xn, g, epsilon=epsilon)
                        ref = oracle.solveDerivativesQCQP(P, q, d["l_n"][b], d["mu"][b], xn, g, epsilon)
                    else:
                        out = M.solveDerivativesBoxQP(P, q, d["l_min"][b], d["l_max"][b], xn, g, epsilon=epsilon)
                        ref = oracle.solveDerivativesBoxQP(P, q, d["l_min"][b], d["l_max"][b], xn, g, epsilon)
                    for a, r in zip(out, ref):
                        assert np.allclose(a, r, rtol=1e-9, atol=1e-12), (structure, kind, b, epsilon)
