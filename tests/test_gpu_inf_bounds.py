"""One-sided boxes (DQQ_F_INFINITE_BOUNDS) on the device (-m gpu): every kernel family of dqq_polish_f64, dqq_newton_bwd_f64,
dqq_newton_jvp_f64 and dqq_newton_jac_f64 against the flagged host core (tests/hostcore/inf_bounds_check.cpp, held to the numpy
restatement by tests/test_inf_bounds_hostcore.py) bit for bit on small ragged batches of mixed bounds with a refused problem in the
middle; a diagonal P given as (B,N,N); the public Functions on the problem the flag exists for; replay from a captured graph.
Inputs: tests/inf_bounds_cases.py."""
import numpy as np
import pytest
import torch

import inf_bounds_cases as C
import inf_bounds_reference as IR
import polish_cases as PC
import polish_reference as R

pytestmark = pytest.mark.gpu
AUTO, DENSE, DIAG = C.AUTO, C.DENSE, C.DIAG
INF = C.INF
KEYS = C.INT_KEYS + C.FLOAT_KEYS
ROWS = C.ROWS


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()


def col(a):
    return None if a is None else dev(a[:, :, None])


def host(t):
    return t.cpu().numpy().reshape(t.shape[0], -1) if t.dim() == 3 and t.shape[2] == 1 else t.cpu().numpy()


def gpu_all(kind, P, q, ex, x, gx, tan, layout, flag=True, in_place=False):
    """The four ops with infinite_bounds=flag -> a dict keyed as inf_bounds_cases.host_all's."""
    from diffqcqp_amd import ops
    k = R.KIND[kind]
    Pd, qd, exd, xd = dev(P), col(q), [col(e) for e in ex], col(x)
    kw = dict(infinite_bounds=flag)
    o = {}
    start = xd.clone() if in_place else xd
    xo, resid, steps, st = ops._polish(k, Pd, qd, exd, start, C.MAX_STEPS, layout, out=start if in_place else None, return_info=True, **kw)
    assert (xo.data_ptr() == start.data_ptr()) == in_place
    o["x_out"], o["resid"], o["steps"], o["st_polish"] = host(xo), resid.cpu().numpy(), steps.cpu().numpy(), st.cpu().numpy()
    dx, st = ops._newton_jvp(k, Pd, qd, exd, xd, [dev(tan[0])] + [col(t) for t in tan[1:]], layout, return_status=True, **kw)
    o["dx"], o["st_jvp"] = host(dx), st.cpu().numpy()
    gP, gq, ga, gb, st = ops._newton_backward(k, Pd, qd, exd, xd, col(gx), (True,) * 4, layout, return_status=True, **kw)
    o["gP"], o["gq"], o["ga"], o["gb"], o["st_bwd"] = host(gP), host(gq), host(ga), host(gb), st.cpu().numpy()
    Jq, Ja, Jb, st = ops._newton_jacobian(k, Pd, qd, exd, xd, (True,) * 3, layout, return_status=True, **kw)
    o["Jq"], o["Ja"], o["Jb"], o["st_jac"] = Jq.cpu().numpy(), Ja.cpu().numpy(), Jb.cpu().numpy(), st.cpu().numpy()
    return o


def same_all(got, ref, what, keys=KEYS):
    for k in keys:
        assert got[k].dtype == ref[k].dtype and C.same_bits(got[k], ref[k]), "%s: %s %s vs %s" % (what, k, got[k].ravel()[:4], ref[k].ravel()[:4])


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("layout,structure,N,B", ROWS)
def test_every_family_is_the_flagged_host_core(kind, layout, structure, N, B):
    """Case 8.  The problem in the middle has l_min = +inf: status 2 with the flag too, NaN outputs, x_out = x."""
    P, q, ex, x, gx, tan = C.problem(kind, B, N, structure, bad_row=B // 2)
    diag = layout == DIAG
    Pa, ta = (C.compact(P), (C.compact(tan[0]),) + tan[1:]) if diag else (P, tan)
    ref = C.host_all(kind, Pa, q, ex, x, gx, ta, diag=diag, flag=True)
    want = np.zeros(B, dtype=np.int32)
    want[B // 2] = 2
    for k in ("st_jvp", "st_bwd", "st_jac"):
        assert np.array_equal(ref[k], want), k
    assert ref["st_polish"][B // 2] == 2 and (np.delete(ref["st_polish"], B // 2) != 2).all() and (ref["st_polish"] == 0).any()
    got = gpu_all(kind, Pa, q, ex, x, gx, ta, layout)
    same_all(got, ref, "%s N=%d layout %d" % (kind, N, layout))
    # in place: x_out = x, once per family
    same_all(gpu_all(kind, Pa, q, ex, x, gx, ta, layout, in_place=True), ref, "in place", ("x_out", "resid", "steps", "st_polish"))
    # and without the flag every problem with an infinite bound is refused, as before
    plain = gpu_all(kind, Pa, q, ex, x, gx, ta, layout, flag=False)
    has_inf = np.isinf(ex[0]).any(axis=1) | np.isinf(ex[1]).any(axis=1)
    assert has_inf.any() and all((plain[k][has_inf] == 2).all() for k in ("st_polish", "st_jvp", "st_bwd", "st_jac"))
    same_all(plain, C.host_all(kind, Pa, q, ex, x, gx, ta, diag=diag, flag=False), "unflagged")


def diagonal_p_both_ways(kind, N, B):
    P, q, ex, x, gx, tan = C.problem(kind, B, N, "diag", bad_row=B // 2)
    cd = gpu_all(kind, C.compact(P), q, ex, x, gx, (C.compact(tan[0]),) + tan[1:], DIAG)
    for layout in (AUTO, DENSE):
        full = gpu_all(kind, P, q, ex, x, gx, tan, layout)
        same_all(full, cd, "dense form of a diagonal P", C.INT_KEYS + ("x_out", "resid", "dx", "gq", "ga", "gb"))
        for k in ("gP", "Jq", "Ja", "Jb"):
            assert C.same_bits(C.compact(full[k]), cd[k]), k
            if k != "gP":   # (grad_P = -v x' is a full outer product; the Jacobians of a diagonal P are diagonal)
                assert (full[k][cd["st_jac"] == 0][:, ~np.eye(N, dtype=bool)] == 0.0).all(), k


@pytest.mark.parametrize("kind", C.KINDS)
def test_a_diagonal_P_given_dense_gives_the_diagonal_kernels_flagged_bits(kind):
    """Case 9."""
    diagonal_p_both_ways(kind, *C.DIAG_MATRIX[0])


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("N,B", C.DIAG_MATRIX[1:])
def test_a_diagonal_P_given_dense_at_the_other_diagonal_sizes(kind, N, B):
    """N = 16 runs the general kernels on their teams of 16."""
    diagonal_p_both_ways(kind, N, B)


def _twin_bound(P, q, x, v):
    """How far grad_P of two exact derivatives of the same problem may differ when their x differ: both x are within the polish's
    bar of the solution in the natural residual r, |x - x*| <= |M^-1| r with |M^-1|_inf <= sqrt(N) / lambda_min(P) (M is P on the
    free rows, the identity elsewhere; lambda_min >= 0.5 on these batches), and grad_P = -v x' moves by |v| |dx|.  Twice that for
    the two points."""
    N = x.shape[1]
    return 2.0 * np.abs(v).max() * (np.sqrt(N) / 0.5) * 64 * PC.BAR * R.scale(P, q, x).max()


def test_the_failing_before_case_through_the_public_api():
    """Case 10: BoxQPFn2 with l_max = +inf on half the coordinates, polish 8, newton derivatives."""
    from diffqcqp_amd import ops, qcqp
    N, B = 8, 37
    P, q, ex, _, gx, _ = C.problem("box", B, N, "dense")
    l_min = -np.abs(ex[1])                         # finite lower bounds ...
    l_min[~np.isfinite(l_min)] = -0.3
    l_max = np.where(np.arange(N)[None, :] % 2 == 0, INF, 0.4) * np.ones((B, 1))   # ... and l_max = +inf on half the coordinates
    prev = (qcqp.get_default_polish(), qcqp.get_default_derivative(), qcqp.get_default_infinite_bounds())
    assert prev[2] is False

    def run(fn, tensors):
        leaves = [t.clone().requires_grad_(True) for t in tensors]
        x = fn.apply(*leaves, None, 1e-4, 10000)
        grads = torch.autograd.grad(x, leaves, col(gx))
        return x.detach(), grads

    try:
        qcqp.set_default_polish(8)
        qcqp.set_default_derivative("newton")
        qcqp.set_default_infinite_bounds(True)
        tensors = (dev(P), col(q), col(l_min), col(l_max))
        x, grads = run(qcqp.BoxQPFn2, tensors)
        # the polish's own word on the point the Function saved: nothing left to do, nothing refused
        _, resid, _, status = ops.boxqp_polish(*tensors, x, 8, return_info=True, infinite_bounds=True)
        assert (status.cpu().numpy() != 2).all()
        xs = ops.boxqp_forward(*tensors, 1e-4, 10000)
        _, _, _, st = ops.boxqp_polish(*tensors, xs, 8, return_info=True, infinite_bounds=True)
        assert (st.cpu().numpy() == 0).all()       # from the loose forward: every problem accepts a step
        nat = IR.natural_residual("box", P, q, (l_min, l_max), host(x))
        bar = 64 * PC.BAR * R.scale(P, q, host(x))
        print("natural residual after the flagged polish: max %.2e, bar %.2e" % (nat.max(), bar.min()))
        assert (nat <= bar).all()
        assert all(torch.isfinite(g).all() for g in grads)
        g_hi = host(grads[3])
        assert (g_hi[np.isinf(l_max)] == 0.0).all() and not np.signbit(g_hi[np.isinf(l_max)]).any()
        assert (host(grads[2]) != 0.0).any() and (g_hi != 0.0).any()                 # finite bounds are sat on and get gradients
        # the [0, +inf) twin: QPFn2.  On the same x the two kinds share their evaluation order: the bits are equal.
        zero, inf = np.zeros((B, N)), np.full((B, N), INF)
        xb, gb_ = run(qcqp.BoxQPFn2, (dev(P), col(q), col(zero), col(inf)))
        gP, gq = ops.qp_newton_backward(dev(P), col(q), xb, col(gx))
        assert torch.equal(gP, gb_[0]) and torch.equal(gq, gb_[1])
        assert C.same_bits(host(ops.qp_polish(dev(P), col(q), xb, 8)), host(ops.boxqp_polish(dev(P), col(q), col(zero), col(inf), xb, 8,
                                                                                          infinite_bounds=True)))
        # QPFn2 itself solves with the QP's forward: another x within the polish's bar, so the gradients agree to _twin_bound
        xq, gq_ = run(qcqp.QPFn2, (dev(P), col(q)))
        assert all(torch.isfinite(g).all() for g in gq_)
        tol = _twin_bound(P, q, host(xb), host(gb_[1]))
        dP, dq = (gq_[0] - gb_[0]).abs().max().item(), (gq_[1] - gb_[1]).abs().max().item()
        print("QPFn2 against its box twin: |d grad_P| %.2e, |d grad_q| %.2e, bound %.2e" % (dP, dq, tol))
        assert dP <= tol and dq <= tol
        assert (host(gb_[2]) == 0.0).sum() > 0 and (host(gb_[3]) == 0.0).all()
        # the flag off: the same call is what it was on the parent commit -- refused, NaN gradients
        qcqp.set_default_infinite_bounds(False)
        x0, grads0 = run(qcqp.BoxQPFn2, tensors)
        _, _, _, st0 = ops.boxqp_polish(*tensors, xs, 8, return_info=True)
        assert (st0.cpu().numpy() == 2).all()
        assert torch.equal(x0, xs)                                                    # left unpolished
        assert all(torch.isnan(g).all() for g in grads0)
    finally:
        qcqp.set_default_polish(prev[0])
        qcqp.set_default_derivative(prev[1])
        qcqp.set_default_infinite_bounds(prev[2])


def test_forward_flagged_polish_and_newton_backward_in_a_captured_graph():
    """Case 11: kind 2, dense, N = 8, B = 37 -- replayed bit-equal to eager."""
    from diffqcqp_amd import ops
    N, B, k = 8, 37, 2
    P, q, ex, _, gx, _ = C.problem("box", B, N, "dense")
    Pd, qd, exd, g = dev(P), col(q), [col(e) for e in ex], col(gx)
    kw = dict(infinite_bounds=True)
    xe = ops._polish(k, Pd, qd, exd, ops._forward(k, Pd, qd, exd, 1e-4, 1000), 8, **kw)
    eager = ops._newton_backward(k, Pd, qd, exd, xe, g, **kw)
    assert all(torch.isfinite(a).all() for a in eager)
    ws = ops.make_workspace(torch.device("cuda"), B, k, 0, N)
    x = torch.zeros((B, N, 1), dtype=torch.float64, device="cuda")
    outs = [torch.zeros_like(a) for a in eager]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        def chain():
            ops._forward(k, Pd, qd, exd, 1e-4, 1000, out=x, workspace=ws)
            ops._polish(k, Pd, qd, exd, x, 8, out=x, **kw)
            ops._newton_backward(k, Pd, qd, exd, x, g, out=outs, **kw)
        chain()                                              # warm-up on the capture stream
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            chain()
    torch.cuda.current_stream().wait_stream(stream)
    for o in outs:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(x, xe)
    for a, b in zip(outs, eager):
        assert torch.equal(a, b)
