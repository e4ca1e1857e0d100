"""dqq_jvp_f64 and Function.jvp on the device (-m gpu): every route family and kind against the host core
(tests/hostcore/jvp_check.cpp, held bit-equal to the numpy restatement on the CPU) at the bar that family's backward is held to
against the oracle in its small-batch test -- bit-equal, step counts included, for the diagonal kernel, the LDS team kernel
and the global-memory kernel alike (tests/test_gpu_parity.py: check_backward_exact) --, then the properties of the entry point:
non-default epsilon, single tangents, NULL = zero, batch slices, the adjoint identity against the library's own backward, the signed box QP as the
box QP at the effective bounds, autograd's forward mode, HIP-graph capture, NaN isolation.  Inputs: tests/jvp_cases.py."""
import numpy as np
import pytest
import torch

import jvp_cases as C
import jvp_reference as R
from sbox_cases import effective_bounds

pytestmark = pytest.mark.gpu

AUTO, DENSE, DIAG = 0, 1, 2
DIAG_ROWS = [(k, N, 67) for k in C.EXTRAS for N in (2, 8, 64)] + [("box", 16, 67), ("qcqp", 4, 67), ("qp", 32, 67)]
TEAM_ROWS = [(k, N, 37) for k in C.EXTRAS for N in (3, 8, 16, 21) if not (k == "qcqp" and N % 2)] + [("qcqp", 42, 37), ("qp", 64, 37)]
ANY_ROWS = [("box", 22, 5), ("sbox", 22, 5), ("qcqp", 44, 5), ("qp", 65, 5)]
# one row per persistent family past its first trip: 2 * per_trip + 1 problems and more, sized as tests/trip_cases.py sizes the
# backward's rows of the same geometry (bteam QCQP N = 18: 4096 per trip; bany: 512), on a tiled base of 61 problems
TRIP_ROWS = [("qcqp", 18, 8195, 61), ("box", 22, 1027, 61)]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ops_jvp(kind, d, x, tan, layout, B=None, **kw):
    """ops._jvp on a batch given as numpy arrays.  tan: jvp_reference's flat tangents (dP (B,N,N), dq (B,N), ...), None = NULL.
    DIAG: P and dP go in as their compact diagonals.  B: tile the batch up to B problems."""
    from diffqcqp_amd import ops
    n = d["q"].shape[1]
    rep = (lambda a: a) if B is None else (lambda a: np.concatenate([a] * -(-B // a.shape[0]))[:B])
    P, dP = d["P"], tan[0]
    if layout == DIAG:
        P = np.diagonal(P, axis1=1, axis2=2)
        dP = None if dP is None else np.diagonal(dP, axis1=1, axis2=2)
    shaped = [dP, None if tan[1] is None else tan[1][:, :, None]] + [None if t is None else t[:, :, None] for t in tan[2:]]
    extras = [dev(rep(d[k])) for k in C.EXTRAS[kind]]
    return ops._jvp(R.KIND[kind], dev(rep(P)), dev(rep(d["q"])), extras, dev(rep(x)), [None if t is None else dev(rep(t)) for t in shaped],
                    layout, **kw)


def check_against_host(kind, N, B, layout, structure):
    d, x = C.problem(kind, N, B, structure)
    tan = R.random_tangents(kind, B, N, 3 + N, diag=layout == DIAG)
    ref, ref_steps = C.host_jvp(kind, d, x, tan)
    dx, steps = ops_jvp(kind, d, x, tan, layout, return_steps=True)
    dx, steps = dx.cpu().numpy()[:, :, 0], steps.cpu().numpy().reshape(ref_steps.shape)
    print("%s N=%d B=%d layout %d: max |dx - host| %.3g, steps %s" % (kind, N, B, layout, np.abs(dx - ref).max(), np.unique(steps)))
    assert np.array_equal(steps, ref_steps), "refinement step counts differ"
    assert np.array_equal(dx, ref), "max diff %g" % np.abs(dx - ref).max()
    assert np.abs(ref).max() > 1e-3
    return d, x, tan, dx


@pytest.mark.parametrize("kind,N,B", DIAG_ROWS)
def test_diagonal_kernel_is_the_host_core(oracle, kind, N, B):
    check_against_host(kind, N, B, DIAG, "diag")


@pytest.mark.parametrize("layout", [AUTO, DENSE])
@pytest.mark.parametrize("kind,N,B", TEAM_ROWS)
def test_team_kernel_is_the_host_core(oracle, kind, N, B, layout):
    check_against_host(kind, N, B, layout, "dense")


@pytest.mark.parametrize("kind,N,B", ANY_ROWS)
def test_global_memory_kernel_is_the_host_core(oracle, kind, N, B):
    check_against_host(kind, N, B, DENSE, "dense")


@pytest.mark.parametrize("epsilon", C.EPSILONS)
@pytest.mark.parametrize("kind,N,B,structure", C.EPSILON_ROWS)
def test_every_family_applies_the_callers_epsilon(oracle, kind, N, B, structure, epsilon):
    """epsilon sets the active sets: on jvp_cases.loose_problem's x, whose near-active coordinates lie about 1e-4 off their bounds
    (tests/test_jvp_reference.py: the three epsilons give different dx on most of every batch), each family is the host core
    at the caller's epsilon bit for bit, step counts included -- and not at another one."""
    layout = DIAG if structure == "diag" else DENSE
    d, x = C.loose_problem(kind, N, B, structure)
    tan = C.epsilon_tangents(kind, N, B, structure)
    ref, ref_steps = C.host_jvp(kind, d, x, tan, epsilon=epsilon)
    dx, steps = ops_jvp(kind, d, x, tan, layout, return_steps=True, epsilon=epsilon)
    dx, steps = dx.cpu().numpy()[:, :, 0], steps.cpu().numpy().reshape(ref_steps.shape)
    other = C.host_jvp(kind, d, x, tan, epsilon=C.EPSILONS[0] if epsilon == C.EPSILONS[-1] else C.EPSILONS[-1])[0]
    print("%s N=%d %s epsilon %g: max |dx - host| %.3g, rows that another epsilon moves %d of %d, steps %s" % (
        kind, N, structure, epsilon, np.abs(dx - ref).max(), (other != ref).any(axis=1).sum(), B, np.unique(steps)))
    assert np.array_equal(steps, ref_steps), "refinement step counts differ"
    assert np.array_equal(dx.view(np.int64), ref.view(np.int64)), "max diff %g" % np.abs(dx - ref).max()


def test_auto_on_a_diagonal_p_is_the_general_kernel(oracle):
    """DQQ_P_AUTO never assumes: a diagonal P through the general kernel, against the host core AND the diagonal kernel's bits."""
    for kind in C.EXTRAS:
        d, x, tan, dx = check_against_host(kind, 8, 67, AUTO, "diag")
        tan_d = (tan[0] * np.eye(8),) + tan[1:]
        a = ops_jvp(kind, d, x, tan_d, AUTO).cpu().numpy()
        b = ops_jvp(kind, d, x, tan_d, DIAG).cpu().numpy()
        assert np.array_equal(a, b), kind


@pytest.mark.parametrize("kind,N,B,base", TRIP_ROWS)
def test_persistent_kernels_past_their_first_trip(oracle, kind, N, B, base):
    d, x = C.problem(kind, N, base, "dense")
    tan = R.random_tangents(kind, base, N, 5)
    ref, ref_steps = C.host_jvp(kind, d, x, tan)
    dx, steps = ops_jvp(kind, d, x, tan, DENSE | 0x100, B=B, return_steps=True)
    dx, steps = dx.cpu().numpy()[:, :, 0], steps.cpu().numpy().reshape(B, -1)
    assert np.array_equal(dx[:base], ref) and np.array_equal(steps[:base], ref_steps)
    idx = np.arange(B) % base
    assert np.array_equal(dx, dx[:base][idx]) and np.array_equal(steps, steps[:base][idx])   # every replica: the first one's bits


@pytest.mark.parametrize("kind,N,B,layout,structure", [(k, 8, 67, DIAG, "diag") for k in C.EXTRAS] +
                         [(k, 8, 37, DENSE, "dense") for k in C.EXTRAS] + [("box", 22, 5, DENSE, "dense"), ("qcqp", 44, 5, DENSE, "dense")])
def test_single_tangents_null_tangents_and_batch_slices(oracle, kind, N, B, layout, structure):
    from diffqcqp_amd import ops
    d, x = C.problem(kind, N, B, structure)
    tan = R.random_tangents(kind, B, N, 17, diag=layout == DIAG)
    full = ops_jvp(kind, d, x, tan, layout)
    for i in range(len(tan)):
        only = tuple(t if j == i else None for j, t in enumerate(tan))
        zeros = tuple(t if j == i else np.zeros_like(t) for j, t in enumerate(tan))
        a, b = ops_jvp(kind, d, x, only, layout), ops_jvp(kind, d, x, zeros, layout)
        assert torch.equal(a, b), i                      # NULL is a zero buffer, bit for bit
        assert np.array_equal(a.cpu().numpy()[:, :, 0], C.host_jvp(kind, d, x, only)[0]), i
    assert not ops_jvp(kind, d, x, (None,) * len(tan), layout).any()
    # a batch slice t[1:] of every argument is a valid argument and gives the unsliced call's bits
    P = d["P"] if layout != DIAG else np.diagonal(d["P"], axis1=1, axis2=2)
    dP = tan[0] if layout != DIAG else np.diagonal(tan[0], axis1=1, axis2=2)
    t = [dev(a) for a in (P, d["q"], x, dP, tan[1][:, :, None])]
    ex = [dev(d[k]) for k in C.EXTRAS[kind]]
    te = [dev(a[:, :, None]) for a in tan[2:]]
    sl = ops._jvp(R.KIND[kind], t[0][1:], t[1][1:], [e[1:] for e in ex], t[2][1:], [t[3][1:], t[4][1:]] + [a[1:] for a in te], layout)
    assert torch.equal(sl, full[1:])


def _backward(kind, d, x, g, layout):
    from diffqcqp_amd import ops
    P = d["P"] if layout != DIAG else np.diagonal(d["P"], axis1=1, axis2=2)
    args = [dev(P), dev(d["q"])] + [dev(d[k]) for k in C.EXTRAS[kind]]
    out = ops._backward(R.KIND[kind], args[0], args[1], args[2:], dev(x), dev(g[:, :, None]), (True,) * 4, layout | 0x100, False, None,
                        C.EPSILON, None, None, None)
    grads = [o.cpu().numpy() for o in out]
    if layout == DIAG:
        grads[0] = np.stack([np.diag(r) for r in grads[0]])
    return [grads[0]] + [a[:, :, 0] for a in grads[1:]]


@pytest.mark.parametrize("kind", list(C.EXTRAS))
@pytest.mark.parametrize("N,B,structure", C.ADJOINT_BATCHES)
def test_adjoint_identity_against_the_librarys_backward(oracle, kind, N, B, structure):
    """<g, dx> = sum <grad, tangent> per problem, the JVP against the backward of the same route family (DQQ_P_DIAG against
    DQQ_P_DIAG, the reference-order general kernels against each other), within 10 x the gap the numpy restatement's two modes
    leave on the same batches (jvp_cases.ADJOINT_GAP_CPU, measured on the CPU by tests/test_jvp_reference.py)."""
    if kind == "qcqp" and N % 2:
        N += 1
    layout = DIAG if structure == "diag" else DENSE
    d, x = C.problem(kind, N, B, structure)
    tan, g = C.adjoint_inputs(kind, N, B, structure)
    dx = ops_jvp(kind, d, x, tan, layout).cpu().numpy()[:, :, 0]
    grads = _backward(kind, d, x, g, layout)
    gap = C.adjoint_gap(g, dx, grads, tan)
    print("%s N=%d %s: adjoint gap %.3g (CPU record %.3g)" % (kind, N, structure, gap, C.ADJOINT_GAP_CPU[kind]))
    assert gap <= 10 * C.ADJOINT_GAP_CPU[kind]


@pytest.mark.parametrize("N,B,layout,structure", [(8, 67, DIAG, "diag"), (8, 37, DENSE, "dense"), (22, 5, DENSE, "dense")])
def test_signed_box_is_the_box_jvp_at_the_effective_bounds(oracle, N, B, layout, structure):
    d, x = C.problem("sbox", N, B, structure)
    tan = R.random_tangents("sbox", B, N, 23, diag=layout == DIAG)
    lo, hi, keep_lo, keep_hi = (t.numpy() for t in effective_bounds(*(torch.from_numpy(np.array(d[k])) for k in ("l_min", "l_max", "v"))))
    assert (~keep_lo).any() and (~keep_hi).any() and keep_lo.any() and keep_hi.any()
    box = dict(d, l_min=lo, l_max=hi)
    masked = tan[:2] + (np.where(keep_lo[:, :, 0], tan[2], 0.0), np.where(keep_hi[:, :, 0], tan[3], 0.0))
    a, sa = ops_jvp("sbox", d, x, tan, layout, return_steps=True)
    b, sb = ops_jvp("box", box, x, masked, layout, return_steps=True)
    assert torch.equal(a, b) and torch.equal(sa, sb)


def _functions():
    from diffqcqp_amd import qcqp as Q
    return {"qp": (Q.QPFn2, Q.QPWarmFn2), "qcqp": (Q.QCQPFn2, Q.QCQPWarmFn2), "box": (Q.BoxQPFn2, Q.BoxQPWarmFn2),
            "sbox": (Q.SignedBoxQPDiffFn2, Q.SignedBoxQPWarmFn2)}


@pytest.mark.parametrize("kind", list(C.EXTRAS))
def test_forward_ad_through_every_function_is_ops_jvp(oracle, kind):
    import torch.autograd.forward_ad as fwAD
    from diffqcqp_amd import ops, qcqp as Q
    N, B = 8, 37
    d, _ = C.problem(kind, N, B, "dense")
    tan = R.random_tangents(kind, B, N, 29)
    prim = [dev(d["P"]), dev(d["q"])] + [dev(d[k]) for k in C.EXTRAS[kind]]
    tans = [dev(tan[0]), dev(tan[1][:, :, None])] + [dev(t[:, :, None]) for t in tan[2:]]
    prev = Q.set_default_layout("dense")
    try:
        for F in _functions()[kind]:
            with fwAD.dual_level():
                duals = [fwAD.make_dual(p, t) for p, t in zip(prim, tans)] + prim[len(tans):]     # (v: no tangent)
                x0 = torch.zeros_like(prim[1])
                out = F.apply(*duals, x0, 1e-10, 100000)
                x, dx = fwAD.unpack_dual(out)
            want = ops._jvp(R.KIND[kind], prim[0], prim[1], prim[2:], x, tans, DENSE)
            assert dx is not None and torch.equal(dx, want), F.__name__
            with fwAD.dual_level():      # one tangent only: the others reach the kernel as NULL
                out = F.apply(prim[0], fwAD.make_dual(prim[1], tans[1]), *prim[2:], x0, 1e-10, 100000)
                assert torch.equal(fwAD.unpack_dual(out).tangent, ops._jvp(R.KIND[kind], prim[0], prim[1], prim[2:], x, [None, tans[1]], DENSE))
        if kind == "sbox":
            with fwAD.dual_level(), pytest.raises(NotImplementedError):
                Q.SignedBoxQPFn2.apply(prim[0], fwAD.make_dual(prim[1], tans[1]), *prim[2:], torch.zeros_like(prim[1]), 1e-10, 100000)
    finally:
        Q.set_default_layout(prev)


@pytest.mark.parametrize("kind", list(C.EXTRAS))
def test_func_jvp_agrees_with_autograd_grad_through_the_adjoint_identity(oracle, kind):
    """torch.func.jvp through the Function is ops._jvp bit for bit, and <g, dx> = sum <grad, tangent> against the gradients
    torch.autograd.grad takes through the same Function, at the adjoint bar: 10 x jvp_cases.ADJOINT_GAP_CPU."""
    from diffqcqp_amd import ops, qcqp as Q
    N, B, structure = C.ADJOINT_BATCHES[0]
    d, _ = C.problem(kind, N, B, structure)
    tan, g = C.adjoint_inputs(kind, N, B, structure)
    prim = [dev(d["P"]), dev(d["q"])] + [dev(d[k]) for k in C.EXTRAS[kind]]
    tans = [dev(tan[0]), dev(tan[1][:, :, None])] + [dev(t[:, :, None]) for t in tan[2:]]
    nt = len(tans)
    x0 = torch.zeros_like(prim[1])
    prev = Q.set_default_layout("dense")
    try:
        for F in _functions()[kind]:
            f = lambda *a: F.apply(*a, *prim[nt:], x0, 1e-10, 100000)   # noqa: E731  (v rides along without a tangent)
            x, dx = torch.func.jvp(f, tuple(prim[:nt]), tuple(tans))
            assert torch.equal(dx, ops._jvp(R.KIND[kind], prim[0], prim[1], prim[2:], x, tans, DENSE)), F.__name__
            leaves = [p.clone().requires_grad_(True) for p in prim[:nt]]
            out = f(*leaves)
            assert torch.equal(out, x)
            grads = torch.autograd.grad(out, leaves, dev(g[:, :, None]))
            flat = [grads[0].cpu().numpy()] + [a.cpu().numpy()[:, :, 0] for a in grads[1:]]
            gap = C.adjoint_gap(g, dx.cpu().numpy()[:, :, 0], flat, tan)
            print("%s %s: adjoint gap %.3g (CPU record %.3g)" % (kind, F.__name__, gap, C.ADJOINT_GAP_CPU[kind]))
            assert gap <= 10 * C.ADJOINT_GAP_CPU[kind]
        if kind == "sbox":
            with pytest.raises(NotImplementedError):
                torch.func.jvp(lambda q: Q.SignedBoxQPFn2.apply(prim[0], q, *prim[2:], x0, 1e-10, 100000), (prim[1],), (tans[1],))
    finally:
        Q.set_default_layout(prev)


def test_one_problem_functions_of_the_numpy_module(oracle):
    from diffqcqp_amd import diffqcqp as M
    d, x = C.problem("qcqp", 8, 37, "dense")
    tan = R.random_tangents("qcqp", 37, 8, 31)
    ref = C.host_jvp("qcqp", d, x, tan)[0]
    got = M.jvpQCQP(d["P"][2], d["q"][2], d["l_n"][2], d["mu"][2], x[2], tan[0][2], tan[1][2], tan[2][2], tan[3][2])
    assert got.shape == (8,) and np.array_equal(got, ref[2])
    d, x = C.problem("sbox", 8, 37, "dense")
    tan = R.random_tangents("sbox", 37, 8, 31)
    got = M.jvpSignedBoxQP(d["P"][1], d["q"][1], d["l_min"][1], d["l_max"][1], d["v"][1], x[1], dq=tan[1][1], dl_max=tan[3][1])
    assert np.array_equal(got, C.host_jvp("sbox", d, x, (None, tan[1], None, tan[3]))[0][1])


@pytest.mark.parametrize("kind,layout,structure", [("qcqp", DIAG, "diag"), ("box", DENSE, "dense"), ("qp", DENSE, "dense")])
def test_forward_and_jvp_captured_into_a_graph_replay_to_the_same_bits(oracle, kind, layout, structure):
    from diffqcqp_amd import ops
    N, B = 8, 67
    d, _ = C.problem(kind, N, B, structure)
    tan = R.random_tangents(kind, B, N, 37, diag=layout == DIAG)
    P = d["P"] if layout != DIAG else np.diagonal(d["P"], axis1=1, axis2=2)
    dP = tan[0] if layout != DIAG else np.diagonal(tan[0], axis1=1, axis2=2)
    Pd, qd, ex = dev(P), dev(d["q"]), [dev(d[k]) for k in C.EXTRAS[kind]]
    tans = [dev(dP), dev(tan[1][:, :, None])] + [dev(t[:, :, None]) for t in tan[2:]]
    x, dx = torch.empty_like(qd), torch.empty_like(qd)

    def step():
        ops._forward(R.KIND[kind], Pd, qd, ex, 1e-10, 100000, layout=layout, out=x)
        ops._jvp(R.KIND[kind], Pd, qd, ex, x, tans, layout, out=dx)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                               # warm-up: the stream's workspace exists before the capture
        s.synchronize()
        x_eager, dx_eager = x.clone(), dx.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            step()
        for _ in range(2):
            x.fill_(float("nan"))
            dx.fill_(float("nan"))
            graph.replay()
            s.synchronize()
            assert torch.equal(x, x_eager) and torch.equal(dx, dx_eager)
    torch.cuda.current_stream().wait_stream(s)


@pytest.mark.parametrize("kind,N,B,layout,structure", [(k, 8, 67, DIAG, "diag") for k in C.EXTRAS] +
                         [(k, 8, 37, DENSE, "dense") for k in C.EXTRAS] + [("box", 22, 5, DENSE, "dense")])
def test_a_nan_x_stays_in_its_problem(oracle, kind, N, B, layout, structure):
    d, x = C.problem(kind, N, B, structure)
    tan = R.random_tangents(kind, B, N, 41, diag=layout == DIAG)
    clean = ops_jvp(kind, d, x, tan, layout)
    bad = x.copy()
    bad[3, 1, 0] = np.nan
    got = ops_jvp(kind, d, bad, tan, layout)
    keep = torch.arange(B, device=got.device) != 3
    assert torch.equal(got[keep], clean[keep])
