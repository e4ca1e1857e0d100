"""dqq_newton_bwd_f64 / dqq_newton_jvp_f64 on the device (-m gpu): every route family, kind and mode against the host core
(tests/hostcore/newton_core_check.cpp, held bit-equal to the numpy restatement on the CPU) bit for bit -- every output and the
status --, with NaN, Inf and singular problems in the middle of the batch, a diagonal P through the general kernel and
single-output requests; the adjoint identity between the two entry points and between torch.func.jvp and torch.autograd.grad
under set_default_derivative("newton"); and the Functions: the default setting untouched, "newton" with a polish equal to the
ops at the saved x, replayable from a captured graph.  Inputs: tests/newton_cases.py over tests/polish_cases.py."""
import numpy as np
import pytest
import torch

import jvp_cases as JC
import newton_cases as C
import polish_cases as PC
import polish_reference as R

pytestmark = pytest.mark.gpu

AUTO, DENSE, DIAG = PC.AUTO, PC.DENSE, PC.DIAG
DIAG_ROWS, TEAM_ROWS, ANY_ROWS = C.DIAG_ROWS, C.TEAM_ROWS, C.ANY_ROWS


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()


def col(a):
    return None if a is None else dev(a[:, :, None])


def host(t):
    return None if t is None else t.cpu().numpy().reshape(t.shape[0], -1) if t.dim() == 3 and t.shape[2] == 1 else t.cpu().numpy()


def batch(kind, N, B, structure):
    """-> (P (B,N,N), q, ex, x (B,N)): polish_cases' batch, x its loose forward polished on the device (ops._polish, held to its
    own host core by tests/test_gpu_polish.py); tangents and cotangent from newton_cases.inputs."""
    from diffqcqp_amd import ops
    d, x0 = PC.problem(kind, N, B, structure)
    P, q, ex = PC.flat(d, kind)
    x = ops._polish(R.KIND[kind], dev(P), col(q), [col(e) for e in ex], dev(x0), PC.MAX_STEPS, DENSE)
    return P, q, ex, x.cpu().numpy()[:, :, 0]


def gpu_jvp(kind, P, q, ex, x, tan, layout, **kw):
    from diffqcqp_amd import ops
    tan = tuple(tan) + (None,) * (4 - len(tan))
    t = [dev(tan[0])] + [col(v) for v in tan[1:]]
    dx, st = ops._newton_jvp(R.KIND[kind], dev(P), col(q), [col(e) for e in ex], col(x), t, layout, return_status=True, **kw)
    return host(dx), st.cpu().numpy()


def gpu_bwd(kind, P, q, ex, x, g, layout, need=(True, True, True, True), **kw):
    from diffqcqp_amd import ops
    out = ops._newton_backward(R.KIND[kind], dev(P), col(q), [col(e) for e in ex], col(x), col(g), need, layout, return_status=True,
                               **kw)
    out = tuple(out) if kind != "qp" else (out[0], out[1], None, None, out[2])
    return tuple(host(t) for t in out[:4]) + (out[4].cpu().numpy(),)


def same_all(got, ref, what):
    for i, (g, r) in enumerate(zip(got, ref)):
        assert (g is None) == (r is None), (what, i)
        if r is not None:
            assert g.dtype == r.dtype and C.same_bits(g, r), "%s output %d: %s vs %s" % (what, i, g.ravel()[:4], r.ravel()[:4])


def with_bad_rows(kind, P, q, ex, x):
    """Copies with a singular, a NaN and an Inf problem in the middle of the batch (B >= 5) -> (P, q, ex, x, want status)."""
    B = x.shape[0]
    P, q, x, ex = P.copy(), q.copy(), x.copy(), tuple(e.copy() for e in ex)
    want = np.zeros(B, dtype=np.int32)
    if B < 5:
        return P, q, ex, x, want
    m = B // 2
    x[m, -1] = np.nan
    P[m + 1, 1, 1] = np.inf
    want[[m, m + 1]] = 2
    s = m - 1                     # a zero row of P at a coordinate that is free whatever the kind
    P[s, 0, :] = 0.0
    x[s, 0], q[s, 0] = 0.01, -0.01
    if kind == "qcqp":
        P[s, 1, :] = 0.0
        P[s, 1, 1] = 1.0
        x[s, 1], q[s, 1] = 0.0, 0.0
        ex[0][s, 0], ex[1][s, 0] = 1.0, 1.0
    elif kind != "qp":
        ex[0][s, 0], ex[1][s, 0] = -1.0, 1.0
        if kind == "sbox":
            ex[2][s, 0] = -1.0
    want[s] = 1
    return P, q, ex, x, want


def check_family(kind, N, B, layout, structure, **kw):
    P, q, ex, x = batch(kind, N, B, structure)
    tan, g = C.inputs(kind, N, B, structure)
    Pb, qb, exb, xb, want = with_bad_rows(kind, P, q, ex, x)
    diag = layout == DIAG
    for Pi, qi, exi, xi, wi in ((P, q, ex, x, np.zeros(B, dtype=np.int32)), (Pb, qb, exb, xb, want)):
        Pa = PC.compact(Pi) if diag else Pi
        ta = ((PC.compact(tan[0]) if diag else tan[0]),) + tan[1:]
        ref_j = C.host_jvp(kind, Pa, qi, exi, xi, ta, diag=diag)
        ref_b = C.host_backward(kind, Pa, qi, exi, xi, g, diag=diag)
        assert np.array_equal(ref_j[1], wi) and np.array_equal(ref_b[4], wi)
        got_j, got_b = gpu_jvp(kind, Pa, qi, exi, xi, ta, layout, **kw), gpu_bwd(kind, Pa, qi, exi, xi, g, layout, **kw)
        same_all(got_j, ref_j, "%s N=%d jvp" % (kind, N))
        same_all(got_b, ref_b, "%s N=%d bwd" % (kind, N))
        if wi.any():   # the neighbours of the bad problems are what they were
            keep = wi == 0
            same_all(tuple(a[keep] for a in got_j), tuple(a[keep] for a in clean_j), "jvp neighbours")
            same_all(tuple(None if a is None else a[keep] for a in got_b), tuple(None if a is None else a[keep] for a in clean_b),
                     "bwd neighbours")
        else:
            clean_j, clean_b = got_j, got_b
    # single-output requests and NULL tangents
    Pa = PC.compact(P) if diag else P
    ta = ((PC.compact(tan[0]) if diag else tan[0]),) + tan[1:]
    for i in range(2 if kind == "qp" else 4):
        need = tuple(j == i for j in range(4))
        one = gpu_bwd(kind, Pa, q, ex, x, g, layout, need, **kw)
        assert C.same_bits(one[i], clean_b[i]) and all(one[j] is None for j in range(4) if j != i), (kind, i)
        part = tuple(t if j == i else None for j, t in enumerate(ta))
        same_all(gpu_jvp(kind, Pa, q, ex, x, part, layout, **kw), C.host_jvp(kind, Pa, q, ex, x, part, diag=diag), "NULL tangents")
    return P, q, ex, x, tan, g, clean_j, clean_b


@pytest.mark.parametrize("kind,N,B", DIAG_ROWS)
def test_diagonal_kernel_is_the_host_core(oracle, kind, N, B):
    P, q, ex, x, tan, g, dj, db = check_family(kind, N, B, DIAG, "diag")
    # the same diagonal P as (B,N,N) through the general kernel: DQQ_P_DIAG's bits
    fj, fb = gpu_jvp(kind, P, q, ex, x, tan, DENSE), gpu_bwd(kind, P, q, ex, x, g, DENSE)
    same_all(fj, dj, "dense jvp of a diagonal P")
    assert C.same_bits(PC.compact(fb[0]), db[0])
    same_all(fb[1:], db[1:], "dense bwd of a diagonal P")
    if B > 8:   # a batch slice that starts at an odd problem
        s = slice(3, B)
        cut = lambda t: tuple(None if a is None else a[s] for a in t)   # noqa: E731
        same_all(gpu_jvp(kind, PC.compact(P)[s], q[s], cut(ex), x[s], (PC.compact(tan[0])[s],) + cut(tan[1:]), DIAG), cut(dj), "slice")


@pytest.mark.parametrize("layout", C.TEAM_LAYOUTS)
@pytest.mark.parametrize("kind,N,B", TEAM_ROWS)
def test_team_kernel_is_the_host_core(oracle, kind, N, B, layout):
    check_family(kind, N, B, layout, "dense")


@pytest.mark.parametrize("kind,N,B", ANY_ROWS)
def test_global_memory_kernel_is_the_host_core(oracle, kind, N, B):
    from diffqcqp_amd import ops
    ws = ops.newton_workspace(torch.device("cuda"), R.KIND[kind], N, B)
    assert ws is not None and ws.numel() * 4 == ops._capi.lib().dqq_newton_scratch_bytes(R.KIND[kind], N, B)
    assert ops.newton_workspace(torch.device("cuda"), R.KIND[kind], 64, B) is None
    check_family(kind, N, B, DENSE, "dense", workspace=ws)


@pytest.mark.parametrize("kind,N,structure", [(k, N, s) for k in C.KINDS for N in (8, 20) for s in ("diag", "dense")])
def test_adjoint_identity_between_the_two_entry_points(oracle, kind, N, structure):
    """The CPU measurement's batches: 10 x the record, the JVP tests' margin -- a bar that means something for every kind."""
    P, q, ex, x = C.problem(kind, N, structure)
    tan, g = C.inputs(kind, N, x.shape[0], structure)
    for layout in (DENSE,) + ((DIAG,) if structure == "diag" and N == 8 else ()):
        Pa = PC.compact(P) if layout == DIAG else P
        ta = ((PC.compact(tan[0]) if layout == DIAG else tan[0]),) + tan[1:]
        dx, sj = gpu_jvp(kind, Pa, q, ex, x, ta, layout)
        out = gpu_bwd(kind, Pa, q, ex, x, g, layout)
        assert not sj.any() and not out[4].any()
        gap = JC.adjoint_gap(g, dx, [o for o in out[:4] if o is not None], ta)
        print("%s N=%d %s layout %d: adjoint gap %.3g" % (kind, N, structure, layout, gap))
        assert gap <= 10 * C.ADJOINT_GAP_CPU[kind]


def _functions(kind):
    from diffqcqp_amd import qcqp
    return {"qp": qcqp.QPFn2, "qcqp": qcqp.QCQPFn2, "box": qcqp.BoxQPFn2, "sbox": qcqp.SignedBoxQPDiffFn2}[kind]


@pytest.mark.parametrize("kind", C.KINDS)
def test_jvp_and_grad_of_the_functions_are_adjoint_under_newton(oracle, kind):
    from diffqcqp_amd import qcqp
    N, B = 8, 32
    d, _ = PC.problem(kind, N, B, "dense")
    t = {k: dev(v) for k, v in d.items()}
    names = PC.EXTRAS[kind]
    ins = [t["P"], t["q"]] + [t[n] for n in names]
    nd = 2 + min(len(names), 2)          # differentiable inputs
    tan, g = C.inputs(kind, N, B, "dense", seed=1)
    tans = [dev(tan[0]), col(tan[1])] + [col(v) for v in tan[2:]]
    fn = _functions(kind)
    eps, max_iter = 1e-4, 1000
    prev_p, prev_d = qcqp.set_default_polish(8), qcqp.set_default_derivative("newton")
    assert prev_d == "reference"
    try:
        f = lambda *a: fn.apply(*a, *ins[nd:], None, eps, max_iter)   # noqa: E731
        _, dx = torch.func.jvp(f, tuple(ins[:nd]), tuple(tans))
        leaves = [a.clone().requires_grad_(True) for a in ins[:nd]]
        grads = torch.autograd.grad(f(*leaves), leaves, col(g))
    finally:
        assert qcqp.set_default_derivative(prev_d) == "newton"
        qcqp.set_default_polish(prev_p)
    gap = JC.adjoint_gap(g, host(dx), [host(a) if a.dim() == 3 and a.shape[2] == 1 else a.cpu().numpy() for a in grads], tan)
    print("%s: adjoint gap of Function.jvp and backward %.3g" % (kind, gap))
    assert gap <= 10 * C.ADJOINT_GAP_CPU[kind]


class Recorder:
    """A proxy of the library handle that writes down the name of every C call made through it."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("dqq_") or not callable(fn):
            return fn

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call


@pytest.mark.parametrize("kind", C.KINDS)
def test_functions_default_is_untouched_and_newton_is_the_ops(oracle, kind, monkeypatch):
    from diffqcqp_amd import _capi, ops, qcqp
    N, B = 8, 37
    k = R.KIND[kind]
    d, _ = PC.problem(kind, N, B, "dense")
    t = {n: dev(v) for n, v in d.items()}
    ins = [t["P"], t["q"]] + [t[n] for n in PC.EXTRAS[kind]]
    nd = 2 + min(len(ins) - 2, 2)
    fn = _functions(kind)
    eps, max_iter = 1e-4, 1000
    g = col(C.inputs(kind, N, B, "dense")[1])
    rec = Recorder(_capi.lib())
    monkeypatch.setattr(_capi, "_lib", rec)

    def run():
        leaves = [a.clone().requires_grad_(True) for a in ins[:nd]]
        x = fn.apply(*leaves, *ins[nd:], None, eps, max_iter)
        return x.detach(), torch.autograd.grad(x, leaves, g)

    # the default: the reference derivative, call for call and bit for bit
    assert qcqp.get_default_derivative() == "reference" and qcqp.get_default_polish() == 0
    x, grads = run()
    fwd, bwd = ops._KIND[k][2], ops._KIND[k][3]
    made = [c for c in rec.calls if c.endswith("_f64")]
    assert made == [fwd, bwd], made
    ref = ops._backward(k, ins[0], ins[1], ins[2:], x, g, (True,) * 4, AUTO, False, None, 1e-10, None, None, None)
    for a, b in zip(grads, ref):
        assert torch.equal(a, b)
    # "newton" with a polish: forward, polish, the Newton backward; equal to the op at the saved x
    del rec.calls[:]
    qcqp.set_default_polish(8)
    qcqp.set_default_derivative("newton")
    try:
        xn, gn = run()
    finally:
        qcqp.set_default_derivative("reference")
        qcqp.set_default_polish(0)
    assert [c for c in rec.calls if c.endswith("_f64")] == [fwd, "dqq_polish_f64", "dqq_newton_bwd_f64"]
    assert torch.equal(xn, ops._polish(k, ins[0], ins[1], ins[2:], x, 8))
    front = {"qp": ops.qp_newton_backward, "qcqp": ops.qcqp_newton_backward, "box": ops.boxqp_newton_backward,
             "sbox": ops.signedboxqp_newton_backward}[kind]
    out = front(*ins, xn, g, return_status=True)
    assert not out[-1].any().item()
    for a, b in zip(gn, out[:-1]):
        assert torch.equal(a, b)
    assert not torch.equal(gn[1], grads[1])     # (and it is another derivative than the default's)
    # the raising class keeps raising under either setting
    if kind == "sbox":
        qcqp.set_default_derivative("newton")
        try:
            leaves = [a.clone().requires_grad_(True) for a in ins[:4]]
            x = qcqp.SignedBoxQPFn2.apply(*leaves, ins[4], None, eps, max_iter)
            with pytest.raises(NotImplementedError):
                torch.autograd.grad(x.sum(), leaves[1])
        finally:
            qcqp.set_default_derivative("reference")


def test_forward_polish_and_newton_backward_in_a_captured_graph(oracle):
    from diffqcqp_amd import ops
    for kind, N, B in (("qcqp", 8, 67), ("box", 20, 37)):
        d, _ = PC.problem(kind, N, B, "dense")
        t = {n: dev(v) for n, v in d.items()}
        ex = [t[n] for n in PC.EXTRAS[kind]]
        k = R.KIND[kind]
        g = col(C.inputs(kind, N, B, "dense")[1])
        xe = ops._polish(k, t["P"], t["q"], ex, ops._forward(k, t["P"], t["q"], ex, 1e-4, 1000), 8)
        eager = ops._newton_backward(k, t["P"], t["q"], ex, xe, g)
        ws = ops.make_workspace(torch.device("cuda"), B, k, 0, N)
        x = torch.zeros((B, N, 1), dtype=torch.float64, device="cuda")
        outs = [torch.zeros_like(a) for a in eager]
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            def chain():
                ops._forward(k, t["P"], t["q"], ex, 1e-4, 1000, out=x, workspace=ws)
                ops._polish(k, t["P"], t["q"], ex, x, 8, out=x)
                ops._newton_backward(k, t["P"], t["q"], ex, x, g, out=outs)
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
            assert torch.equal(a, b), kind
