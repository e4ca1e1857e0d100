"""-m gpu: the power-of-two equilibration on the device.  dqq_equilibrate_f64 and dqq_unscale_f64 against the numpy restatement
(tests/equil_ref.py) bit for bit, every buffer inside a poisoned arena (tests/footprint_arena.py); the scaled forwards of
ops.py against the three calls they are made of; the no-op on a batch that needs no scaling; parity with the oracle on the
figure fixture; the autograd classes under qcqp.set_default_scaling; a captured scaled forward."""
import os

import numpy as np
import pytest
import torch

import equil_ref as R
import footprint_arena as A
from conftest import make_problem

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
X_TOL = 1e-6            # tests/test_gpu_parity.py: the forward's tolerance against the oracle ...
MIN_ITERS_MATCH = 0.95  # ... and test_hip_reproduces_golden's rule for the iteration counts of a fixture
DENSE_N, DIAG_N, BS = R.DENSE_N, (2, 8, 64), (0, 1, 33, 257)
KERNEL_CASES = [(k, N, d) for k in R.KINDS for d, Ns in ((False, DENSE_N), (True, DIAG_N)) for N in Ns
                if not (k == "qcqp" and N % 2)]
EXTRA_NAMES = {"qp": (), "qcqp": ("l_n", "mu"), "box": ("l_min", "l_max"), "sbox": ("l_min", "l_max", "v")}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from diffqcqp_amd import build, ops as _ops, _capi
    build.build()
    _capi.lib()
    return _ops


def col(a):
    """(B,M) numpy -> (B,M,1) CPU tensor"""
    return torch.from_numpy(np.ascontiguousarray(a)).unsqueeze(-1)


def cuda_problem(P, q, extras, x0=None):
    return (torch.from_numpy(P).cuda(), col(q).cuda(), tuple(col(a).cuda() for a in extras),
            None if x0 is None else col(x0).cuda())


def npy(t):
    return t.detach().cpu().numpy()


def flat(t):
    a = npy(t)
    return a.reshape(a.shape[:-1]) if a.ndim == 3 and a.shape[-1] == 1 else a


def problems_per_workgroup(N, diag):
    """equil.hip: 4 waves of 64 / L problems on check.hip's lane mapping; DQQ_P_DIAG: 256 threads of two coordinates."""
    if diag:
        return max(1, 512 // N)
    need, L = (N + 1) // 2 if N % 2 == 0 else N, 1
    while L < need and L < 64:
        L *= 2
    return 4 * 64 // L


# ---- the two kernels against the restatement, inside a poisoned arena
@pytest.mark.parametrize("kind,N,diag", KERNEL_CASES)
def test_kernels_equal_the_restatement_bit_for_bit(ops, kind, N, diag):
    from diffqcqp_amd import _capi
    lib, k = _capi.lib(), R.KIND_ID[kind]
    layout = _capi.P_DIAG if diag else _capi.P_DENSE
    stream = torch.cuda.current_stream().cuda_stream
    g = problems_per_workgroup(N, diag)
    for B in BS:
        Bm = max(B, 1)   # B = 0: the pointers of a one-problem arena, which must come back untouched
        P, q, extras, x0 = R.make_batch(kind, Bm, N, 1000 * N + 10 * B + k, diag)
        r = np.random.default_rng(B + N)
        y = r.uniform(-1.0, 1.0, (Bm, N))
        want = R.equilibrate(kind, P, q, extras, x0, diag)
        pshape = (Bm, N) if diag else (Bm, N, N)
        eshape = (Bm, N // 2, 1) if kind == "qcqp" else (Bm, N, 1)
        names = EXTRA_NAMES[kind]
        specs = [("P", "in", A.F64, pshape, torch.from_numpy(P)), ("q", "in", A.F64, (Bm, N, 1), col(q))]
        specs += [(n, "in", A.F64, eshape, col(a)) for n, a in zip(names, extras)]
        specs += [("x0", "in", A.F64, (Bm, N, 1), col(x0)), ("y", "in", A.F64, (Bm, N, 1), col(y)),
                  ("e", "in", A.I32, (Bm, N), torch.from_numpy(want[4]))]
        specs += [("P_out", "out", A.F64, pshape, None), ("q_out", "out", A.F64, (Bm, N, 1), None)]
        specs += [(n + "_out", "out", A.F64, eshape, None) for n in names]
        specs += [("x0_out", "out", A.F64, (Bm, N, 1), None), ("e_out", "out", A.I32, (Bm, N), None),
                  ("x_out", "out", A.F64, (Bm, N, 1), None)]
        a = A.Arena(specs, g, "cuda", sliced=True)
        p = a.ptr
        ex_in = [p(n) for n in names] + [None] * (3 - len(names))
        ex_out = [p(n + "_out") for n in names] + [None] * (3 - len(names))
        rc = lib.dqq_equilibrate_f64(k, p("P"), p("q"), *ex_in, p("x0"), B, N, layout, p("P_out"), p("q_out"), *ex_out, p("x0_out"),
                                     p("e_out"), stream)
        assert rc == 0, (B, rc)
        rc = lib.dqq_unscale_f64(p("y"), p("e"), B, N, p("x_out"), stream)
        assert rc == 0, (B, rc)
        torch.cuda.synchronize()
        if B == 0:
            a.check_untouched()
            continue
        a.check_guards()
        a.check_inputs()
        outs = ["P_out", "q_out"] + [n + "_out" for n in names] + ["x0_out", "e_out", "x_out"]
        for n in outs:
            a.check_written(n)
        got = (npy(a.view("P_out")), flat(a.view("q_out")), tuple(flat(a.view(n + "_out")) for n in names), flat(a.view("x0_out")),
               npy(a.view("e_out")))
        assert R.same_problem(got, want) is None, (B, R.same_problem(got, want))
        assert R.same_bits(flat(a.view("x_out")), R.unscale(y, want[4])), B
        # the optional outputs left out: nothing of theirs is written, the rest keeps its bits
        a2 = A.Arena(specs, g, "cuda", sliced=False)
        p = a2.ptr
        ex_in = [p(n) for n in names] + [None] * (3 - len(names))
        rc = lib.dqq_equilibrate_f64(k, p("P"), p("q"), *ex_in, None, B, N, layout, p("P_out"), p("q_out"), None, None, None, None,
                                     p("e_out"), stream)
        assert rc == 0, (B, rc)
        torch.cuda.synchronize()
        a2.check_guards()
        a2.check_inputs()
        for n in [n + "_out" for n in names] + ["x0_out", "x_out"]:
            a2.check_pristine(n)
        assert R.same_bits(npy(a2.view("P_out")), want[0]) and R.same_bits(flat(a2.view("q_out")), want[1])
        assert np.array_equal(npy(a2.view("e_out")), want[4])


@pytest.mark.parametrize("kind", R.KINDS)
def test_ops_equilibrate_and_unscale(ops, kind):
    """The tensor-level entries: the restatement's bits, mu and v handed on as they are, unscale in place."""
    N, B = 8, 33
    P, q, extras, x0 = R.make_batch(kind, B, N, 4242 + R.KIND_ID[kind])
    want = R.equilibrate(kind, P, q, extras, x0)
    Pc, qc, exc, x0c = cuda_problem(P, q, extras, x0)
    Pt, qt, ext, x0t, e = ops.equilibrate(kind, Pc, qc, exc, x0c, layout=1)
    got = (npy(Pt), flat(qt), tuple(flat(t) for t in ext), flat(x0t), npy(e))
    assert R.same_problem(got, want) is None
    nscaled = {"qp": 0, "qcqp": 1, "box": 2, "sbox": 2}[kind]
    for given, back in zip(exc[nscaled:], ext[nscaled:]):
        assert back.data_ptr() == given.data_ptr()
    assert ops.equilibrate(kind, Pc, qc, exc, None, layout=1)[3] is None
    y = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (B, N, 1))).cuda()
    ref = R.unscale(flat(y), want[4])
    assert R.same_bits(flat(ops.unscale(y, e)), ref)
    assert ops.unscale(y, e, out=y) is y and R.same_bits(flat(y), ref)
    with pytest.raises(ValueError):   # an output over an input
        ops.equilibrate(kind, Pc, qc, exc, None, layout=1, out=(Pc, qt, ext[:nscaled], None, e))


# ---- the scaled forwards
def _forward(ops, kind, P, q, extras, eps=1e-7, max_iter=1000, x0=None, **kw):
    if x0 is not None:
        if kind == "qp":
            return ops.qp_forward_warm(P, q, x0, eps, max_iter, return_iters=True, **kw)
        if kind == "qcqp":
            return ops.qcqp_forward_warm(P, q, extras[0], extras[1], x0, eps, max_iter, return_iters=True, **kw)
        return ops.boxqp_forward_warm(P, q, extras[0], extras[1], x0, eps, max_iter, v=extras[2] if kind == "sbox" else None,
                                      return_iters=True, **kw)
    if kind == "qp":
        return ops.qp_forward(P, q, eps, max_iter, return_iters=True, **kw)
    if kind == "qcqp":
        return ops.qcqp_forward(P, q, extras[0], extras[1], eps, max_iter, return_iters=True, **kw)
    return ops.boxqp_forward(P, q, extras[0], extras[1], eps, max_iter, v=extras[2] if kind == "sbox" else None, return_iters=True, **kw)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("N", (4, 8, 20))
def test_scaled_forward_is_equilibrate_forward_unscale(ops, kind, N):
    B = 64
    P, q, extras, x0 = cuda_problem(*R.make_batch(kind, B, N, 500 + N, special=False, inf_bounds=False))
    for start in (None, x0):
        x, it = _forward(ops, kind, P, q, extras, x0=start, scaling="pow2")
        Pt, qt, ext, x0t, e = ops.equilibrate(kind, P, q, extras, start)
        assert int(e.min()) < 0 < int(e.max())
        y, ity = _forward(ops, kind, Pt, qt, ext, x0=x0t)
        assert torch.equal(it, ity)
        assert R.same_bits(npy(x), npy(ops.unscale(y, e)))
        assert bool(torch.isfinite(x).all())
    with pytest.raises(ValueError):
        _forward(ops, kind, P, q, extras, scaling="ruiz")
    with pytest.raises(ValueError):
        _forward(ops, kind, P, q, extras, scaling="pow2", cache=ops.diag_cache(q))


@pytest.mark.parametrize("kind", R.KINDS)
def test_scaling_is_a_no_op_where_every_exponent_is_zero(ops, kind):
    """P = S S'/N + 0.1 I brought to a unit diagonal (by a scaling of the test's own, not a power of two): every diagonal entry
    is 1 to rounding, every exponent 0, and the scaled route returns the unscaled route's bits."""
    B, N = 64, 8
    d = make_problem(kind, B, N, 321, "dense")
    s = 1.0 / torch.sqrt(torch.diagonal(d["P"], dim1=1, dim2=2))
    P = (d["P"] * s.unsqueeze(2) * s.unsqueeze(1)).contiguous().cuda()
    q = d["q"].cuda()
    extras = tuple(d[n].cuda() for n in EXTRA_NAMES[kind])
    diag = torch.diagonal(P, dim1=1, dim2=2)
    assert bool(((diag >= 0.5) & (diag < 2.0)).all())
    assert not bool(ops.equilibrate(kind, P, q, extras)[4].any())
    x0, it0 = _forward(ops, kind, P, q, extras)
    x1, it1 = _forward(ops, kind, P, q, extras, scaling="pow2")
    assert R.same_bits(npy(x1), npy(x0)) and torch.equal(it0, it1)
    x2, it2 = _forward(ops, kind, P, q, extras, scaling=None)
    assert R.same_bits(npy(x2), npy(x0)) and torch.equal(it0, it2)


@pytest.mark.parametrize("kind", ("qp", "qcqp"))
def test_scaled_route_follows_the_oracle_on_the_figure_fixture(oracle, ops, kind):
    from diffqcqp_amd import diagnostics
    d = np.load(os.path.join(GOLDEN, "qcqp_figure_n8.npz"))
    eps, mi = float(d["eps"]), int(d["max_iter"])
    P, q = d["P"], d["q"][:, :, 0]
    extras = (d["l_n"][:, :, 0], d["mu"][:, :, 0]) if kind == "qcqp" else ()
    Pt, qt, ext, _, e = R.equilibrate(kind, P, q, extras)
    if kind == "qp":
        yo, ito = oracle.qp_fwd_batch(Pt, qt[:, :, None], eps, mi, nthreads=8)
    else:
        yo, ito = oracle.qcqp_fwd_batch(Pt, qt[:, :, None], ext[0][:, :, None], ext[1][:, :, None], eps, mi, nthreads=8)
    xo = R.unscale(yo[:, :, 0], e)
    Pc, qc, exc, _ = cuda_problem(P, q, extras)
    xh, ith = _forward(ops, kind, Pc, qc, exc, eps=eps, max_iter=mi, scaling="pow2")
    diff = np.abs(flat(xh) - xo)
    print("%s: max |x - D y_oracle| = %.3e, iteration counts equal on %d of %d, max %d (oracle %d)"
          % (kind, diff.max(), (npy(ith) == ito).sum(), ito.size, int(ith.max()), ito.max()))
    assert diff.max() <= X_TOL
    assert (npy(ith) == ito).mean() >= MIN_ITERS_MATCH
    check = diagnostics.check_qcqp if kind == "qcqp" else diagnostics.check_qp
    info = check(Pc, qc, *exc, xh, iters=ith, max_iter=mi)
    assert not bool(info.status.any()), "status on the caller's problem: %s" % npy(info.status)
    solve = diagnostics.solve_qcqp_checked if kind == "qcqp" else diagnostics.solve_qp_checked
    xs, info2 = solve(Pc, qc, *exc, eps, mi, scaling="pow2")
    assert R.same_bits(npy(xs), npy(xh)) and R.same_bits(npy(info2.natural), npy(info.natural)) and not bool(info2.status.any())


# ---- the autograd classes
def _classes():
    from diffqcqp_amd import qcqp
    return {"qp": qcqp.QPFn2, "qcqp": qcqp.QCQPFn2, "box": qcqp.BoxQPFn2, "sbox": qcqp.SignedBoxQPDiffFn2}


def _backward(ops, kind, P, q, extras, x, g):
    if kind == "qp":
        return ops.qp_backward(P, q, x, g)
    if kind == "qcqp":
        return ops.qcqp_backward(P, q, extras[0], extras[1], x, g)
    return ops.boxqp_backward(P, q, extras[0], extras[1], x, g, v=extras[2] if kind == "sbox" else None)


@pytest.mark.parametrize("kind", R.KINDS)
def test_autograd_classes_under_the_default_scaling(ops, kind):
    from diffqcqp_amd import qcqp
    B, N = 64, 8
    P, q, extras, _ = cuda_problem(*R.make_batch(kind, B, N, 900 + R.KIND_ID[kind], special=False, inf_bounds=False))
    g = torch.from_numpy(np.random.default_rng(3).standard_normal((B, N, 1))).cuda()
    Fn = _classes()[kind]
    ngrad = 2 if kind == "qp" else 4

    def run():
        ins = [t.clone().requires_grad_(True) for t in (P, q) + extras]
        x = Fn.apply(*ins, None, 1e-7, 1000)
        x.backward(g)
        return x.detach(), [t.grad for t in ins[:ngrad]]

    assert qcqp.get_default_scaling() is None
    x_plain, _ = run()
    assert R.same_bits(npy(x_plain), npy(_forward(ops, kind, P, q, extras)[0]))       # the default: today's path and bits
    with pytest.raises(ValueError):
        qcqp.set_default_scaling("ruiz")
    assert qcqp.set_default_scaling("pow2") is None
    try:
        assert qcqp.get_default_scaling() == "pow2"
        x, grads = run()
    finally:
        assert qcqp.set_default_scaling(None) == "pow2"
    assert R.same_bits(npy(x), npy(_forward(ops, kind, P, q, extras, scaling="pow2")[0]))
    want = _backward(ops, kind, P, q, extras, x, g)       # on the caller's tensors and the unscaled x
    for a, b in zip(grads, want[:ngrad]):
        assert R.same_bits(npy(a), npy(b))


# ---- a captured scaled forward
@pytest.mark.parametrize("kind,N,B,structure", [("qp", 8, 4096, "diag"), ("qcqp", 8, 2051, "mixed"), ("box", 20, 64, "dense")])
def test_scaled_forward_captured_into_a_graph_and_replayed(ops, kind, N, B, structure):
    def data(seed):
        d = make_problem(kind, B, N, seed, structure)
        s = torch.from_numpy(np.ldexp(1.0, np.random.default_rng(seed).integers(-20, 21, (B, N))))
        d["P"] = (d["P"] * s.unsqueeze(2) * s.unsqueeze(1)).contiguous()
        d["q"] = d["q"] * s.unsqueeze(2)
        for n in ("l_min", "l_max"):
            if n in d:
                d[n] = d[n] / s.unsqueeze(2)
        return d
    d1, d2 = data(8100 + N), data(8200 + N)
    keys = ["P", "q"] + list(EXTRA_NAMES[kind])
    t = {k: d1[k].cuda().clone() for k in keys}
    t["x"] = torch.empty(B, N, 1, device="cuda", dtype=torch.float64)

    def run():
        extras = tuple(t[n] for n in EXTRA_NAMES[kind])
        kw = dict(scaling="pow2", out=t["x"])
        if kind == "qp":
            ops.qp_forward(t["P"], t["q"], 1e-7, 1000, **kw)
        elif kind == "qcqp":
            ops.qcqp_forward(t["P"], t["q"], *extras, 1e-7, 1000, **kw)
        else:
            ops.boxqp_forward(t["P"], t["q"], *extras, 1e-7, 1000, **kw)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):          # warm-up on the capture stream: the workspace
        run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager1 = t["x"].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        run()
    t["x"].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(t["x"], eager1), "replay differs from the eager call"
    for k in keys:                      # new inputs in the captured buffers
        t[k].copy_(d2[k])
    graph.replay()
    torch.cuda.synchronize()
    replayed = t["x"].clone()
    assert not torch.equal(replayed, eager1)
    with torch.cuda.stream(s):
        run()
    torch.cuda.synchronize()
    assert torch.equal(t["x"], replayed), "replay differs from the eager call on the new inputs"
    assert bool(torch.isfinite(replayed).all())
