"""-m gpu: what the Python layer hands to the C ABI, argument by argument.

`_capi._lib` is replaced by a proxy that forwards every dqq_* call to the real library and keeps (symbol, args).  Every public
`ops` function and every autograd Function of qcqp.py is called once per variant, and each recorded compute call is held against
the parameter order of include/diffqcqp_hip.h, written down below as literal tuples of names: the symbol, the data_ptr() of the
tensor that belongs at each pointer position, None exactly where an optional pointer was not asked for, the scalars (distinctive,
non-default values), the workspace and the stream.  No kernel result is compared: the parity tests do that."""
import pytest
import torch

from conftest import make_problem

pytestmark = pytest.mark.gpu

_FWD_TAIL = ("B", "N", "eps", "mu_prox", "max_iter", "adaptive_rho", "p_layout", "iters", "pdiag_out", "diag_flags_out",
             "workspace", "workspace_bytes", "stream")
_BWD_TAIL = ("B", "N", "epsilon", "p_layout", "ir_steps", "pdiag", "diag_flags")
_WS = ("workspace", "workspace_bytes", "stream")
PARAMS = {   # include/diffqcqp_hip.h, in its order
    "dqq_qp_fwd_f64": ("P", "q", "x") + _FWD_TAIL,
    "dqq_qcqp_fwd_f64": ("P", "q", "l_n", "mu", "x") + _FWD_TAIL,
    "dqq_boxqp_fwd_f64": ("P", "q", "l_min", "l_max", "x") + _FWD_TAIL,
    "dqq_signedboxqp_fwd_f64": ("P", "q", "l_min", "l_max", "v", "x") + _FWD_TAIL,
    "dqq_fwd_warm_f64": ("kind", "P", "q", "a", "b", "c", "x0", "x") + _FWD_TAIL,
    "dqq_qp_bwd_f64": ("P", "q", "x", "grad_x", "grad_P", "grad_q") + _BWD_TAIL + ("report",) + _WS,
    "dqq_qcqp_bwd_f64": ("P", "q", "l_n", "mu", "x", "grad_x", "grad_P", "grad_q", "grad_l_n", "grad_mu", "gamma", "dgamma")
                        + _BWD_TAIL + ("report",) + _WS,
    "dqq_boxqp_bwd_f64": ("P", "q", "l_min", "l_max", "x", "grad_x", "grad_P", "grad_q", "grad_l_min", "grad_l_max", "gamma",
                          "dgamma") + _BWD_TAIL + _WS,
    "dqq_signedboxqp_bwd_f64": ("P", "q", "l_min", "l_max", "v", "x", "grad_x", "grad_P", "grad_q", "grad_l_min", "grad_l_max",
                                "gamma", "dgamma") + _BWD_TAIL + _WS,
    "dqq_check_f64": ("kind", "P", "q", "a", "b", "c", "x", "iters", "max_iter", "B", "N", "p_layout", "resid", "status", "counts",
                      "stream"),
}
KIND = {"qp": 0, "qcqp": 1, "box": 2, "sbox": 3}
EXTRAS = {"qp": (), "qcqp": ("l_n", "mu"), "box": ("l_min", "l_max"), "sbox": ("l_min", "l_max", "v")}
FWD = {"qp": "dqq_qp_fwd_f64", "qcqp": "dqq_qcqp_fwd_f64", "box": "dqq_boxqp_fwd_f64", "sbox": "dqq_signedboxqp_fwd_f64"}
BWD = {"qp": "dqq_qp_bwd_f64", "qcqp": "dqq_qcqp_bwd_f64", "box": "dqq_boxqp_bwd_f64", "sbox": "dqq_signedboxqp_bwd_f64"}
GRADS = {"qp": ("grad_P", "grad_q"), "qcqp": ("grad_P", "grad_q", "grad_l_n", "grad_mu"),
         "box": ("grad_P", "grad_q", "grad_l_min", "grad_l_max"), "sbox": ("grad_P", "grad_q", "grad_l_min", "grad_l_max")}
AUTO, DENSE, DIAG = 0, 1, 2
EPS, MU_PROX, MAX_ITER, EPSILON = 3e-6, 2e-7, 37, 3e-10
SOME = object()   # a pointer that must be there, whose address the caller of the Function never sees


class Recorder:
    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("dqq_"):
            return fn

        def call(*args):
            self.calls.append((name, args))
            return fn(*args)
        return call

    def take(self):
        """The compute calls since the last take (the pure queries -- sizes, hint flags, device pointers -- are not compared)."""
        got = [(s, a) for s, a in self.calls if s in PARAMS]
        self.calls = []
        return got


@pytest.fixture(scope="module")
def rec():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from diffqcqp_amd import build, _capi
    build.build()
    real = _capi.lib()
    hints_were_on = _capi._hints_on
    _capi.enable_feedback(True)
    proxy = Recorder(real)
    _capi._lib = proxy
    try:
        yield proxy
    finally:
        _capi._lib = real
        _capi.enable_feedback(hints_were_on)


def _gpu(kind, B, N, seed):
    return {k: v.cuda() for k, v in make_problem(kind, B, N, seed, "mixed").items()}


def _held(call, symbol, kind, pas, want, workspace=None, ws_kind=None):
    """One recorded call against `want` (parameter name -> tensor, None, SOME or scalar; every parameter of the symbol but the
    workspace triple, which is checked against the cache entry of the current stream or the caller's `workspace`)."""
    from diffqcqp_amd import ops
    got_symbol, args = call
    assert got_symbol == symbol
    names = PARAMS[symbol]
    assert len(args) == len(names), symbol
    got = dict(zip(names, args))
    stream = ops._raw_stream(0)
    assert got.pop("stream") == stream, symbol
    if "workspace" in names:
        ws = workspace if workspace is not None else ops._workspaces[(0, stream)]
        need = ops.workspace_bytes(want["B"], KIND[kind] if ws_kind is None else ws_kind, pas, want["N"], want["p_layout"])
        assert got.pop("workspace") == ws.data_ptr() and got.pop("workspace_bytes") == ws.numel() * 4 >= need, symbol
    assert set(got) == set(want), (symbol, set(got) ^ set(want))
    for name, w in want.items():
        g = got[name]
        if w is None:
            assert g is None or g == 0, "%s: %s should be NULL" % (symbol, name)
        elif w is SOME:
            assert g, "%s: %s is missing" % (symbol, name)
        elif isinstance(w, torch.Tensor):
            assert g == w.data_ptr(), "%s: %s is not the tensor that belongs there" % (symbol, name)
        else:
            assert g == w and type(g) is type(w), "%s: %s = %r, expected %r" % (symbol, name, g, w)


def _fwd_want(kind, g, x, layout, warm, iters=None, cache=None, adaptive=1, **over):
    B, N = g["q"].shape[:2]
    want = dict(P=g["P"], q=g["q"], x=x, B=B, N=N, eps=EPS, mu_prox=MU_PROX, max_iter=MAX_ITER, adaptive_rho=adaptive,
                p_layout=layout, iters=iters, pdiag_out=cache and cache[0], diag_flags_out=cache and cache[1])
    if warm is None:
        want.update({n: g[n] for n in EXTRAS[kind]})
    else:
        ex = [g[n] for n in EXTRAS[kind]] + [None] * 3
        want.update(kind=KIND[kind], a=ex[0], b=ex[1], c=ex[2], x0=warm)
    want.update(over)
    return want


def _bwd_want(kind, g, x, grad_x, grads, layout, steps=None, cache=None, duals=None, report=None, epsilon=EPSILON):
    B, N = g["q"].shape[:2]
    want = dict(P=g["P"], q=g["q"], x=x, grad_x=grad_x, B=B, N=N, epsilon=epsilon, p_layout=layout, ir_steps=steps,
                pdiag=cache and cache[0], diag_flags=cache and cache[1])
    want.update({n: g[n] for n in EXTRAS[kind]})
    want.update(zip(GRADS[kind], grads))
    if kind != "qp":
        want.update(gamma=duals and duals[0], dgamma=duals and duals[1])
    if kind in ("qp", "qcqp"):
        want["report"] = report
    return want


def _ops_forward(ops, kind, g, x0=None, **kw):
    common = dict(mu_prox=MU_PROX, **kw)
    if kind == "qp":
        return (ops.qp_forward(g["P"], g["q"], EPS, MAX_ITER, **common) if x0 is None else
                ops.qp_forward_warm(g["P"], g["q"], x0, EPS, MAX_ITER, **common))
    if kind == "qcqp":
        return (ops.qcqp_forward(g["P"], g["q"], g["l_n"], g["mu"], EPS, MAX_ITER, **common) if x0 is None else
                ops.qcqp_forward_warm(g["P"], g["q"], g["l_n"], g["mu"], x0, EPS, MAX_ITER, **common))
    if x0 is None:
        return ops.boxqp_forward(g["P"], g["q"], g["l_min"], g["l_max"], EPS, MAX_ITER, v=g.get("v"), **common)
    return ops.boxqp_forward_warm(g["P"], g["q"], g["l_min"], g["l_max"], x0, EPS, MAX_ITER, v=g.get("v"), **common)


def _ops_backward(ops, kind, g, x, **kw):
    if kind == "qp":
        return ops.qp_backward(g["P"], g["q"], x, g["grad_x"], epsilon=EPSILON, **kw)
    if kind == "qcqp":
        return ops.qcqp_backward(g["P"], g["q"], g["l_n"], g["mu"], x, g["grad_x"], epsilon=EPSILON, **kw)
    return ops.boxqp_backward(g["P"], g["q"], g["l_min"], g["l_max"], x, g["grad_x"], epsilon=EPSILON, v=g.get("v"), **kw)


def _report(kind, N, B):
    """The report word the QP / QCQP backwards of an N <= 8 DQQ_P_AUTO call carry (the hint protocol of _capi.py)."""
    from diffqcqp_amd import _capi
    address = _capi.hint(KIND[kind], 1, N, B, 0)[1]
    assert address
    return address


@pytest.mark.parametrize("kind", ("qp", "qcqp", "box", "sbox"))
def test_ops_calls(rec, kind):
    from diffqcqp_amd import ops
    B, N = 5, 4
    g = _gpu(kind, B, N, 31 + KIND[kind])
    x0 = 0.25 * g["grad_x"]
    rec.take()
    # forwards, cold and warm: DQQ_P_AUTO with the verified-diagonal buffers and the iteration counts, DQQ_P_DENSE without
    for warm in (None, x0):
        symbol = FWD[kind] if warm is None else "dqq_fwd_warm_f64"
        cache = ops.diag_cache(g["q"])
        x, iters = _ops_forward(ops, kind, g, warm, adaptive_rho=False, layout=AUTO, cache=cache, return_iters=True)
        assert x.shape == (B, N, 1) and iters.shape == (B,) and iters.dtype is torch.int32
        (call,) = rec.take()
        _held(call, symbol, kind, 0, _fwd_want(kind, g, x, AUTO, warm, iters, cache, adaptive=0))
        out = torch.empty(B, N, 1, dtype=torch.float64, device="cuda")
        ws = ops.make_workspace(g["q"].device, B, KIND[kind], 0, N, DENSE)
        x = _ops_forward(ops, kind, g, warm, layout=DENSE, out=out, workspace=ws)
        assert x is out
        (call,) = rec.take()
        _held(call, symbol, kind, 0, _fwd_want(kind, g, out, DENSE, warm), workspace=ws)
    # backwards: DQQ_P_AUTO with the forward's buffers, every gradient and the step counts; DQQ_P_DENSE with outputs left out
    cache = ops.diag_cache(g["q"])
    x = _ops_forward(ops, kind, g, layout=AUTO, cache=cache)
    rec.take()
    shape = (B, N // 2, 1) if kind == "qcqp" else (B, 2 * N)
    duals = None if kind == "qp" else tuple(torch.empty(shape, dtype=torch.float64, device="cuda") for _ in range(2))
    kw = {} if kind == "qp" else {"duals": duals}
    *grads, steps = _ops_backward(ops, kind, g, x, layout=AUTO, cache=cache, return_steps=True, **kw)
    assert steps.shape == ((B,) if kind in ("qp", "qcqp") else (B, 2)) and steps.dtype is torch.int32
    assert [tuple(t.shape) for t in grads] == [(B, N, N), (B, N, 1)] + ([] if kind == "qp" else [tuple(g[EXTRAS[kind][0]].shape)] * 2)
    report = _report(kind, N, B) if kind in ("qp", "qcqp") else None
    (call,) = rec.take()
    ws_kind = 2 if kind == "sbox" else None
    _held(call, BWD[kind], kind, 1, _bwd_want(kind, g, x, g["grad_x"], grads, AUTO, steps, cache, duals, report), ws_kind=ws_kind)
    need = {"need_P": False, "need_q": True} if kind == "qp" else {"need": (True, False, False, True)}
    grads = _ops_backward(ops, kind, g, x, layout=DENSE, **need)
    assert [t is None for t in grads] == ([True, False] if kind == "qp" else [False, True, True, False])
    (call,) = rec.take()
    _held(call, BWD[kind], kind, 1, _bwd_want(kind, g, x, g["grad_x"], grads, DENSE), ws_kind=ws_kind)
    outs = tuple(torch.empty_like(t) for t in (g["P"], g["q"]) + tuple(g[n] for n in EXTRAS[kind][:2]))
    got = _ops_backward(ops, kind, g, x, layout=DENSE, out=outs)
    assert all(a is b for a, b in zip(got, outs))
    (call,) = rec.take()
    _held(call, BWD[kind], kind, 1, _bwd_want(kind, g, x, g["grad_x"], outs, DENSE), ws_kind=ws_kind)
    # the solution check: with the forward's counts and into the caller's buffers, then without either
    x, iters = _ops_forward(ops, kind, g, layout=AUTO, return_iters=True)
    rec.take()
    extras = tuple(g[n] for n in EXTRAS[kind])
    ex = list(extras) + [None] * 3
    bufs = (torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, 4, dtype=torch.float64, device="cuda"),
            torch.empty(3, dtype=torch.int64, device="cuda"))
    for name, its, mi, out in ((kind, iters, MAX_ITER, bufs), (KIND[kind], None, None, None)):
        status, resid, counts = ops.solution_check(name, g["P"], g["q"], extras, x, iters=its, max_iter=mi, layout=DENSE, out=out)
        assert out is None or (status is out[0] and resid is out[1] and counts is out[2])
        (call,) = rec.take()
        _held(call, "dqq_check_f64", kind, 0, dict(kind=KIND[kind], P=g["P"], q=g["q"], a=ex[0], b=ex[1], c=ex[2], x=x, iters=its,
                                                   max_iter=mi or 0, B=B, N=N, p_layout=DENSE, resid=resid, status=status,
                                                   counts=counts))
    torch.cuda.synchronize()


def test_compact_diagonal_scratch_and_the_signed_box_workspace(rec):
    from diffqcqp_amd import ops
    rec.take()
    # DQQ_P_DIAG: P is the compact (B,N) diagonal
    g = _gpu("qp", 5, 4, 77)
    g["P"] = torch.diagonal(g["P"], dim1=1, dim2=2).contiguous()
    x = ops.qp_forward(g["P"], g["q"], EPS, MAX_ITER, MU_PROX, layout=DIAG)
    (call,) = rec.take()
    _held(call, "dqq_qp_fwd_f64", "qp", 0, _fwd_want("qp", g, x, DIAG, None))
    gP, gq = ops.qp_backward(g["P"], g["q"], x, g["grad_x"], layout=DIAG, epsilon=EPSILON)
    assert gP.shape == (5, 4)
    (call,) = rec.take()
    _held(call, "dqq_qp_bwd_f64", "qp", 1, _bwd_want("qp", g, x, g["grad_x"], (gP, gq), DIAG))
    # N = 70: the global-memory kernel, scratch behind the work-list
    g = _gpu("qp", 3, 70, 78)
    assert rec._real.dqq_scratch_bytes(0, 0, 70, 3, 0) > 0
    x = ops.qp_forward(g["P"], g["q"], EPS, MAX_ITER, MU_PROX)
    (call,) = rec.take()
    _held(call, "dqq_qp_fwd_f64", "qp", 0, _fwd_want("qp", g, x, AUTO, None))
    assert call[1][PARAMS["dqq_qp_fwd_f64"].index("workspace_bytes")] >= ops.workspace_bytes(3, 0, 0, 70) > ops.workspace_bytes(3, 0, 0, 8)
    # the signed box backward beyond the wave kernel, on a stream of its own (a workspace made for this call): sized as the
    # box QP's, dqq_scratch_bytes(2, 1, ...) -- the library's answer for kind 3 is 0
    B, N = 3, 22
    g = _gpu("sbox", B, N, 79)
    assert ops.workspace_bytes(B, 2, 1, N) > ops.workspace_bytes(B, 3, 1, N)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        x = ops.boxqp_forward(g["P"], g["q"], g["l_min"], g["l_max"], EPS, MAX_ITER, v=g["v"], mu_prox=MU_PROX)
        rec.take()
        grads = ops.boxqp_backward(g["P"], g["q"], g["l_min"], g["l_max"], x, g["grad_x"], v=g["v"], epsilon=EPSILON)
        (call,) = rec.take()
        _held(call, "dqq_signedboxqp_bwd_f64", "sbox", 1, _bwd_want("sbox", g, x, g["grad_x"], grads, AUTO), ws_kind=2)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


FUNCTIONS = (   # class, kind, warm, has a backward
    ("QPFn2", "qp", False, True), ("QCQPFn2", "qcqp", False, True), ("BoxQPFn2", "box", False, True),
    ("SignedBoxQPFn2", "sbox", False, False), ("SignedBoxQPDiffFn2", "sbox", False, True),
    ("QPWarmFn2", "qp", True, True), ("QCQPWarmFn2", "qcqp", True, True), ("BoxQPWarmFn2", "box", True, True),
    ("SignedBoxQPWarmFn2", "sbox", True, True))


@pytest.mark.parametrize("name,kind,warm,diff", FUNCTIONS, ids=[f[0] for f in FUNCTIONS])
def test_function_calls(rec, name, kind, warm, diff):
    from diffqcqp_amd import qcqp
    assert qcqp.get_default_layout() == "auto"
    B, N = 5, 4
    g = _gpu(kind, B, N, 51 + KIND[kind])
    # every input but the last extra asks for a gradient (v never gets one; the QCQP's mu is left out here)
    grad_names = ("P", "q") + EXTRAS[kind][:1]
    ins = [g[n].clone().requires_grad_(n in grad_names) for n in ("P", "q") + EXTRAS[kind]]
    gi = dict(zip(("P", "q") + EXTRAS[kind], ins))
    w = 0.25 * g["grad_x"]
    rec.take()
    x = getattr(qcqp, name).apply(*ins, w, EPS, MAX_ITER, MU_PROX)
    (call,) = rec.take()
    symbol = "dqq_fwd_warm_f64" if warm else FWD[kind]
    cache = (SOME, SOME) if diff else None       # SignedBoxQPFn2 has no backward to hand the diagonal to
    _held(call, symbol, kind, 0, _fwd_want(kind, gi, x, AUTO, w if warm else None, None, cache))
    if not diff:
        with pytest.raises(NotImplementedError):
            x.sum().backward()
        return
    names = PARAMS[symbol]
    saved = (call[1][names.index("pdiag_out")], call[1][names.index("diag_flags_out")])
    x.sum().backward()
    (call,) = rec.take()
    grads = [SOME if n in grad_names else None for n in ("P", "q") + EXTRAS[kind][:2]]
    want = _bwd_want(kind, gi, x, SOME, grads, AUTO, report=_report(kind, N, B) if kind in ("qp", "qcqp") else None,
                     epsilon=1e-10)
    want.update(pdiag=SOME, diag_flags=SOME)
    _held(call, BWD[kind], kind, 1, want, ws_kind=2 if kind == "sbox" else None)
    got = dict(zip(PARAMS[BWD[kind]], call[1]))
    assert (got["pdiag"], got["diag_flags"]) == saved      # the buffers the forward filled
    for t, n in zip(ins, ("P", "q") + EXTRAS[kind]):
        assert (t.grad is not None) == (n in grad_names)
    torch.cuda.synchronize()
