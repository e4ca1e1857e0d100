"""Drop-in for the reference's `qcqp.py`: the `QPFn2` and `QCQPFn2`
`torch.autograd.Function`s with the same forward/backward signatures, argument
order, output shapes and `None` padding (reference qcqp.py:22-52, 141-181), but
each pass is ONE launch of a hand-written HIP kernel over the whole batch
instead of a Python loop over per-problem C++ calls.

    from diffqcqp_amd.qcqp import QPFn2, QCQPFn2
    x = QPFn2.apply(P, q, warm_start, eps, max_iter)          # (B,N,1)
    x = QCQPFn2.apply(P, q, l_n, mu, warm_start, eps, max_iter)
    x = BoxQPFn2.apply(P, q, l_min, l_max, warm_start, eps, max_iter)            # qcqp.py:54-94
    x = SignedBoxQPFn2.apply(P, q, l_min, l_max, v, warm_start, eps, max_iter)   # qcqp.py:97-137, forward only
    x = SignedBoxQPDiffFn2.apply(P, q, l_min, l_max, v, warm_start, eps, max_iter)   # the same, with a backward
    x = QPWarmFn2.apply(P, q, x_prev, eps, max_iter)          # an extension: QPWarmFn2, QCQPWarmFn2, BoxQPWarmFn2 and
                                                              # SignedBoxQPWarmFn2 START from warm_start (end of this file)

Behaviour kept from the reference:
  * importing this module sets torch's default dtype to float64 (qcqp.py:13);
  * `warm_start` is accepted and has no effect on the result (the reference
    overwrites it before reading it, Solver.cpp:70/80, 529/539); it gets no grad;
  * backward honours ctx.needs_input_grad and returns 6 / 8 (SignedBoxQPDiffFn2: 9) values.
An extension: every class with a backward also has a `jvp` (torch.autograd.forward_ad, torch.func.jvp; one launch of
dqq_jvp_f64), and the classes are written as forward + setup_context, so torch.func's transforms accept them.
Differences: tensors on the GPU are used in place and results stay there; CPU
tensors are staged through cuda:0 and the result is returned on the CPU.  There
is no CPU solver in this package: without a GPU and the HIP library the calls
raise.
"""
import torch
from torch.autograd import Function

from . import ops

torch.set_default_dtype(torch.double)


_FAST_N = (2, 4, 8, 16, 32, 64)

# How the Functions below hand P to the C ABI (include/diffqcqp_hip.h: p_layout).  "auto" (default): every tile's
# off-diagonals are verified in-kernel, diagonal tiles take the fast path, the others the general kernels -- nothing is
# assumed.  "dense": straight to the general kernels, for callers who know their P is dense (a Delassus matrix): saves
# the verifying pass.  A module-level default because the reference's signatures (qcqp.py:24, 144) have no slot for it.
# "auto_expect_dense": "auto" with the hint flag DQQ_F_EXPECT_DENSE given by the CALLER instead of derived from a report word --
# still verified in-kernel, bit-identical results on any input (a wrong expectation costs time only), but an ARGUMENT: it
# holds on a first call and inside a captured HIP graph, where the report word's hints do not.
_LAYOUTS = {"auto": ops._capi.P_AUTO, "dense": ops._capi.P_DENSE,
            "auto_expect_dense": ops._capi.P_AUTO | ops._capi.F_EXPECT_DENSE}
_default_layout = ops._capi.P_AUTO


def set_default_layout(layout):
    """layout: "auto", "dense" or "auto_expect_dense".  Returns the previous setting (as a string)."""
    global _default_layout
    prev = [k for k, v in _LAYOUTS.items() if v == _default_layout][0]
    if layout not in _LAYOUTS:
        raise ValueError("layout must be one of %s" % sorted(_LAYOUTS))
    _default_layout = _LAYOUTS[layout]
    return prev


def get_default_layout():
    return [k for k, v in _LAYOUTS.items() if v == _default_layout][0]


# Newton steps every forward below takes on its solution before it returns (ops._polish: dqq_polish_f64, each step kept only if
# it lowers the natural residual).  0 (default): none, the forwards' bits as they always were.  A module-level default for the
# reason given above: the reference's signatures have no slot for it.
_default_polish = 0


def set_default_polish(steps):
    """steps >= 0: every *Fn2 forward polishes its solution with up to that many Newton steps before it returns and saves it;
    the backward and the JVP then differentiate at the polished point.  Returns the previous setting."""
    global _default_polish
    prev = _default_polish
    if int(steps) != steps or steps < 0:
        raise ValueError("steps must be a non-negative integer")
    _default_polish = int(steps)
    return prev


def get_default_polish():
    return _default_polish


# How often a step of that polish may be halved before it is given up (ops._polish: max_halvings, dqq_polish_ls_f64).  0
# (default): full steps only, every call what it was.  With a value such as 8 the polish also repairs a forward that stopped
# outside the Newton basin (a small max_iter).  Read when the polish runs; a launch argument, so a captured graph replays the
# value it was captured with.
_default_polish_halvings = 0


def set_default_polish_halvings(k):
    """k: an integer in 0 .. 60.  Returns the previous setting."""
    global _default_polish_halvings
    prev = _default_polish_halvings
    _default_polish_halvings = ops._halvings(k)
    return prev


def get_default_polish_halvings():
    return _default_polish_halvings


# Which derivative the backward and the jvp of every differentiable Function below compute.  "reference" (default): the
# reference's regularised KKT systems (ops._backward / ops._jvp), every call what it always was.  "newton": the exact derivative
# from the polish's Jacobian at the saved solution (ops._newton_backward / ops._newton_jvp: no epsilon, no refinement, no hints,
# no diagonal cache; both modes each other's transpose to rounding).  With set_default_polish(k): solve, polish, differentiate
# exactly.  Read when the derivative runs, not when the forward did.
_DERIVATIVES = ("reference", "newton")
_default_derivative = "reference"


def set_default_derivative(which):
    """which: "reference" or "newton".  Returns the previous setting."""
    global _default_derivative
    prev = _default_derivative
    if which not in _DERIVATIVES:
        raise ValueError("derivative must be one of %s" % (_DERIVATIVES,))
    _default_derivative = which
    return prev


def get_default_derivative():
    return _default_derivative


# Whether the polish and the "newton" derivatives of the box kinds (BoxQPFn2, SignedBoxQPDiffFn2 and their warm twins) take
# one-sided boxes: l_min = -inf / l_max = +inf per coordinate, which the forwards accept (DQQ_F_INFINITE_BOUNDS,
# include/diffqcqp_hip.h).  False (default): every call what it was -- such a problem is left unpolished (status 2) and its
# "newton" gradients are NaN.  True: it is polished and differentiated like any other; the gradient of an infinite bound is
# +0.0.  Read when the polish / the derivative runs.  The QP and the QCQP have no bounds: nothing changes for them.
_default_infinite_bounds = False


def set_default_infinite_bounds(flag):
    """flag: bool.  Returns the previous setting."""
    global _default_infinite_bounds
    prev = _default_infinite_bounds
    if not isinstance(flag, (bool, int)) or flag not in (0, 1):
        raise ValueError("flag must be a bool")
    _default_infinite_bounds = bool(flag)
    return prev


def get_default_infinite_bounds():
    return _default_infinite_bounds


# The proximal weight of the polish (set_default_polish) and of the "newton" derivatives (set_default_derivative): `reg` of
# ops._polish / ops._newton_backward / ops._newton_jvp, M_reg = (I - D) + D (P + reg I).  0.0 (default): every call what it was
# -- on a P that is only positive semidefinite (redundant contacts) a singular free block then ends in NaN gradients or
# numbers of size 1e16.  A value such as 1e-7 (the weight of the reference-order derivatives' Tikhonov iterate) makes both finite:
# the derivative of one proximal-point step at the saved solution.  Read when the polish / the derivative runs; a launch
# argument, so a captured graph replays the value it was captured with.
_default_newton_reg = 0.0


def set_default_newton_reg(value):
    """value: a finite float >= 0.  Returns the previous setting."""
    global _default_newton_reg
    prev = _default_newton_reg
    _default_newton_reg = ops._reg(value)
    return prev


def get_default_newton_reg():
    return _default_newton_reg


# Smoothed ("central path") derivatives (ops._polish / ops._newton_backward / ops._newton_jvp: kappa; csrc/smooth_core.h).  With
# kappa > 0 under set_default_derivative("newton") the forward output of every class is what it was; the backward and the jvp
# first run the smoothed polish from the saved solution -- `steps` Newton steps, each halved up to `max_halvings` times, with
# set_default_newton_reg's weight -- and differentiate at the point it returns, with the same kappa: a bound or radius that is not
# active gets a gradient that is not zero.  kappa = 0 (default): every call what it was.  kappa > 0 with the "reference"
# derivative is refused where a class is applied; one-sided boxes (set_default_infinite_bounds) are refused by the ops.  Read
# when the derivative runs; launch arguments, so a captured graph replays the values it was captured with.
_default_smoothing = (0.0, 20, 8)


def set_default_smoothing(kappa, steps=20, max_halvings=8):
    """kappa: a finite float >= 0; steps: an int >= 0; max_halvings: 0 .. 60.  Returns the previous (kappa, steps, max_halvings)."""
    global _default_smoothing
    prev = _default_smoothing
    if int(steps) != steps or steps < 0:
        raise ValueError("steps must be an integer >= 0, got %r" % (steps,))
    _default_smoothing = (ops._kappa(kappa), int(steps), ops._halvings(max_halvings))
    return prev


def get_default_smoothing():
    return _default_smoothing


def _smoothed(cls, saved, n, l, layout):
    """-> (the point the derivative is taken at, kappa): the saved solution and 0.0, or the smoothed polish's point from it."""
    kappa, steps, halvings = _default_smoothing
    if not kappa:
        return l, 0.0
    return ops._polish(cls.kind, saved[0], saved[1], saved[2:n], l, steps, layout, infinite_bounds=_default_infinite_bounds,
                       reg=_default_newton_reg, max_halvings=halvings, kappa=kappa), kappa


# Whether every forward below solves the problem as it is handed over (None, the default: every call what it was) or
# equilibrated: "pow2" runs ops.equilibrate, the unchanged forward on the scaled problem and ops.unscale, on one stream
# (include/diffqcqp_hip.h: dqq_equilibrate_f64; the factors are powers of two, so the scaled problem is the caller's in other
# units).  eps then bounds the scaled problem's residuals.  What is saved for the backward and the jvp are the caller's tensors
# and the unscaled solution: no derivative, polish or Newton code knows of the scaling.  The forward fills no diagonal cache then
# (it would hold the scaled diagonal): the backward reads P itself, which gives the same bits.  Read when the forward runs.
_default_scaling = None


def set_default_scaling(scaling):
    """scaling: None or "pow2".  Returns the previous setting."""
    global _default_scaling
    prev = _default_scaling
    _default_scaling = ops._scaling(scaling)
    return prev


def get_default_scaling():
    return _default_scaling


def _cache_for(tensors, qd, n_inputs):
    """Buffers for the verified diagonal of P (forward -> backward of the same problems), only when a backward
    can follow (some input requires grad: what ctx.needs_input_grad will say) and the diagonal fast path exists for this N."""
    if _default_scaling is not None:
        return None
    if (_default_layout & 0xff) == ops._capi.P_AUTO and qd.shape[1] in _FAST_N and any(t.requires_grad for t in tensors[:n_inputs]):
        return ops.diag_cache(qd)
    return None


def _saved_cache(saved):
    return (saved[-2], saved[-1]) if saved[-1].dtype is torch.uint8 else None


def _device_for(t):
    if t.is_cuda:
        return t.device
    if not torch.cuda.is_available():
        raise RuntimeError("diffqcqp_amd needs an MI355X (ROCm) device: the solver is a HIP kernel and "
                           "there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


# ---- one forward body, one backward body ------------------------------------------------------------------------------------
# A class below says what it is -- `kind` (ops._KIND: 0 QP, 1 QCQP, 2 box QP, 3 signed box QP), `grads` (how many of its inputs,
# from P on, can get a gradient), `warm` (the forward starts from warm_start), `saves` (a backward follows) -- and keeps the
# reference's explicit forward signature, which autograd needs.  The Functions are written as forward + setup_context, the form
# torch.func's transforms (jvp, vjp, grad, jacfwd ...) accept: forward has no ctx, so what it staged and the diagonal cache it had
# the kernel fill travel to setup_context on the output tensor (`_dqq_saved`, taken off again there).
def _warm(q, warm_start, dev):
    if warm_start is None:
        raise ValueError("the warm-started classes need warm_start (B,N,1); QPFn2 and its siblings are the cold forwards")
    w = warm_start.detach().to(dev)
    return w.reshape(q.shape) if w.shape != q.shape else w


_detach = torch.Tensor.detach


def _solve_forward(cls, tensors, warm_start, eps, max_iter, mu_prox):
    """tensors: (P, q, the kind's extras).  Resident tensors are used in place, CPU ones staged through _device_for."""
    if cls.saves and _default_smoothing[0] and _default_derivative != "newton":
        raise ValueError('set_default_smoothing(kappa > 0) needs set_default_derivative("newton"): the reference derivatives '
                         "have no smoothed form")
    q = tensors[1]
    if q.is_cuda and not cls.warm:  # resident tensors: no staging, no copies
        dev, staged = q.device, list(map(_detach, tensors))
    else:
        dev = _device_for(q)
        staged = [t.detach().to(dev) for t in tensors]
    qd = staged[1]
    x0 = _warm(qd, warm_start, dev) if cls.warm else None
    if not cls.saves:
        l_2 = ops._forward(cls.kind, staged[0], qd, staged[2:], eps, max_iter, mu_prox, True, _default_layout, x0=x0,
                           scaling=_default_scaling)
    else:
        cache = _cache_for(tensors, qd, cls.grads)  # verified diagonal of P, reused by backward instead of re-reading P
        l_2 = ops._forward(cls.kind, staged[0], qd, staged[2:], eps, max_iter, mu_prox, True, _default_layout, False, None, cache,
                           None, x0, _default_scaling)
    if _default_polish > 0:   # in place: l_2 is this call's own buffer
        ops._polish(cls.kind, staged[0], qd, staged[2:], l_2, _default_polish, _default_layout, out=l_2,
                    infinite_bounds=_default_infinite_bounds, reg=_default_newton_reg, max_halvings=_default_polish_halvings)
    out = l_2 if q.is_cuda else l_2.to(q.device)
    if cls.saves:
        out._dqq_saved = (staged, l_2, cache, _default_layout)   # for _solve_setup
    return out


def _solve_setup(ctx, cls, inputs, output):
    """setup_context of every class with a backward: saves what the forward staged, the solution and the diagonal cache, for both
    modes.  A torch.func level above the one whose forward ran sees an output without `_dqq_saved`: it stages the inputs again
    and goes without the cache (the backward then reads P itself: the same bits)."""
    if not cls.saves:
        return
    n = 2 + len(ops._KIND[cls.kind][0])
    stash = output.__dict__.pop("_dqq_saved", None)
    if stash is None:
        dev = _device_for(inputs[1])
        stash = ([t.detach().to(dev) for t in inputs[:n]], output.detach().to(dev), None, _default_layout)
    staged, l_2, cache, layout = stash
    ctx.save_for_backward(*staged, l_2, *(cache or ()))
    ctx.save_for_forward(*staged, l_2)   # forward mode (jvp below) differentiates at the same point
    ctx.home = inputs[1].device
    ctx.layout = layout  # the backward of these problems takes the same route


_wrapped, _unwrap = torch._C._functorch.is_functorch_wrapped_tensor, torch._C._functorch.get_unwrapped


def _plain(t):
    """Inside a torch.func transform the saved tensors, tangents and cotangents arrive wrapped (no storage to take a pointer of):
    the tensor underneath.  The derivative kernels are leaves: nothing is differentiated through them a second time."""
    while t is not None and _wrapped(t):
        t = _unwrap(t)
    return t


def _leaf(fn, *args):
    """fn(*args) on plain tensors.  While a torch.func transform is active every torch call (detach, to, empty) wraps its result
    again: the call is made with the interpreter stack set aside."""
    if not torch._C._are_functorch_transforms_active():
        return fn(*args)
    from torch._functorch.pyfunctorch import temporarily_clear_interpreter_stack
    with temporarily_clear_interpreter_stack():
        return fn(*args)


def _solve_backward(ctx, cls, grad_l):
    """-> one value per forward input: the gradients ctx.needs_input_grad asks for, None for the rest (v, warm_start, eps,
    max_iter, mu_prox)."""
    return _leaf(_backward_leaf, ctx, cls, grad_l)


def _backward_leaf(ctx, cls, grad_l):
    saved = tuple(map(_plain, ctx.saved_tensors))
    n = 2 + len(ops._KIND[cls.kind][0])   # tensor inputs: P, q and the kind's extras
    l = saved[n]
    need = tuple(ctx.needs_input_grad[:cls.grads])
    grads = (None,) * cls.grads
    if any(need):
        if _default_derivative == "newton":
            at, kappa = _smoothed(cls, saved, n, l, ctx.layout)
            grads = ops._newton_backward(cls.kind, saved[0], saved[1], saved[2:n], at, _plain(grad_l).to(l.device), need, ctx.layout,
                                         infinite_bounds=_default_infinite_bounds, reg=_default_newton_reg, kappa=kappa)
        else:
            grads = ops._backward(cls.kind, saved[0], saved[1], saved[2:n], l, _plain(grad_l).to(l.device), need, ctx.layout, False,
                                  None, 1e-10, None, _saved_cache(saved), None)
        if ctx.home != l.device:
            grads = tuple(None if g is None else g.to(ctx.home) for g in grads)
    return grads + (None,) * (n + 4 - cls.grads)


def _solve_jvp(ctx, cls, tangents):
    """Forward mode (torch.autograd.forward_ad, torch.func.jvp): tangents has one entry per forward input; those of P, q and the kind's first two
    extras are used (None: a zero tangent), those of v, warm_start, eps, max_iter and mu_prox are ignored.  -> the tangent of x,
    one launch (ops._jvp: the exact transpose of the backward above)."""
    return _leaf(_jvp_leaf, ctx, cls, tangents)


def _jvp_leaf(ctx, cls, tangents):
    saved = tuple(map(_plain, ctx.saved_tensors))
    n = 2 + len(ops._KIND[cls.kind][0])
    l = saved[n]
    tans = [None if t is None else _plain(t).detach().to(l.device) for t in tangents[:cls.grads]]
    if _default_derivative == "newton":
        at, kappa = _smoothed(cls, saved, n, l, ctx.layout)
        dx = ops._newton_jvp(cls.kind, saved[0], saved[1], saved[2:n], at, tans, ctx.layout, infinite_bounds=_default_infinite_bounds,
                             reg=_default_newton_reg, kappa=kappa)
    else:
        dx = ops._jvp(cls.kind, saved[0], saved[1], saved[2:n], l, tans, ctx.layout)
    return dx if ctx.home == l.device else dx.to(ctx.home)


class QPFn2(Function):
    kind, grads, warm, saves = 0, 2, False, True

    @staticmethod
    def forward(P, q, warm_start, eps, max_iter, mu_prox=1e-7):
        return _solve_forward(QPFn2, (P, q), warm_start, eps, max_iter, mu_prox)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _solve_setup(ctx, QPFn2, inputs, output)

    @staticmethod
    def backward(ctx, grad_l):
        return _solve_backward(ctx, QPFn2, grad_l)

    @staticmethod
    def jvp(ctx, *tangents):
        return _solve_jvp(ctx, QPFn2, tangents)


class QCQPFn2(Function):
    kind, grads, warm, saves = 1, 4, False, True

    @staticmethod
    def forward(P, q, l_n, mu, warm_start, eps, max_iter, mu_prox=1e-7):
        return _solve_forward(QCQPFn2, (P, q, l_n, mu), warm_start, eps, max_iter, mu_prox)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _solve_setup(ctx, QCQPFn2, inputs, output)

    @staticmethod
    def backward(ctx, grad_l):
        return _solve_backward(ctx, QCQPFn2, grad_l)

    @staticmethod
    def jvp(ctx, *tangents):
        return _solve_jvp(ctx, QCQPFn2, tangents)


class BoxQPFn2(Function):
    """min 1/2 x'Px + q'x, l_min <= x <= l_max (reference qcqp.py:54-94).

    The reference's forward works; its backward does not run (wrong unpack counts, swapped saved tensors,
    `.asDiagonal()` on a tensor -- SURVEY.md section 2 #7).  This backward computes what that code spells out,
    grad_P = -dl l', grad_q = -dl, grad_l_min = -dgamma_lo*gamma_lo, and grad_l_max = +dgamma_hi*gamma_hi: the
    reference writes a minus sign there (qcqp.py:93), finite differences say plus (tests/test_oracle.py)."""
    kind, grads, warm, saves = 2, 4, False, True

    @staticmethod
    def forward(P, q, l_min, l_max, warm_start, eps, max_iter, mu_prox=1e-7):
        return _solve_forward(BoxQPFn2, (P, q, l_min, l_max), warm_start, eps, max_iter, mu_prox)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _solve_setup(ctx, BoxQPFn2, inputs, output)

    @staticmethod
    def backward(ctx, grad_l):
        return _solve_backward(ctx, BoxQPFn2, grad_l)

    @staticmethod
    def jvp(ctx, *tangents):
        return _solve_jvp(ctx, BoxQPFn2, tangents)


class SignedBoxQPFn2(Function):
    """The box QP with the extra constraint sign(v_i) x_i <= 0 (reference qcqp.py:97-137).  Forward only: the
    reference marks its backward "not implemented" (qcqp.py:111) -- it would differentiate the plain box QP,
    ignoring v -- so asking for a gradient raises instead of returning something wrong.  SignedBoxQPDiffFn2 below is
    the same operator with a backward."""
    kind, grads, warm, saves = 3, 4, False, False

    @staticmethod
    def forward(P, q, l_min, l_max, v, warm_start, eps, max_iter, mu_prox=1e-7):
        return _solve_forward(SignedBoxQPFn2, (P, q, l_min, l_max, v), warm_start, eps, max_iter, mu_prox)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _solve_setup(ctx, SignedBoxQPFn2, inputs, output)

    @staticmethod
    def backward(ctx, grad_l):
        raise NotImplementedError("SignedBoxQPFn2 has no backward (not implemented in the reference either, "
                                  "qcqp.py:111)")

    @staticmethod
    def jvp(ctx, *tangents):
        raise NotImplementedError("SignedBoxQPFn2 has no derivative, in either mode (qcqp.py:111); SignedBoxQPDiffFn2 has both")


class SignedBoxQPDiffFn2(Function):
    """SignedBoxQPFn2 with a backward: the signed box QP is the box QP on the effective bounds the sign constraint
    leaves (include/diffqcqp_hip.h: dqq_signedboxqp_bwd_f64), so its gradients are BoxQPFn2's there -- grad_l_min /
    grad_l_max +0.0 where the constraint sign(v_i) x_i <= 0 has replaced the bound, and no gradient for v (x is piecewise
    constant in it).  A class of its own: SignedBoxQPFn2 keeps raising, as callers of the reference's surface expect."""
    kind, grads, warm, saves = 3, 4, False, True

    @staticmethod
    def forward(P, q, l_min, l_max, v, warm_start, eps, max_iter, mu_prox=1e-7):
        return _solve_forward(SignedBoxQPDiffFn2, (P, q, l_min, l_max, v), warm_start, eps, max_iter, mu_prox)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _solve_setup(ctx, SignedBoxQPDiffFn2, inputs, output)

    @staticmethod
    def backward(ctx, grad_l):
        return _solve_backward(ctx, SignedBoxQPDiffFn2, grad_l)

    @staticmethod
    def jvp(ctx, *tangents):
        return _solve_jvp(ctx, SignedBoxQPDiffFn2, tangents)


# ---- warm-started twins (an extension: the reference has none) --------------------------------------------------------------
# The same signatures as the classes above, but `warm_start` (B,N,1) is honoured: the ADMM loop starts from it (l_2 = warm_start,
# u = -(P warm_start + q), include/diffqcqp_hip.h: dqq_fwd_warm_f64) -- the previous step's x of a time-stepping simulation or a
# training loop saves most of the iterations.  Not projected; max_iter = 0 returns it; zeros are not the cold start.  The
# solution, and with it the backward, is the base class's: each backward and jvp IS the base class's, and warm_start gets no
# gradient and no tangent.
class QPWarmFn2(QPFn2):
    warm = True

    @staticmethod
    def forward(P, q, warm_start, eps, max_iter, mu_prox=1e-7):
        return _solve_forward(QPWarmFn2, (P, q), warm_start, eps, max_iter, mu_prox)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _solve_setup(ctx, QPWarmFn2, inputs, output)


class QCQPWarmFn2(QCQPFn2):
    warm = True

    @staticmethod
    def forward(P, q, l_n, mu, warm_start, eps, max_iter, mu_prox=1e-7):
        return _solve_forward(QCQPWarmFn2, (P, q, l_n, mu), warm_start, eps, max_iter, mu_prox)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _solve_setup(ctx, QCQPWarmFn2, inputs, output)


class BoxQPWarmFn2(BoxQPFn2):
    warm = True

    @staticmethod
    def forward(P, q, l_min, l_max, warm_start, eps, max_iter, mu_prox=1e-7):
        return _solve_forward(BoxQPWarmFn2, (P, q, l_min, l_max), warm_start, eps, max_iter, mu_prox)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _solve_setup(ctx, BoxQPWarmFn2, inputs, output)


class SignedBoxQPWarmFn2(SignedBoxQPDiffFn2):
    """The warm-started signed box QP; its backward is SignedBoxQPDiffFn2's."""
    warm = True

    @staticmethod
    def forward(P, q, l_min, l_max, v, warm_start, eps, max_iter, mu_prox=1e-7):
        return _solve_forward(SignedBoxQPWarmFn2, (P, q, l_min, l_max, v), warm_start, eps, max_iter, mu_prox)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _solve_setup(ctx, SignedBoxQPWarmFn2, inputs, output)
