"""Tensor-level entry points over the C ABI: one asynchronous launch per batch.

Inputs are float64 CUDA (ROCm) tensors in the reference's layouts -- P (B,N,N),
q (B,N,1), l_n / mu (B,N/2,1) -- and every call runs on torch's current stream.
torch is used here for device memory and streams only.

Workspace: every op takes `workspace=` (ops.make_workspace); without it a per-(device, stream) cache is used.  HIP-graph
capture: warm the capture stream up with one eager call first (or pass workspace=); a cached workspace that was live
during a capture is never replaced or freed afterwards, so a replayed graph cannot write into recycled memory.
"""
import ctypes
from collections import namedtuple

import torch

from . import _capi

_workspaces = {}

try:  # raw stream handle of torch's current stream without building a Stream object (private but stable)
    _raw_stream = torch._C._cuda_getCurrentRawStream
except AttributeError:  # pragma: no cover
    def _raw_stream(index):
        return torch.cuda.current_stream(index).cuda_stream


class _device_guard:
    """`with torch.cuda.device(dev)` only when dev is not already current (the context manager costs
    several microseconds per call, the hot path is tens of microseconds)."""

    def __init__(self, dev):
        self.ctx = None if dev.index == torch.cuda.current_device() else torch.cuda.device(dev)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.ctx is not None:
            self.ctx.__exit__(*a)


_MAX_WORKSPACES = 16   # cached (device, stream) pairs; the least recently used one is dropped beyond that
_pinned = []           # workspaces handed out while a stream capture was going on: a captured graph has their address
                       # baked in, so they are never replaced, evicted or freed
_need_cache = {}       # (kind, pas, N, B, flags) -> bytes: dqq_workspace_bytes + dqq_scratch_bytes are functions of exactly these


def _hints(kind, pas, N, B, layout, dev):
    """(flags, report address) for this call: the caller's side of include/diffqcqp_hip.h's hint protocol.  Only DQQ_P_AUTO
    batches of QP / QCQP, N <= 8; a caller that already passes hint flags in `layout` keeps them."""
    if (layout & 0xff) != _capi.P_AUTO or N > 8 or kind > 1 or (layout & (_capi.F_EXPECT_DENSE | _capi.F_EXPECT_LONG_LIST)):
        return 0, None
    flags, report = _capi.hint(kind, pas, N, B, dev.index)
    if flags and _capturing():   # (asked only when a hint is about to be followed) a graph is replayed on batches the word
        flags = 0                # knows nothing about: what goes into it is the argument-determined route
    return flags, report


def _capturing():
    try:
        return torch.cuda.is_current_stream_capturing()
    except Exception:  # pragma: no cover
        return False


def workspace_bytes(B, kind=0, pas=0, N=8, layout=0):
    """Bytes of `workspace` a call needs: the work-list + whatever scratch the kernels of (kind, pas, N, B, layout flags) use
    -- asked of the library (dqq_workspace_bytes + dqq_scratch_bytes), never guessed here."""
    key = (int(kind), int(pas), int(N), int(B), int(layout) & _capi.F_REFERENCE_ORDER)
    need = _need_cache.get(key)
    if need is None:
        lib = _capi.lib()
        need = lib.dqq_workspace_bytes(int(B)) + lib.dqq_scratch_bytes(*key)
        if len(_need_cache) >= 1024:   # (B varies freely in a caller's hands: bounded)
            _need_cache.clear()
        _need_cache[key] = need
    return need


def make_workspace(device, B, kind=0, pas=0, N=8, layout=0):
    """A caller-owned workspace for the `workspace=` argument of the ops below (int32, zero-initialised work-list header,
    uninitialised scratch behind it).  A caller that captures ops calls into a HIP graph should own one per stream and
    keep it alive as long as the graph: the captured launches hold its address."""
    lib = _capi.lib()
    head = lib.dqq_workspace_bytes(int(B))
    need = max(workspace_bytes(B, kind, pas, N, layout), 4096)
    ws = torch.empty((need + 3) // 4, dtype=torch.int32, device=device)
    ws[: (head + 3) // 4].zero_()     # only the work-list must start zeroed (= dqq_workspace_reset); the scratch needs no initialisation
    return ws


def _workspace(device, B, stream=None, kind=0, pas=0, N=8, given=None, layout=0):
    """The work-list (+ the scratch of the global-memory kernels behind it, when (kind, pas, N) needs any): the
    caller's (`given`, checked for size) or one cached per (device, stream); the kernels leave the work-list empty again
    (include/diffqcqp_hip.h: dqq_workspace_bytes, dqq_scratch_bytes).
    Lifetime rule of the cache: an entry is replaced when a larger call arrives and evicted beyond 16 streams -- except
    entries that were handed out during a stream capture, which stay alive for the life of the process."""
    need = workspace_bytes(B, kind, pas, N, layout)
    if given is not None:
        if not (given.is_cuda and given.dtype is torch.int32 and given.is_contiguous() and given.numel() * 4 >= need):
            raise ValueError("workspace must be a contiguous int32 GPU tensor of at least %d bytes (ops.make_workspace)" % need)
        return given
    if stream is None:
        stream = _raw_stream(device.index)
    key = (device.index, stream)
    ws = _workspaces.get(key)
    cap = _capturing()
    if ws is None or ws.numel() * 4 < need:
        if cap:   # (created OR grown: either way an allocation and a zero-fill would be captured, and the cache entry replaced)
            raise RuntimeError("diffqcqp_amd.ops: a call inside a stream capture needs a workspace that is not there yet (first "
                               "call on this stream, or a larger batch than any before) -- it would be allocated and zero-filled "
                               "inside the capture; warm the stream up with the largest call first or pass workspace=")
        ws = make_workspace(device, B, kind, pas, N, layout)
        _workspaces.pop(key, None)
        _workspaces[key] = ws
        while len(_workspaces) > _MAX_WORKSPACES:
            _workspaces.pop(next(iter(_workspaces)))   # (pinned ones stay referenced by _pinned)
    elif len(_workspaces) > 1:
        _workspaces[key] = _workspaces.pop(key)  # most recently used last
    if cap and not any(w is ws for w in _pinned):
        _pinned.append(ws)
    return ws


def _ptr(t):
    return 0 if t is None else t.data_ptr()


_data_ptr = torch.Tensor.data_ptr


def _prep(t, name, shape=None):
    if t.is_cuda and t.dtype is torch.float64 and t.is_contiguous() and (shape is None or t.shape == shape):
        return t  # the common case: nothing to do (data_ptr() ignores autograd state)
    if not t.is_cuda:
        raise ValueError("%s must live on the GPU (got %s)" % (name, t.device))
    if t.dtype != torch.float64:
        t = t.to(torch.float64)
    t = t.detach().contiguous()
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    return t


def _out(t, shape, name):
    """A caller-provided output buffer: the kernels write float64 into it, so anything else must be refused here."""
    if t is None:
        return None
    if not (t.is_cuda and t.dtype is torch.float64 and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise ValueError("%s must be a contiguous float64 GPU tensor of shape %s (got %s %s on %s)"
                         % (name, tuple(shape), t.dtype, tuple(t.shape), t.device))
    return t


def _dims(P, q, layout):
    """layout: DQQ_P_* optionally ORed with _capi.F_REFERENCE_ORDER (include/diffqcqp_hip.h), passed to the C ABI as is."""
    B, N = q.shape[0], q.shape[1]
    pshape = (B, N) if (layout & 0xff) == _capi.P_DIAG else (B, N, N)
    return B, N, pshape


def diag_cache(q):
    """Buffers a forward can fill for the backward of the same problems: (pdiag (B,N), flags (B) uint8)."""
    B, N = q.shape[0], q.shape[1]
    return (torch.empty((B, N), dtype=torch.float64, device=q.device),
            torch.empty(B, dtype=torch.uint8, device=q.device))


# What a call of each kind (include/diffqcqp_hip.h: 0 QP, 1 QCQP, 2 box QP, 3 signed box QP) differs in -- the one table the
# generic _forward / _backward / solution_check below read:
#   names        the kind's extra inputs, in the order of the C ABI (as many as capi.hip's kExtras says); the first two get
#                gradients, v gets none
#   per_contact  the extras and their gradients are (B, N/2, 1), one entry per contact; (B, N, 1) otherwise
#   fwd, bwd     the cold C symbols (every warm forward is dqq_fwd_warm_f64)
#   hints        QP / QCQP: the calls take hint flags, the backward a report word, and ir_steps is (B,); the box kinds: no hints,
#                no report parameter, ir_steps (B, 2)
#   bwd_ws       the kind whose scratch the backward is sized by (the signed box backward runs on the box QP's)
_KIND = (((),                      False, "dqq_qp_fwd_f64",          "dqq_qp_bwd_f64",          True,  0),
         (("l_n", "mu"),           True,  "dqq_qcqp_fwd_f64",        "dqq_qcqp_bwd_f64",        True,  1),
         (("l_min", "l_max"),      False, "dqq_boxqp_fwd_f64",       "dqq_boxqp_bwd_f64",       False, 2),
         (("l_min", "l_max", "v"), False, "dqq_signedboxqp_fwd_f64", "dqq_signedboxqp_bwd_f64", False, 2))
_KINDS = {"qp": 0, "qcqp": 1, "box": 2, "sbox": 3}
_GENERIC_NAMES = ("extras[0]", "extras[1]", "extras[2]")   # what the kind-generic entries (warm forward, check) call the extras
_NULLS = ((0, 0, 0), (0, 0), (0,), ())                      # the a, b, c a kind with that many extras leaves NULL


def _forward(kind, P, q, extras, eps, max_iter, mu_prox=1e-7, adaptive_rho=True, layout=_capi.P_AUTO, return_iters=False,
             out=None, cache=None, workspace=None, x0=None, scaling=None):
    """The forward of every kind, cold (x0 None: the kind's own entry point) or started from x0 (dqq_fwd_warm_f64: the cold
    forward entered from x0, include/diffqcqp_hip.h has the start state; x0 (B,N,1) is read only and must not be the output
    buffer).  extras: the kind's extra inputs in _KIND's order.  One workspace cache and one set of hints for both.
    scaling: None, or "pow2" (_forward_scaled: the same forward on the equilibrated problem)."""
    if scaling is not None:
        return _forward_scaled(kind, P, q, extras, eps, max_iter, mu_prox, adaptive_rho, layout, return_iters, out, cache,
                               workspace, x0, scaling)
    names, per_contact, what, _, hints, _ = _KIND[kind]
    B, N, pshape = _dims(P, q, layout)
    P, q = _prep(P, "P", pshape), _prep(q, "q", (B, N, 1))
    dev = q.device
    if extras:
        eshape = (B, N // 2, 1) if per_contact else (B, N, 1)
        extras = [_prep(e, n, eshape) for e, n in zip(extras, names if x0 is None else _GENERIC_NAMES)]   # (held until the call)
        head = (P.data_ptr(), q.data_ptr(), *map(_data_ptr, extras))
    else:
        head = (P.data_ptr(), q.data_ptr())
    x = _out(out, (B, N, 1), "out") if out is not None else torch.empty((B, N, 1), dtype=torch.float64, device=dev)
    if x0 is not None:
        what = "dqq_fwd_warm_f64"
        x0 = _prep(x0, "x0", (B, N, 1))
        if B > 0 and x.data_ptr() == x0.data_ptr():
            raise ValueError("x0 must not be the output buffer (include/diffqcqp_hip.h: dqq_fwd_warm_f64)")
        head = (kind, *head, *_NULLS[len(extras)], x0.data_ptr())
    iters = torch.empty(B, dtype=torch.int32, device=dev) if return_iters else None
    stream = _raw_stream(dev.index)
    ws = _workspace(dev, B, stream, kind, 0, N, workspace, layout)
    if hints:
        layout |= _hints(kind, 0, N, B, layout, dev)[0]
    pd, fl = (_ptr(cache[0]), _ptr(cache[1])) if cache is not None else (0, 0)
    with _device_guard(dev):
        rc = getattr(_capi.lib(), what)(*head, x.data_ptr(), B, N, float(eps), float(mu_prox), int(max_iter),
                                        int(bool(adaptive_rho)), layout, iters.data_ptr() if return_iters else 0, pd, fl,
                                        ws.data_ptr(), ws.numel() * 4, stream)
    _capi.check(rc, what)
    return (x, iters) if return_iters else x


def qp_forward(P, q, eps, max_iter, mu_prox=1e-7, adaptive_rho=True, layout=_capi.P_AUTO, return_iters=False,
               out=None, cache=None, workspace=None, scaling=None):
    """Batched QP solve min 1/2 x'Px + q'x, x >= 0 (reference qcqp.py:24-33). -> x (B,N,1).
    cache: optional `diag_cache(q)` buffers; pass the same pair to qp_backward (P must be unchanged)."""
    return _forward(0, P, q, (), eps, max_iter, mu_prox, adaptive_rho, layout, return_iters, out, cache, workspace, scaling=scaling)


def qcqp_forward(P, q, l_n, mu, eps, max_iter, mu_prox=1e-7, adaptive_rho=True, layout=_capi.P_AUTO,
                 return_iters=False, out=None, cache=None, workspace=None, scaling=None):
    """Batched QCQP solve, ||x_(i)|| <= mu_i*l_n_i per contact (reference qcqp.py:144-153)."""
    return _forward(1, P, q, (l_n, mu), eps, max_iter, mu_prox, adaptive_rho, layout, return_iters, out, cache, workspace, scaling=scaling)


def boxqp_forward(P, q, l_min, l_max, eps, max_iter, v=None, mu_prox=1e-7, adaptive_rho=True, layout=_capi.P_AUTO,
                  return_iters=False, out=None, cache=None, workspace=None, scaling=None):
    """Batched box QP solve, l_min <= x <= l_max (reference qcqp.py:56-65); with `v` the signed box QP,
    additionally sign(v_i) x_i <= 0 (reference qcqp.py:99-108)."""
    kind, extras = (2, (l_min, l_max)) if v is None else (3, (l_min, l_max, v))
    return _forward(kind, P, q, extras, eps, max_iter, mu_prox, adaptive_rho, layout, return_iters, out, cache, workspace, scaling=scaling)


def qp_forward_warm(P, q, x0, eps, max_iter, mu_prox=1e-7, adaptive_rho=True, layout=_capi.P_AUTO, return_iters=False,
                    out=None, cache=None, workspace=None, scaling=None):
    """qp_forward started from x0 (B,N,1), e.g. the last step's x: l_2 = x0, u = -(P x0 + q).  max_iter = 0 returns x0; x0 = 0 is
    not the cold start."""
    return _forward(0, P, q, (), eps, max_iter, mu_prox, adaptive_rho, layout, return_iters, out, cache, workspace, x0, scaling)


def qcqp_forward_warm(P, q, l_n, mu, x0, eps, max_iter, mu_prox=1e-7, adaptive_rho=True, layout=_capi.P_AUTO,
                      return_iters=False, out=None, cache=None, workspace=None, scaling=None):
    """qcqp_forward started from x0 (B,N,1)."""
    return _forward(1, P, q, (l_n, mu), eps, max_iter, mu_prox, adaptive_rho, layout, return_iters, out, cache, workspace, x0, scaling)


def boxqp_forward_warm(P, q, l_min, l_max, x0, eps, max_iter, v=None, mu_prox=1e-7, adaptive_rho=True, layout=_capi.P_AUTO,
                       return_iters=False, out=None, cache=None, workspace=None, scaling=None):
    """boxqp_forward (with `v`: the signed box QP) started from x0 (B,N,1)."""
    kind, extras = (2, (l_min, l_max)) if v is None else (3, (l_min, l_max, v))
    return _forward(kind, P, q, extras, eps, max_iter, mu_prox, adaptive_rho, layout, return_iters, out, cache, workspace, x0, scaling)


# ---- power-of-two equilibration (include/diffqcqp_hip.h: dqq_equilibrate_f64, dqq_unscale_f64; csrc/equil_core.h has the rule) ---
SCALINGS = (None, "pow2")


def _scaling(scaling):
    if scaling not in SCALINGS:
        raise ValueError('scaling must be None or "pow2", got %r' % (scaling,))
    return scaling


def equilibrate(kind, P, q, extras, x0=None, layout=_capi.P_AUTO, out=None):
    """The problem in the units x = D y, D = diag(2^e): one streaming launch on the current stream.  kind: 0 / "qp", 1 / "qcqp",
    2 / "box", 3 / "sbox"; extras: the kind's extra inputs in the forwards' order; x0 (B,N,1): a warm start, or None; layout: as
    the forward's (DQQ_P_DIAG: P is (B,N)).
    -> (P~ = D P D, q~ = D q, extras~, x0~ = D^-1 x0 or None, e (B,N) int32).  extras~: the QCQP's (2^-e l_n, mu), the box kinds'
    (D^-1 l_min, D^-1 l_max[, v]); mu and v are not copied: the tensors given (prepared as every op prepares its inputs).
    Every factor is a power of two: nothing is rounded, the scaled problem is the caller's (csrc/equil_core.h).
    out: optional (P~, q~, extras~, x0~, e) buffers to write into, extras~ with one buffer per scaled extra (mu and v have none);
    no buffer may overlap an input."""
    k = _KINDS.get(kind, kind)
    if k not in (0, 1, 2, 3):
        raise ValueError("kind must be one of %s or 0..3 (got %r)" % (sorted(_KINDS), kind))
    names, per_contact = _KIND[k][0], _KIND[k][1]
    B, N, pshape = _dims(P, q, layout)
    extras = tuple(extras or ())
    if len(extras) != len(names):
        raise ValueError("kind %r takes %d extra inputs (got %d)" % (kind, len(names), len(extras)))
    P, q = _prep(P, "P", pshape), _prep(q, "q", (B, N, 1))
    eshape = (B, N // 2, 1) if per_contact else (B, N, 1)
    extras = [_prep(t, n, eshape) for t, n in zip(extras, names)]
    nscaled = (0, 1, 2, 2)[k]   # l_n; l_min, l_max: the extras that change
    if x0 is not None:
        x0 = _prep(x0, "x0", (B, N, 1))
    dev = q.device
    new = lambda shape: torch.empty(shape, dtype=torch.float64, device=dev)
    if out is not None:
        Pt, qt, ext, x0t, e = out
        Pt, qt = _out(Pt, pshape, "out[0]"), _out(qt, (B, N, 1), "out[1]")
        ext = [_out(t, eshape, "out[2][%d]" % i) for i, t in enumerate(tuple(ext or ())[:nscaled])]
        if len(ext) != nscaled:
            raise ValueError("out[2] must hold %d buffers" % nscaled)
        x0t = _out(x0t, (B, N, 1), "out[3]") if x0 is not None else None
        if not (e.is_cuda and e.dtype is torch.int32 and e.is_contiguous() and tuple(e.shape) == (B, N)):
            raise ValueError("out[4] must be a contiguous int32 GPU tensor of shape (%d, %d)" % (B, N))
    else:
        Pt, qt = new(pshape), new((B, N, 1))
        ext = [new(eshape) for _ in range(nscaled)]
        x0t = new((B, N, 1)) if x0 is not None else None
        e = torch.empty((B, N), dtype=torch.int32, device=dev)
    ins = extras + [None] * (3 - len(extras))
    outs = ext + [None] * (3 - nscaled)
    with _device_guard(dev):
        rc = _capi.lib().dqq_equilibrate_f64(k, P.data_ptr(), q.data_ptr(), *map(_ptr, ins), _ptr(x0), B, N, layout, Pt.data_ptr(),
                                             qt.data_ptr(), *map(_ptr, outs), _ptr(x0t), e.data_ptr(), _raw_stream(dev.index))
    _capi.check(rc, "dqq_equilibrate_f64")
    return Pt, qt, tuple(ext) + tuple(extras[nscaled:]), x0t, e


def unscale(y, e, out=None):
    """x = D y (B,N,1) from a solution y of the equilibrated problem and equilibrate's e (B,N) int32: one elementwise launch on
    the current stream.  out: the buffer to write into; may be y itself."""
    if y.dim() != 3 or y.shape[2] != 1:
        raise ValueError("y must be (B,N,1), got %s" % (tuple(y.shape),))
    B, N = y.shape[0], y.shape[1]
    y = _out(y, (B, N, 1), "y") if out is y else _prep(y, "y", (B, N, 1))
    if not (e.is_cuda and e.dtype is torch.int32 and e.is_contiguous() and tuple(e.shape) == (B, N)):
        raise ValueError("e must be a contiguous int32 GPU tensor of shape (%d, %d)" % (B, N))
    dev = y.device
    x = _out(out, (B, N, 1), "out") if out is not None else torch.empty((B, N, 1), dtype=torch.float64, device=dev)
    with _device_guard(dev):
        rc = _capi.lib().dqq_unscale_f64(y.data_ptr(), e.data_ptr(), B, N, x.data_ptr(), _raw_stream(dev.index))
    _capi.check(rc, "dqq_unscale_f64")
    return x


def _forward_scaled(kind, P, q, extras, eps, max_iter, mu_prox, adaptive_rho, layout, return_iters, out, cache, workspace, x0,
                    scaling):
    """_forward with scaling="pow2": equilibrate, the unchanged forward on the scaled problem, unscale (in place on the forward's
    output) -- three launches on the current stream.  eps is applied to the scaled problem's residuals and the iteration counts
    are the scaled solve's; workspace, hints and report see the scaled batch, which takes the route the caller's would (a
    diagonal P stays diagonal).  cache: refused -- pdiag_out would hold the scaled diagonal, and the backward runs on the
    caller's P."""
    _scaling(scaling)
    if cache is not None:
        raise ValueError('cache= holds the diagonal of the matrix that was solved: with scaling="pow2" that is the scaled one, and '
                         "the backward differentiates the caller's problem -- call without cache")
    Pt, qt, ext, x0t, e = equilibrate(kind, P, q, extras, x0, layout)
    res = _forward(kind, Pt, qt, ext, eps, max_iter, mu_prox, adaptive_rho, layout, return_iters, out, None, workspace, x0t)
    y = res[0] if return_iters else res
    unscale(y, e, out=y)
    return res


# (The gradient-buffer block below is _grad_buffers', stated a second time: the benchmark's path takes no call for it.)
def _backward(kind, P, q, extras, x, grad_x, need, layout, return_steps, out, epsilon, duals, cache, workspace):
    """The implicit-function backward of every kind.  need / out: one entry per gradient output -- P, q and, but for the QP, the
    kind's first two extras.  -> the gradients (None where not needed), then the step counts if asked for."""
    names, per_contact, _, what, hints, ws_kind = _KIND[kind]
    B, N, pshape = _dims(P, q, layout)
    P, q = _prep(P, "P", pshape), _prep(q, "q", (B, N, 1))
    eshape = (B, N // 2, 1) if per_contact else (B, N, 1)
    extras = [_prep(e, n, eshape) for e, n in zip(extras, names)]   # (held until the call)
    x, grad_x = _prep(x, "x", (B, N, 1)), _prep(grad_x, "grad_x", (B, N, 1))
    dev = q.device
    ga = gb = None
    if out is not None:
        gP, gq = _out(out[0], pshape, "out[0]"), _out(out[1], (B, N, 1), "out[1]")
        if kind:
            ga, gb = _out(out[2], eshape, "out[2]"), _out(out[3], eshape, "out[3]")
    else:
        gP = torch.empty(pshape, dtype=torch.float64, device=dev) if need[0] else None
        gq = torch.empty((B, N, 1), dtype=torch.float64, device=dev) if need[1] else None
        if kind:
            ga = torch.empty(eshape, dtype=torch.float64, device=dev) if need[2] else None
            gb = torch.empty(eshape, dtype=torch.float64, device=dev) if need[3] else None
    steps = torch.empty(B if hints else (B, 2), dtype=torch.int32, device=dev) if return_steps else None
    stream = _raw_stream(dev.index)
    ws = _workspace(dev, B, stream, ws_kind, 1, N, workspace, layout)
    head = (P.data_ptr(), q.data_ptr(), *map(_data_ptr, extras), x.data_ptr(), grad_x.data_ptr(), _ptr(gP), _ptr(gq))
    if kind:
        head += (_ptr(ga), _ptr(gb), *((_ptr(duals[0]), _ptr(duals[1])) if duals is not None else (0, 0)))
    report = ()
    if hints:
        hf, word = _hints(kind, 1, N, B, layout, dev)
        layout |= hf
        report = (word,)
    pd, fl = (_ptr(cache[0]), _ptr(cache[1])) if cache is not None else (0, 0)
    with _device_guard(dev):
        rc = getattr(_capi.lib(), what)(*head, B, N, float(epsilon), layout, steps.data_ptr() if return_steps else 0, pd, fl,
                                        *report, ws.data_ptr(), ws.numel() * 4, stream)
    _capi.check(rc, what)
    grads = (gP, gq, ga, gb) if kind else (gP, gq)
    return grads + (steps,) if return_steps else grads


def qp_backward(P, q, x, grad_x, need_P=True, need_q=True, layout=_capi.P_AUTO, return_steps=False, out=None,
                epsilon=1e-10, cache=None, workspace=None):
    """Implicit-function backward of the QP (reference qcqp.py:36-52). -> (grad_P|None, grad_q|None)"""
    return _backward(0, P, q, (), x, grad_x, (need_P, need_q), layout, return_steps, out, epsilon, None, cache, workspace)


def qcqp_backward(P, q, l_n, mu, x, grad_x, need=(True, True, True, True), layout=_capi.P_AUTO, return_steps=False,
                  out=None, epsilon=1e-10, duals=None, cache=None, workspace=None):
    """Implicit-function backward of the QCQP (reference qcqp.py:156-181).
    -> (grad_P, grad_q, grad_l_n, grad_mu), None where not needed.  duals: optional pair of (B,N/2,1)
    tensors that receive the contact duals gamma and their derivative terms dgamma."""
    return _backward(1, P, q, (l_n, mu), x, grad_x, need, layout, return_steps, out, epsilon, duals, cache, workspace)


def boxqp_backward(P, q, l_min, l_max, x, grad_x, need=(True, True, True, True), layout=_capi.P_AUTO,
                   return_steps=False, out=None, duals=None, epsilon=1e-10, cache=None, workspace=None, v=None):
    """Implicit-function backward of the box QP: what BoxQPFn2.backward (reference qcqp.py:67-94) spells out,
    with the signs finite differences confirm.  -> (grad_P, grad_q, grad_l_min, grad_l_max), None where not
    needed.  duals: optional pair of (B,2N) tensors that receive gamma and dgamma ([lower | upper]).
    return_steps: also the (B,2) refinement step counts (dual recovery, derivative system).
    With `v` (B,N,1) the signed box QP's backward (dqq_signedboxqp_bwd_f64): the box backward on the effective bounds the
    sign constraint leaves, grad_l_min / grad_l_max +0.0 where it has replaced the bound; v itself gets no gradient."""
    kind, extras = (2, (l_min, l_max)) if v is None else (3, (l_min, l_max, v))
    return _backward(kind, P, q, extras, x, grad_x, need, layout, return_steps, out, epsilon, duals, cache, workspace)


def _jvp(kind, P, q, extras, x, tangents, layout=_capi.P_AUTO, return_steps=False, out=None, epsilon=1e-10, workspace=None):
    """The forward-mode derivative of every kind (include/diffqcqp_hip.h: dqq_jvp_f64, the exact transpose of the kind's
    backward).  tangents: (dP, dq) and, but for the QP, those of the kind's first two extras -- each of its input's shape
    (DQQ_P_DIAG: dP (B,N) like P) or None for a zero tangent; v takes none.  -> dx (B,N,1), then the step counts if asked for."""
    names, per_contact, _, _, hints, ws_kind = _KIND[kind]
    B, N, pshape = _dims(P, q, layout)
    P, q, x = _prep(P, "P", pshape), _prep(q, "q", (B, N, 1)), _prep(x, "x", (B, N, 1))
    eshape = (B, N // 2, 1) if per_contact else (B, N, 1)
    extras = [_prep(e, n, eshape) for e, n in zip(extras, names)] + [None] * (3 - len(names))   # (held until the call)
    tangents = _tangents(kind, tangents, pshape, B, N, eshape)
    dev = q.device
    dx = _out(out, (B, N, 1), "out") if out is not None else torch.empty((B, N, 1), dtype=torch.float64, device=dev)
    steps = torch.empty(B if hints else (B, 2), dtype=torch.int32, device=dev) if return_steps else None
    stream = _raw_stream(dev.index)
    ref = layout | _capi.F_REFERENCE_ORDER   # the JVP's general routes are the reference-order ones: their scratch
    ws = None
    if (layout & 0xff) != _capi.P_DIAG and workspace_bytes(B, ws_kind, 1, N, ref) > workspace_bytes(B):
        ws = _workspace(dev, B, stream, ws_kind, 1, N, workspace, ref)
    with _device_guard(dev):
        rc = _capi.lib().dqq_jvp_f64(kind, P.data_ptr(), q.data_ptr(), *map(_ptr, extras), x.data_ptr(), *map(_ptr, tangents),
                                     dx.data_ptr(), B, N, float(epsilon), layout, _ptr(steps), _ptr(ws),
                                     ws.numel() * 4 if ws is not None else 0, stream)
    _capi.check(rc, "dqq_jvp_f64")
    return (dx, steps) if return_steps else dx


def qp_jvp(P, q, x, dP=None, dq=None, layout=_capi.P_AUTO, return_steps=False, out=None, epsilon=1e-10, workspace=None):
    """dx (B,N,1) of the QP's solution along (dP, dq); None = a zero tangent."""
    return _jvp(0, P, q, (), x, (dP, dq), layout, return_steps, out, epsilon, workspace)


def qcqp_jvp(P, q, l_n, mu, x, dP=None, dq=None, dl_n=None, dmu=None, layout=_capi.P_AUTO, return_steps=False, out=None,
             epsilon=1e-10, workspace=None):
    """dx (B,N,1) of the QCQP's solution along (dP, dq, dl_n, dmu)."""
    return _jvp(1, P, q, (l_n, mu), x, (dP, dq, dl_n, dmu), layout, return_steps, out, epsilon, workspace)


def boxqp_jvp(P, q, l_min, l_max, x, dP=None, dq=None, dl_min=None, dl_max=None, layout=_capi.P_AUTO, return_steps=False,
              out=None, epsilon=1e-10, workspace=None):
    """dx (B,N,1) of the box QP's solution along (dP, dq, dl_min, dl_max)."""
    return _jvp(2, P, q, (l_min, l_max), x, (dP, dq, dl_min, dl_max), layout, return_steps, out, epsilon, workspace)


def signedboxqp_jvp(P, q, l_min, l_max, v, x, dP=None, dq=None, dl_min=None, dl_max=None, layout=_capi.P_AUTO,
                    return_steps=False, out=None, epsilon=1e-10, workspace=None):
    """dx (B,N,1) of the signed box QP's solution: boxqp_jvp at the effective bounds, the bound tangents masked where the sign
    constraint has replaced the bound; v takes no tangent."""
    return _jvp(3, P, q, (l_min, l_max, v), x, (dP, dq, dl_min, dl_max), layout, return_steps, out, epsilon, workspace)


def _inf_layout(kind, layout, infinite_bounds):
    """layout with DQQ_F_INFINITE_BOUNDS for the box kinds (2, 3) of the Newton family when asked for: l_min = -inf and
    l_max = +inf are then ordinary input (include/diffqcqp_hip.h).  The other kinds have no bounds: nothing is added."""
    return layout | _capi.F_INFINITE_BOUNDS if infinite_bounds and kind >= 2 else layout


def _scratch(group, device, kind, N, B, layout=_capi.P_DENSE, given=None):
    """The scratch of a Newton-family call -- group "polish", "newton" or "newton_jac": dqq_<group>_scratch_bytes asks, and
    ops.<group>_workspace is the public constructor -- as an int32 tensor, uninitialised (the kernels initialise what they read);
    None where the call needs none: up to N = 64, and on DQQ_P_DIAG.  given: the caller's `workspace=`, checked for size and
    returned instead of a tensor allocated for this call; a call that is captured into a HIP graph must pass one and keep it
    alive as long as the graph."""
    if N <= 64 or (layout & 0xff) == _capi.P_DIAG:
        return None
    need = getattr(_capi.lib(), "dqq_%s_scratch_bytes" % group)(int(kind), int(N), int(B))
    if given is None:
        return torch.empty((need + 3) // 4, dtype=torch.int32, device=device) if need else None
    if not (given.is_cuda and given.is_contiguous() and given.numel() * given.element_size() >= need):
        raise ValueError("workspace must be a contiguous GPU tensor of at least %d bytes (ops.%s_workspace)" % (need, group))
    return given


def polish_workspace(device, kind, N, B):
    """The scratch a polish of (kind, N, B) needs (_scratch) for the `workspace=` argument of the polish ops, or None."""
    return _scratch("polish", device, kind, N, B)


def newton_workspace(device, kind, N, B):
    """The scratch a Newton derivative of (kind, N, B) needs (_scratch) for the `workspace=` argument of the newton ops, or None."""
    return _scratch("newton", device, kind, N, B)


def newton_jac_workspace(device, kind, N, B):
    """The scratch the Newton Jacobians of (kind, N, B) need (_scratch) for the `workspace=` argument of the newton_jacobian ops,
    or None."""
    return _scratch("newton_jac", device, kind, N, B)


def _ws_tail(ws, dev):
    """What every Newton-family entry ends in: (workspace, workspace_bytes, stream)."""
    return _ptr(ws), ws.numel() * ws.element_size() if ws is not None else 0, _raw_stream(dev.index)


def _newton_open(kind, P, q, extras, x, layout, infinite_bounds, polish_out=None):
    """The opening of every Newton-family op, in this order: the layout with _inf_layout's flag, the sizes, P, q and x prepared
    (_prep), then the kind's extras, padded with None to the three the C entries take.  polish_out: _polish's `out`, which may be
    x itself (in place); the same memory under another tensor is in place too, a partial overlap is refused -- before the extras
    are looked at.  -> layout, B, N, pshape, eshape (the extras' shape), P, q, extras, x, the device."""
    names, per_contact = _KIND[kind][0], _KIND[kind][1]
    layout = _inf_layout(kind, layout, infinite_bounds)
    B, N, pshape = _dims(P, q, layout)
    P, q = _prep(P, "P", pshape), _prep(q, "q", (B, N, 1))
    if polish_out is not None and polish_out is x:
        x = _out(polish_out, (B, N, 1), "out")
    else:
        x = _prep(x, "x", (B, N, 1))
        if polish_out is not None and B > 0:
            lo, span = _out(polish_out, (B, N, 1), "out").data_ptr(), 8 * B * N
            if lo != x.data_ptr() and lo < x.data_ptr() + span and x.data_ptr() < lo + span:
                raise ValueError("out overlaps x without being x (include/diffqcqp_hip.h: dqq_polish_f64): problems would read "
                                 "rows that others have already written")
    eshape = (B, N // 2, 1) if per_contact else (B, N, 1)
    extras = [_prep(e, n, eshape) for e, n in zip(extras, names)] + [None] * (3 - len(names))   # (held until the call)
    return layout, B, N, pshape, eshape, P, q, extras, x, q.device


def _grad_buffers(kind, need, out, pshape, B, N, eshape, dev):
    """(gP, gq, ga, gb) of a backward: the caller's `out` checked (_out), or fresh tensors where `need` says so; None where not
    needed, and ga, gb always None for the QP."""
    ga = gb = None
    if out is not None:
        gP, gq = _out(out[0], pshape, "out[0]"), _out(out[1], (B, N, 1), "out[1]")
        if kind:
            ga, gb = _out(out[2], eshape, "out[2]"), _out(out[3], eshape, "out[3]")
    else:
        gP = torch.empty(pshape, dtype=torch.float64, device=dev) if need[0] else None
        gq = torch.empty((B, N, 1), dtype=torch.float64, device=dev) if need[1] else None
        if kind:
            ga = torch.empty(eshape, dtype=torch.float64, device=dev) if need[2] else None
            gb = torch.empty(eshape, dtype=torch.float64, device=dev) if need[3] else None
    return gP, gq, ga, gb


def _tangents(kind, tangents, pshape, B, N, eshape):
    """The four tangents (dP, dq, da, db) of a forward-mode call, prepared (_prep) in their inputs' shapes; None stays None, a
    short tuple is padded, and the QP takes the first two only."""
    tangents = tuple(tangents) + (None,) * (4 - len(tangents))
    if kind == 0 and (tangents[2] is not None or tangents[3] is not None):
        raise ValueError("the QP has no extra inputs: tangents is (dP, dq)")
    shapes = (pshape, (B, N, 1), eshape, eshape)
    tn = ("dP", "dq") + tuple("d" + n for n in _KIND[kind][0][:2]) + ("", "")
    return [None if t is None else _prep(t, tn[i], shapes[i]) for i, t in enumerate(tangents[:4])]


def _reg(reg):
    """The proximal weight of a Newton-family call as the C entry takes it: a finite float >= 0 (csrc/polish_core.h)."""
    reg = float(reg)
    if not (0.0 <= reg < float("inf")):
        raise ValueError("reg must be finite and >= 0, got %r" % (reg,))
    return reg


def _reg_entry(stem, reg):
    """-> (the C entry, its name, the arguments that follow p_layout): the parent entry for reg = 0 -- the call it always was --,
    the *_reg_f64 entry with `reg` otherwise."""
    name = stem + ("_reg_f64" if reg else "_f64")
    return getattr(_capi.lib(), name), name, ((reg,) if reg else ())


def _kappa(kappa):
    """The smoothing parameter of a Newton-family call as the C entries take it: a finite float >= 0 (csrc/smooth_core.h)."""
    kappa = float(kappa)
    if not (0.0 <= kappa < float("inf")):
        raise ValueError("kappa must be finite and >= 0, got %r" % (kappa,))
    return kappa


def _smooth_entry(stem, reg, kappa, infinite_bounds):
    """_reg_entry for an op that also takes kappa: kappa = 0 is the call it always was; otherwise the *_smooth_f64 entry with
    (reg, kappa).  One-sided boxes are not admitted under smoothing."""
    if not kappa:
        return _reg_entry(stem, reg)
    if infinite_bounds:
        raise ValueError("infinite_bounds is not supported with kappa > 0 (include/diffqcqp_hip.h: one-sided boxes under smoothing)")
    name = stem + "_smooth_f64"
    return getattr(_capi.lib(), name), name, (reg, kappa)


def _halvings(max_halvings):
    """The cap on step halvings of a damped polish as the C entry takes it: an integer in 0 .. 60 (csrc/route.h)."""
    if int(max_halvings) != max_halvings or not 0 <= max_halvings <= 60:
        raise ValueError("max_halvings must be an integer in 0 .. 60, got %r" % (max_halvings,))
    return int(max_halvings)


def _polish(kind, P, q, extras, x, max_steps=8, layout=_capi.P_AUTO, out=None, return_info=False, workspace=None,
            infinite_bounds=False, reg=0.0, max_halvings=0, halvings=None, kappa=0.0, scaling=None):
    """The polish of every kind (include/diffqcqp_hip.h: dqq_polish_f64): up to max_steps Newton steps on the natural residual
    from x, each kept only if it lowers the residual.  -> x_out (B,N,1); with return_info also (resid (B,2) float64: the
    residual before and after, steps (B) int32: accepted steps, status (B) int32: 0 improved / 1 x kept / 2 not finite).
    out: the buffer to write into; may be x itself (in place, _newton_open).  workspace: the scratch, from polish_workspace
    (_scratch).  infinite_bounds: the box kinds take one-sided boxes (_inf_layout); without it an infinite bound is status 2.
    reg: the proximal weight (dqq_polish_reg_f64): the step solves with P + reg I in M, acceptance stays on the true residual;
    for a positive semidefinite P and reg > 0 no step fails on a singular free block.  0.0: dqq_polish_f64's kernels and bits.
    A launch argument: a captured call replays with the reg it was captured with.  max_halvings: the damped
    polish (dqq_polish_ls_f64): a step that does not lower the residual is retried at half its length, up to max_halvings times,
    before the problem gives up -- what makes the polish work from a rough or cold start; 0 (default): full steps only, the
    entries and bits above.  halvings: an int32 (B) GPU tensor that receives, per problem, the rejected trial points before its
    accepted steps (zeros at max_halvings = 0).  kappa: the smoothed polish (dqq_polish_smooth_f64, csrc/smooth_core.h): the
    residual driven down is that of the central-path equation x = PI_kappa(x - (P x + q)); resid and status are its; x_out is the
    point to hand to the newton ops with the same kappa.  0.0 (default): the calls above.  scaling: None (default: the calls
    above) or "pow2": equilibrate (x as the start point, in the scaled units), polish the scaled problem, unscale -- the scaled
    merit max |F~| weighs coordinate i by 2^-e_i, another merit function for the damped step.  resid and status
    are those of the SCALED problem; x_out is in the caller's units.  reg and kappa then act on the scaled problem too."""
    if _scaling(scaling) is not None:
        Pt, qt, ext, x0t, e = equilibrate(kind, P, q, extras, x, layout)
        res = _polish(kind, Pt, qt, ext, x0t, max_steps, layout, x0t, return_info, workspace, infinite_bounds, reg, max_halvings,
                      halvings, kappa)
        y = res[0] if return_info else res
        xo = unscale(y, e, out=y if out is None else out)
        return (xo,) + tuple(res[1:]) if return_info else xo
    reg, max_halvings, kappa = _reg(reg), _halvings(max_halvings), _kappa(kappa)
    smooth = _smooth_entry("dqq_polish", reg, kappa, infinite_bounds) if kappa else None   # (refuses one-sided boxes first)
    layout, B, N, _, _, P, q, extras, x, dev = _newton_open(kind, P, q, extras, x, layout, infinite_bounds, out)
    xo = _out(out, (B, N, 1), "out") if out is not None else torch.empty((B, N, 1), dtype=torch.float64, device=dev)
    resid = steps = status = None
    if return_info:
        resid = torch.empty((B, 2), dtype=torch.float64, device=dev)
        steps = torch.empty(B, dtype=torch.int32, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
    ws = _scratch("polish", dev, kind, N, B, layout, workspace)
    if halvings is not None and not (halvings.is_cuda and halvings.dtype is torch.int32 and halvings.is_contiguous() and
                                     tuple(halvings.shape) == (B,)):
        raise ValueError("halvings must be a contiguous int32 GPU tensor of shape (%d,)" % B)
    with _device_guard(dev):
        if kappa:
            fn, name, mid = smooth
            mid, tail = mid + (max_halvings,), (_ptr(halvings),)
        elif max_halvings:
            fn, name, mid, tail = _capi.lib().dqq_polish_ls_f64, "dqq_polish_ls_f64", (reg, max_halvings), (_ptr(halvings),)
        else:
            fn, name, mid = _reg_entry("dqq_polish", reg)
            tail = ()
            if halvings is not None:
                halvings.zero_()
        rc = fn(kind, P.data_ptr(), q.data_ptr(), *map(_ptr, extras), x.data_ptr(), xo.data_ptr(), B, N, int(max_steps), layout, *mid,
                _ptr(resid), _ptr(steps), _ptr(status), *tail, *_ws_tail(ws, dev))
    _capi.check(rc, name)
    return (xo, resid, steps, status) if return_info else xo


def qp_polish(P, q, x, max_steps=8, layout=_capi.P_AUTO, out=None, return_info=False, workspace=None, reg=0.0, max_halvings=0,
              halvings=None, kappa=0.0, scaling=None):
    """Polish an approximate QP solution x (B,N,1) -> x_out (see _polish)."""
    return _polish(0, P, q, (), x, max_steps, layout, out, return_info, workspace, reg=reg, max_halvings=max_halvings, halvings=halvings,
                   kappa=kappa, scaling=scaling)


def qcqp_polish(P, q, l_n, mu, x, max_steps=8, layout=_capi.P_AUTO, out=None, return_info=False, workspace=None, reg=0.0,
                max_halvings=0, halvings=None, kappa=0.0, scaling=None):
    """Polish an approximate QCQP solution x (B,N,1) -> x_out (see _polish)."""
    return _polish(1, P, q, (l_n, mu), x, max_steps, layout, out, return_info, workspace, reg=reg, max_halvings=max_halvings,
                   halvings=halvings, kappa=kappa, scaling=scaling)


def boxqp_polish(P, q, l_min, l_max, x, max_steps=8, layout=_capi.P_AUTO, out=None, return_info=False, workspace=None, v=None,
                 infinite_bounds=False, reg=0.0, max_halvings=0, halvings=None, kappa=0.0, scaling=None):
    """Polish an approximate box QP solution x (B,N,1) -> x_out; with `v` the signed box QP's (see _polish)."""
    kind, extras = (2, (l_min, l_max)) if v is None else (3, (l_min, l_max, v))
    return _polish(kind, P, q, extras, x, max_steps, layout, out, return_info, workspace, infinite_bounds, reg, max_halvings, halvings,
                   kappa, scaling)


PATH_KAPPAS = (1e-1, 1e-2, 1e-3, 1e-4, 0.0)   # the default schedule of the polish path ...
PATH_STEPS = (4, 4, 4, 4, 60)                 # ... and its per-stage step budgets
PATH_MAX_STAGES = 8


def _schedule(kappas, stage_steps):
    """The schedule of a polish path as the C entry takes it: (kappas, stage_steps, S) with the two as ctypes HOST arrays (the
    entry copies them into the launch; they only have to live until it returns).  1 .. 8 stages, every kappa finite and >= 0,
    every budget an integer >= 0."""
    kappas, stage_steps = tuple(kappas), tuple(stage_steps)
    S = len(kappas)
    if not 1 <= S <= PATH_MAX_STAGES or len(stage_steps) != S:
        raise ValueError("kappas and stage_steps must have the same length, 1 .. %d, got %d and %d" % (PATH_MAX_STAGES, S, len(stage_steps)))
    kappas = tuple(_kappa(k) for k in kappas)
    for n in stage_steps:
        if int(n) != n or n < 0:
            raise ValueError("stage_steps must be integers >= 0, got %r" % (stage_steps,))
    return (ctypes.c_double * S)(*kappas), (ctypes.c_int * S)(*(int(n) for n in stage_steps)), S


def _polish_path(kind, P, q, extras, x, kappas=PATH_KAPPAS, stage_steps=PATH_STEPS, max_halvings=8, reg=0.0, layout=_capi.P_AUTO,
                 out=None, return_info=False, workspace=None, scaling=None):
    """The polish path of every kind (include/diffqcqp_hip.h: dqq_polish_path_f64): the chain of smoothed damped polishes
    (_polish with kappa = kappas[s], max_steps = stage_steps[s], the same reg and max_halvings, each from the last one's x_out),
    bit for bit, in one launch.  The default schedule from the cold start x = PI(0) is a solver of its own: continuation in kappa
    reaches the solution where the hard damped polish alone stops short.  -> x_out (B,N,1); with return_info also (resid (B,2):
    stage 0's r before and the last stage's r after, each in its own kappa; steps (B) int32: accepted steps over all stages;
    status (B) int32: 0 moved / 1 x kept / 2 not finite; halvings (B) int32: rejected trial points before accepted steps;
    stage_resid (B,S,2) and stage_steps (B,S): each stage's own resid and steps).  out, workspace: as _polish's.  The schedule is
    a launch argument: a captured call replays the schedule it was captured with.  scaling="pow2": equilibrate (x as the start
    point), run the path on the scaled problem, unscale -- as _polish's; the residuals and status are the scaled problem's."""
    if _scaling(scaling) is not None:
        Pt, qt, ext, x0t, e = equilibrate(kind, P, q, extras, x, layout)
        res = _polish_path(kind, Pt, qt, ext, x0t, kappas, stage_steps, max_halvings, reg, layout, x0t, return_info, workspace)
        y = res[0] if return_info else res
        xo = unscale(y, e, out=y if out is None else out)
        return (xo,) + tuple(res[1:]) if return_info else xo
    reg, max_halvings = _reg(reg), _halvings(max_halvings)
    ks, ns, S = _schedule(kappas, stage_steps)
    layout, B, N, _, _, P, q, extras, x, dev = _newton_open(kind, P, q, extras, x, layout, False, out)
    xo = _out(out, (B, N, 1), "out") if out is not None else torch.empty((B, N, 1), dtype=torch.float64, device=dev)
    info = (None,) * 6
    if return_info:
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)   # noqa: E731
        info = (torch.empty((B, 2), dtype=torch.float64, device=dev), i32(B), i32(B), i32(B),
                torch.empty((B, S, 2), dtype=torch.float64, device=dev), i32(B, S))
    ws = _scratch("polish", dev, kind, N, B, layout, workspace)
    with _device_guard(dev):
        rc = _capi.lib().dqq_polish_path_f64(kind, P.data_ptr(), q.data_ptr(), *map(_ptr, extras), x.data_ptr(), xo.data_ptr(), B, N,
                                             layout, reg, ctypes.addressof(ks), ctypes.addressof(ns), S, max_halvings,
                                             *map(_ptr, info), *_ws_tail(ws, dev))
    _capi.check(rc, "dqq_polish_path_f64")
    return (xo,) + info if return_info else xo


def qp_polish_path(P, q, x, kappas=PATH_KAPPAS, stage_steps=PATH_STEPS, max_halvings=8, reg=0.0, layout=_capi.P_AUTO, out=None,
                   return_info=False, workspace=None, scaling=None):
    """The polish path of a QP from x (B,N,1) -> x_out (see _polish_path)."""
    return _polish_path(0, P, q, (), x, kappas, stage_steps, max_halvings, reg, layout, out, return_info, workspace, scaling)


def qcqp_polish_path(P, q, l_n, mu, x, kappas=PATH_KAPPAS, stage_steps=PATH_STEPS, max_halvings=8, reg=0.0, layout=_capi.P_AUTO,
                     out=None, return_info=False, workspace=None, scaling=None):
    """The polish path of a QCQP from x (B,N,1) -> x_out (see _polish_path)."""
    return _polish_path(1, P, q, (l_n, mu), x, kappas, stage_steps, max_halvings, reg, layout, out, return_info, workspace, scaling)


def boxqp_polish_path(P, q, l_min, l_max, x, kappas=PATH_KAPPAS, stage_steps=PATH_STEPS, max_halvings=8, reg=0.0,
                      layout=_capi.P_AUTO, out=None, return_info=False, workspace=None, scaling=None, v=None):
    """The polish path of a box QP from x (B,N,1) -> x_out; with `v` the signed box QP's (see _polish_path)."""
    kind, extras = (2, (l_min, l_max)) if v is None else (3, (l_min, l_max, v))
    return _polish_path(kind, P, q, extras, x, kappas, stage_steps, max_halvings, reg, layout, out, return_info, workspace, scaling)


def cold_start(kind, q, extras):
    """x = PI(0) (B,N,1) on the kind's effective bounds: 0 for the QP and the QCQP, the point of [l_min, l_max] nearest 0 for the
    box QP, and the same on the bounds the sign constraint leaves (csrc/sbox_bounds.h) for the signed box QP.  Torch ops."""
    x = torch.zeros_like(q)
    if kind < 2:
        return x
    lo, hi = extras[0], extras[1]
    if kind == 3:
        v, zero = extras[2], torch.zeros_like(q)
        hi_p = torch.where(hi < 0, hi, zero)
        lo_p = torch.where(lo < hi_p, lo, hi_p)
        lo_n = torch.where(lo > 0, lo, zero)
        hi_n = torch.where(hi > lo_n, hi, lo_n)
        lo = torch.where(v > 0, lo_p, torch.where(v < 0, lo_n, zero))
        hi = torch.where(v > 0, hi_p, torch.where(v < 0, hi_n, zero))
    return torch.where(lo > 0, lo, torch.where(hi < 0, hi, x))


def _newton_backward(kind, P, q, extras, x, grad_x, need=(True, True, True, True), layout=_capi.P_AUTO, out=None,
                     return_status=False, workspace=None, infinite_bounds=False, reg=0.0, kappa=0.0):
    """The exact backward of every kind from the polish's Jacobian (include/diffqcqp_hip.h: dqq_newton_bwd_f64): no epsilon, no
    refinement, one elimination per problem at the x given.  need / out: one entry per gradient output -- P, q and, but for the
    QP, the kind's first two extras.  -> the gradients (None where not needed), then status (B) int32 if asked for (0 done /
    1 singular / 2 not finite; 1 and 2: the problem's gradients are NaN).  workspace: the scratch, from newton_workspace
    (_scratch).  infinite_bounds: as _polish's; the gradient of an infinite bound is +0.0.  reg: the proximal weight
    (dqq_newton_bwd_reg_f64): the elimination is M_reg's, M_reg = (I - D) + D (P + reg I) -- the derivative of one
    proximal-point step at x, finite on a positive semidefinite P; 0.0: dqq_newton_bwd_f64's kernels and bits.  kappa: the
    smoothed backward (dqq_newton_bwd_smooth_f64, csrc/smooth_core.h): D and E of the smoothed projection, so inactive bounds and
    radii get gradients that are not zero; meant at the point the polish with the same kappa returns.  0.0: the calls above."""
    reg, kappa = _reg(reg), _kappa(kappa)
    layout, B, N, pshape, eshape, P, q, extras, x, dev = _newton_open(kind, P, q, extras, x, layout, infinite_bounds)
    grad_x = _prep(grad_x, "grad_x", (B, N, 1))
    gP, gq, ga, gb = _grad_buffers(kind, need, out, pshape, B, N, eshape, dev)
    status = torch.empty(B, dtype=torch.int32, device=dev) if return_status else None
    ws = _scratch("newton", dev, kind, N, B, layout, workspace)
    with _device_guard(dev):
        fn, name, mid = _smooth_entry("dqq_newton_bwd", reg, kappa, infinite_bounds)
        rc = fn(kind, P.data_ptr(), q.data_ptr(), *map(_ptr, extras), x.data_ptr(), grad_x.data_ptr(), _ptr(gP), _ptr(gq), _ptr(ga),
                _ptr(gb), B, N, layout, *mid, _ptr(status), *_ws_tail(ws, dev))
    _capi.check(rc, name)
    grads = (gP, gq, ga, gb) if kind else (gP, gq)
    return grads + (status,) if return_status else grads


def _newton_jvp(kind, P, q, extras, x, tangents, layout=_capi.P_AUTO, out=None, return_status=False, workspace=None,
                infinite_bounds=False, reg=0.0, kappa=0.0):
    """The exact forward-mode derivative of every kind (dqq_newton_jvp_f64): the transpose of _newton_backward to rounding.
    tangents: as _jvp's.  -> dx (B,N,1), then status (B) int32 if asked for.  infinite_bounds: as _polish's; the tangents stay
    finite-only, the one of an infinite bound takes no part.  reg: as _newton_backward's (dqq_newton_jvp_reg_f64); both modes
    share M_reg and stay adjoint to rounding.  kappa: as _newton_backward's (dqq_newton_jvp_smooth_f64)."""
    reg, kappa = _reg(reg), _kappa(kappa)
    layout, B, N, pshape, eshape, P, q, extras, x, dev = _newton_open(kind, P, q, extras, x, layout, infinite_bounds)
    tangents = _tangents(kind, tangents, pshape, B, N, eshape)
    dx = _out(out, (B, N, 1), "out") if out is not None else torch.empty((B, N, 1), dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev) if return_status else None
    ws = _scratch("newton", dev, kind, N, B, layout, workspace)
    with _device_guard(dev):
        fn, name, mid = _smooth_entry("dqq_newton_jvp", reg, kappa, infinite_bounds)
        rc = fn(kind, P.data_ptr(), q.data_ptr(), *map(_ptr, extras), x.data_ptr(), *map(_ptr, tangents), dx.data_ptr(), B, N, layout,
                *mid, _ptr(status), *_ws_tail(ws, dev))
    _capi.check(rc, name)
    return (dx, status) if return_status else dx


def qp_newton_backward(P, q, x, grad_x, need_P=True, need_q=True, layout=_capi.P_AUTO, out=None, return_status=False,
                       workspace=None, reg=0.0, kappa=0.0):
    """Exact backward of the QP at x -> (grad_P|None, grad_q|None) (see _newton_backward)."""
    return _newton_backward(0, P, q, (), x, grad_x, (need_P, need_q), layout, out, return_status, workspace, reg=reg, kappa=kappa)


def qcqp_newton_backward(P, q, l_n, mu, x, grad_x, need=(True, True, True, True), layout=_capi.P_AUTO, out=None,
                         return_status=False, workspace=None, reg=0.0, kappa=0.0):
    """Exact backward of the QCQP at x -> (grad_P, grad_q, grad_l_n, grad_mu), None where not needed."""
    return _newton_backward(1, P, q, (l_n, mu), x, grad_x, need, layout, out, return_status, workspace, reg=reg, kappa=kappa)


def boxqp_newton_backward(P, q, l_min, l_max, x, grad_x, need=(True, True, True, True), layout=_capi.P_AUTO, out=None,
                          return_status=False, workspace=None, infinite_bounds=False, reg=0.0, kappa=0.0):
    """Exact backward of the box QP at x -> (grad_P, grad_q, grad_l_min, grad_l_max), None where not needed."""
    return _newton_backward(2, P, q, (l_min, l_max), x, grad_x, need, layout, out, return_status, workspace, infinite_bounds,
                            reg, kappa=kappa)


def signedboxqp_newton_backward(P, q, l_min, l_max, v, x, grad_x, need=(True, True, True, True), layout=_capi.P_AUTO, out=None,
                                return_status=False, workspace=None, infinite_bounds=False, reg=0.0, kappa=0.0):
    """Exact backward of the signed box QP at x: the box QP's on the effective bounds, the bound gradients +0.0 where the sign
    constraint has replaced the bound; v gets none."""
    return _newton_backward(3, P, q, (l_min, l_max, v), x, grad_x, need, layout, out, return_status, workspace,
                            infinite_bounds, reg, kappa=kappa)


def qp_newton_jvp(P, q, x, dP=None, dq=None, layout=_capi.P_AUTO, out=None, return_status=False, workspace=None, reg=0.0, kappa=0.0):
    """Exact dx (B,N,1) of the QP's solution along (dP, dq); None = a zero tangent."""
    return _newton_jvp(0, P, q, (), x, (dP, dq), layout, out, return_status, workspace, reg=reg, kappa=kappa)


def qcqp_newton_jvp(P, q, l_n, mu, x, dP=None, dq=None, dl_n=None, dmu=None, layout=_capi.P_AUTO, out=None, return_status=False,
                    workspace=None, reg=0.0, kappa=0.0):
    """Exact dx (B,N,1) of the QCQP's solution along (dP, dq, dl_n, dmu)."""
    return _newton_jvp(1, P, q, (l_n, mu), x, (dP, dq, dl_n, dmu), layout, out, return_status, workspace, reg=reg, kappa=kappa)


def boxqp_newton_jvp(P, q, l_min, l_max, x, dP=None, dq=None, dl_min=None, dl_max=None, layout=_capi.P_AUTO, out=None,
                     return_status=False, workspace=None, infinite_bounds=False, reg=0.0, kappa=0.0):
    """Exact dx (B,N,1) of the box QP's solution along (dP, dq, dl_min, dl_max)."""
    return _newton_jvp(2, P, q, (l_min, l_max), x, (dP, dq, dl_min, dl_max), layout, out, return_status, workspace,
                       infinite_bounds, reg=reg, kappa=kappa)


def signedboxqp_newton_jvp(P, q, l_min, l_max, v, x, dP=None, dq=None, dl_min=None, dl_max=None, layout=_capi.P_AUTO, out=None,
                           return_status=False, workspace=None, infinite_bounds=False, reg=0.0, kappa=0.0):
    """Exact dx (B,N,1) of the signed box QP's solution; v takes no tangent."""
    return _newton_jvp(3, P, q, (l_min, l_max, v), x, (dP, dq, dl_min, dl_max), layout, out, return_status, workspace,
                       infinite_bounds, reg=reg, kappa=kappa)


def _jac_shapes(kind, B, N, layout):
    """Shapes of (Jq, Ja, Jb) as include/diffqcqp_hip.h has them."""
    if (layout & 0xff) == _capi.P_DIAG:
        return ((B, N, 2) if kind == 1 else (B, N), (B, N), (B, N))
    ne = N // 2 if _KIND[kind][1] else N
    return ((B, N, N), (B, N, ne), (B, N, ne))


def _newton_jacobian(kind, P, q, extras, x, need=(True, True, True), layout=_capi.P_AUTO, out=None, return_status=False,
                     workspace=None, infinite_bounds=False, reg=0.0, kappa=0.0):
    """The Jacobians of the solution map at x from one elimination per problem (include/diffqcqp_hip.h: dqq_newton_jac_f64):
    column j of Jq / Ja / Jb is _newton_jvp's dx for the unit tangent e_j of q / the kind's first / second extra, bit for bit.
    need / out: one entry per output -- Jq and, but for the QP, Ja and Jb.  (B,N,N) P: Jq (B,N,N), Jq[b,i,j] = dx_i/dq_j; Ja, Jb
    (B,N,N), the QCQP's (B,N,N/2).  DQQ_P_DIAG: the compact blocks -- Jq (B,N), the QCQP's (B,N,2); Ja, Jb (B,N).  dx/dP is
    Jq[i,j] x_k and is not materialised (newton_jacobian_jvp / _vjp apply it).  -> the Jacobians (None where not needed), then
    status (B) int32 if asked for (0 done / 1 singular / 2 not finite; 1 and 2: the problem's Jacobians are NaN).  workspace: the
    scratch, from newton_jac_workspace (_scratch).  infinite_bounds: as _polish's; the column of an infinite bound is zero.  reg: as
    _newton_backward's (dqq_newton_jac_reg_f64); each column keeps the bits of _newton_jvp at the same reg.  kappa: the smoothed
    Jacobians (dqq_newton_jac_smooth_f64, csrc/smooth_core.h): D and E of the smoothed projection, every column the bits of
    _newton_jvp at the same reg and kappa, so the column of an inactive bound or radius is not zero; meant at the point the polish
    with the same kappa returns.  0.0: the calls above.  infinite_bounds with kappa > 0 raises, as in the sibling ops."""
    reg, kappa = _reg(reg), _kappa(kappa)
    layout, B, N, _, _, P, q, extras, x, dev = _newton_open(kind, P, q, extras, x, layout, infinite_bounds)
    shapes = _jac_shapes(kind, B, N, layout)
    nout = 3 if kind else 1
    if out is not None:
        J = [_out(out[i], shapes[i], "out[%d]" % i) for i in range(nout)]
    else:
        need = tuple(need) + (True,) * (3 - len(need))
        J = [torch.empty(shapes[i], dtype=torch.float64, device=dev) if need[i] else None for i in range(nout)]
    J += [None] * (3 - nout)
    if all(j is None for j in J):
        raise ValueError("no Jacobian requested")
    status = torch.empty(B, dtype=torch.int32, device=dev) if return_status else None
    ws = _scratch("newton_jac", dev, kind, N, B, layout, workspace)
    with _device_guard(dev):
        fn, name, mid = _smooth_entry("dqq_newton_jac", reg, kappa, infinite_bounds)
        rc = fn(kind, P.data_ptr(), q.data_ptr(), *map(_ptr, extras), x.data_ptr(), *map(_ptr, J), B, N, layout, *mid, _ptr(status),
                *_ws_tail(ws, dev))
    _capi.check(rc, name)
    res = tuple(J[:nout])
    return res + (status,) if return_status else res


def qp_newton_jacobian(P, q, x, layout=_capi.P_AUTO, out=None, return_status=False, workspace=None, reg=0.0, kappa=0.0):
    """The QP's Jacobian at x -> (Jq,) (see _newton_jacobian)."""
    return _newton_jacobian(0, P, q, (), x, (True,), layout, out, return_status, workspace, reg=reg, kappa=kappa)


def qcqp_newton_jacobian(P, q, l_n, mu, x, need=(True, True, True), layout=_capi.P_AUTO, out=None, return_status=False,
                         workspace=None, reg=0.0, kappa=0.0):
    """The QCQP's Jacobians at x -> (Jq, Jl_n, Jmu), None where not needed."""
    return _newton_jacobian(1, P, q, (l_n, mu), x, need, layout, out, return_status, workspace, reg=reg, kappa=kappa)


def boxqp_newton_jacobian(P, q, l_min, l_max, x, need=(True, True, True), layout=_capi.P_AUTO, out=None, return_status=False,
                          workspace=None, infinite_bounds=False, reg=0.0, kappa=0.0):
    """The box QP's Jacobians at x -> (Jq, Jl_min, Jl_max), None where not needed."""
    return _newton_jacobian(2, P, q, (l_min, l_max), x, need, layout, out, return_status, workspace, infinite_bounds, reg, kappa)


def signedboxqp_newton_jacobian(P, q, l_min, l_max, v, x, need=(True, True, True), layout=_capi.P_AUTO, out=None,
                                return_status=False, workspace=None, infinite_bounds=False, reg=0.0, kappa=0.0):
    """The signed box QP's Jacobians at x: zero columns where the sign constraint has replaced the bound; v takes nothing."""
    return _newton_jacobian(3, P, q, (l_min, l_max, v), x, need, layout, out, return_status, workspace, infinite_bounds, reg, kappa)


ActiveSet = namedtuple("ActiveSet", "state mult margin where status")


def _newton_active(kind, P, q, extras, x, layout=_capi.P_AUTO, need=(True, True, True, True, True), infinite_bounds=False,
                   out=None):
    """The active set the Newton family works on at x, its multipliers and the distance to the nearest kink
    (include/diffqcqp_hip.h: dqq_newton_active_f64), one streaming launch on the current stream; no workspace on any route.
    -> ActiveSet(state int32 (B,N), the QCQP's (B,N/2): 0 free / inside, 1 on the caller's lower bound / sliding, 2 on the
    caller's upper bound, 3 on a constant / outside a disc of radius <= 0;  mult float64, as state: the multiplier, +0.0 where
    state is 0;  margin float64 (B): how far z = x - (P x + q) may move, in the max norm per element, before state changes;
    where int32 (B): the element that is nearest;  status int32 (B): 0 done / 2 not finite -- then state and where are -1, mult
    and margin NaN).  need / out: one entry per output, in that order; an output not needed (out: None) is None, the others have
    the same bits.  infinite_bounds: as _polish's; an infinite side takes no part in margin."""
    layout, B, N, _, eshape, P, q, extras, x, dev = _newton_open(kind, P, q, extras, x, layout, infinite_bounds)
    ne = eshape[1]
    specs = (((B, ne), torch.int32), ((B, ne), torch.float64), ((B,), torch.float64), ((B,), torch.int32), ((B,), torch.int32))
    if out is not None:
        res = list(out)
        for i, (t, (shape, dtype)) in enumerate(zip(res, specs)):
            if t is not None and not (t.is_cuda and t.dtype is dtype and t.is_contiguous() and tuple(t.shape) == shape):
                raise ValueError("out[%d] must be a contiguous %s GPU tensor of shape %s" % (i, dtype, shape))
    else:
        res = [torch.empty(shape, dtype=dtype, device=dev) if n else None for n, (shape, dtype) in zip(need, specs)]
    if len(res) != 5 or all(t is None for t in res):
        raise ValueError("no output requested")
    with _device_guard(dev):
        rc = _capi.lib().dqq_newton_active_f64(kind, P.data_ptr(), q.data_ptr(), *map(_ptr, extras), x.data_ptr(), *map(_ptr, res),
                                               B, N, layout, _raw_stream(dev.index))
    _capi.check(rc, "dqq_newton_active_f64")
    return ActiveSet(*res)


def qp_newton_active(P, q, x, layout=_capi.P_AUTO, need=(True, True, True, True, True), out=None):
    """The QP's active set, multipliers and kink margin at x -> ActiveSet (see _newton_active)."""
    return _newton_active(0, P, q, (), x, layout, need, False, out)


def qcqp_newton_active(P, q, l_n, mu, x, layout=_capi.P_AUTO, need=(True, True, True, True, True), out=None):
    """The QCQP's, per contact -> ActiveSet (see _newton_active)."""
    return _newton_active(1, P, q, (l_n, mu), x, layout, need, False, out)


def boxqp_newton_active(P, q, l_min, l_max, x, layout=_capi.P_AUTO, need=(True, True, True, True, True), infinite_bounds=False,
                        out=None):
    """The box QP's -> ActiveSet (see _newton_active)."""
    return _newton_active(2, P, q, (l_min, l_max), x, layout, need, infinite_bounds, out)


def signedboxqp_newton_active(P, q, l_min, l_max, v, x, layout=_capi.P_AUTO, need=(True, True, True, True, True),
                              infinite_bounds=False, out=None):
    """The signed box QP's, on its effective bounds: state 3 where the bound sat on is the sign constraint's 0."""
    return _newton_active(3, P, q, (l_min, l_max, v), x, layout, need, infinite_bounds, out)


def _jac_apply(kind, J, V, which, compact, transpose):
    """J (one of Jq, Ja, Jb) applied to K stacked vectors V (K,B,.,1): J V, or J' V with transpose.  No kernel of this package:
    torch.bmm on a general Jacobian, elementwise products on DQQ_P_DIAG's compact blocks."""
    K, B = V.shape[0], V.shape[1]
    if not compact:
        Jm = J.transpose(1, 2) if transpose else J
        return torch.bmm(Jm, V[:, :, :, 0].permute(1, 2, 0)).permute(2, 0, 1).unsqueeze(-1)
    N = J.shape[1]
    if kind != 1:
        return J.unsqueeze(0).unsqueeze(-1) * V
    if which == 0:   # (B,N,2): the 2 x 2 block of a contact, rows i = 2k, 2k+1
        blk = J.reshape(B, N // 2, 2, 2)
        if transpose:
            blk = blk.transpose(2, 3)
        v = V[:, :, :, 0].reshape(K, B, N // 2, 1, 2)
        return (blk.unsqueeze(0) * v).sum(-1).reshape(K, B, N, 1)
    if transpose:    # (B,N) of a per-contact extra: sum the contact's two rows
        return (J.unsqueeze(0) * V[:, :, :, 0]).reshape(K, B, N // 2, 2).sum(-1).unsqueeze(-1)
    return J.unsqueeze(0).unsqueeze(-1) * V.repeat_interleave(2, dim=2)


def newton_jacobian_jvp(kind, J, x, tangents, compact=None):
    """K tangents through the Jacobians J = (Jq[, Ja, Jb]) of _newton_jacobian at x (B,N,1): dx = Jq (dP x + dq) + Ja da + Jb db
    (K,B,N,1).  kind: 0..3 or "qp" / "qcqp" / "box" / "sbox"; tangents: (dP, dq[, da, db]), each (K,B,...) in its input's shape
    ((K,B,N) dP on DQQ_P_DIAG's compact Jacobians) or None.  compact: whether J holds DQQ_P_DIAG's compact blocks; None tells it
    from the shapes (_jac_is_compact), which cannot tell a QCQP at N = 2 with Jq alone -- (B,2,2) either way, and read as general
    there: pass compact=True with a (K,B,2) dP.  torch only: no kernel is launched here but torch's own.  Smoothed Jacobians
    (kappa > 0) go through unchanged: d x_i / d P_jk = Jq_ij x_k still holds, the smoothed JVP's right-hand side being
    -D (dP x + dq)."""
    kind = _KINDS.get(kind, kind)
    Jq = J[0]
    B, N = x.shape[0], x.shape[1]
    if compact is None:
        compact = _jac_is_compact(kind, J, N)
    tangents = tuple(tangents) + (None,) * (4 - len(tangents))
    dP, dq = tangents[0], tangents[1]
    t = None
    if dP is not None:
        t = (dP * x[:, :, 0].unsqueeze(0)).unsqueeze(-1) if dP.dim() == 3 else torch.matmul(dP, x.unsqueeze(0))
    if dq is not None:
        t = dq if t is None else t + dq
    dx = None
    if t is not None:
        if Jq is None:
            raise ValueError("dP and dq need Jq")
        dx = _jac_apply(kind, Jq, t, 0, compact, False)
    for which in (1, 2):
        d = tangents[1 + which]
        if d is not None:
            if kind == 0 or J[which] is None:
                raise ValueError("a tangent without its Jacobian")
            term = _jac_apply(kind, J[which], d, which, compact, False)
            dx = term if dx is None else dx + term
    return dx


def newton_jacobian_vjp(kind, J, x, grad_x, compact=None):
    """K cotangents grad_x (K,B,N,1) through the Jacobians J = (Jq[, Ja, Jb]) at x (B,N,1) -> (grad_P, grad_q[, grad_a, grad_b]),
    each (K,B,...) in its input's shape, None where its Jacobian is: grad_q = Jq' g, grad_P = (Jq' g) x' (DQQ_P_DIAG's compact
    Jacobians: (Jq' g)_i x_i, (K,B,N)), grad_a = Ja' g, grad_b = Jb' g.  compact: as newton_jacobian_jvp's (a QCQP at N = 2 with
    Jq alone needs compact=True for the compact grad_P).  torch only.  Smoothed Jacobians (kappa > 0) go through unchanged, as
    in newton_jacobian_jvp: the result is then ops.*_newton_backward(kappa=)'s to rounding."""
    kind = _KINDS.get(kind, kind)
    Jq = J[0]
    N = x.shape[1]
    if compact is None:
        compact = _jac_is_compact(kind, J, N)
    gP = gq = None
    if Jq is not None:
        gq = _jac_apply(kind, Jq, grad_x, 0, compact, True)
        gP = gq[:, :, :, 0] * x[:, :, 0].unsqueeze(0) if compact else gq * x[:, :, 0].unsqueeze(0).unsqueeze(2)
    if kind == 0:
        return gP, gq
    ga, gb = (None if J[w] is None else _jac_apply(kind, J[w], grad_x, w, compact, True) for w in (1, 2))
    return gP, gq, ga, gb


def _jac_is_compact(kind, J, N):
    """Whether J holds DQQ_P_DIAG's compact blocks: told from the shape of any Jacobian that is there -- (B,N) is compact, (B,N,N)
    and the QCQP's (B,N,N/2) are not; the QCQP's Jq (B,N,2) is compact but at N = 2, where (B,2,2) is both and the same matrix."""
    if all(j is None for j in J):
        raise ValueError("no Jacobian given")
    if any(j is not None and j.dim() == 2 for j in J):
        return True
    return kind == 1 and J[0] is not None and J[0].shape[2] == 2 and N != 2


def solution_check(kind, P, q, extras, x, iters=None, max_iter=None, layout=_capi.P_AUTO, out=None):
    """How each solve of a batch ended (include/diffqcqp_hip.h: dqq_check_f64): one streaming launch on the current stream,
    whatever route produced `x`.  kind: 0 / "qp", 1 / "qcqp", 2 / "box", 3 / "sbox"; extras: the kind's extra inputs in the
    forwards' order -- (), (l_n, mu), (l_min, l_max), (l_min, l_max, v).  iters / max_iter: the forward's `return_iters` output
    and its max_iter (both or neither).  layout: as the forward's; DQQ_P_DIAG reads P as (B,N).
    -> (status (B) int32: 0 converged / 1 stopped at max_iter / 2 not finite,
        resid (B,4) float64: natural residual, infeasibility, objective, scale,
        counts (3) int64: problems per status), on the device.
    out: optional (status, resid, counts) buffers to write into; counts is zeroed here."""
    k = _KINDS.get(kind, kind)
    if k not in (0, 1, 2, 3):
        raise ValueError("kind must be one of %s or 0..3 (got %r)" % (sorted(_KINDS), kind))
    B, N, pshape = _dims(P, q, layout)
    extras = tuple(extras or ())
    if len(extras) != len(_KIND[k][0]):
        raise ValueError("kind %r takes %d extra inputs (got %d)" % (kind, len(_KIND[k][0]), len(extras)))
    if (iters is None) != (max_iter is None):
        raise ValueError("iters and max_iter go together")
    P, q, x = _prep(P, "P", pshape), _prep(q, "q", (B, N, 1)), _prep(x, "x", (B, N, 1))
    eshape = (B, N // 2, 1) if _KIND[k][1] else (B, N, 1)
    extras = [_prep(e, _GENERIC_NAMES[i], eshape) for i, e in enumerate(extras)] + [None] * (3 - len(extras))
    dev = q.device
    if iters is not None and not (iters.is_cuda and iters.dtype is torch.int32 and iters.is_contiguous() and iters.numel() == B):
        raise ValueError("iters must be a contiguous int32 GPU tensor of %d entries" % B)
    if out is not None:
        status, resid, counts = out
        ok = (status.is_cuda and status.dtype is torch.int32 and status.is_contiguous() and tuple(status.shape) == (B,)
              and counts.is_cuda and counts.dtype is torch.int64 and counts.is_contiguous() and tuple(counts.shape) == (3,))
        if not ok:
            raise ValueError("out must be (int32 (B), float64 (B,4), int64 (3)) contiguous GPU tensors")
        _out(resid, (B, 4), "out[1]")
        counts.zero_()
    else:
        status = torch.empty(B, dtype=torch.int32, device=dev)
        resid = torch.empty((B, 4), dtype=torch.float64, device=dev)
        counts = torch.zeros(3, dtype=torch.int64, device=dev)
    with _device_guard(dev):
        rc = _capi.lib().dqq_check_f64(k, _ptr(P), _ptr(q), _ptr(extras[0]), _ptr(extras[1]), _ptr(extras[2]), _ptr(x),
                                       _ptr(iters), int(max_iter or 0), B, N, layout, _ptr(resid), _ptr(status),
                                       _ptr(counts), _raw_stream(dev.index))
    _capi.check(rc, "dqq_check_f64")
    return status, resid, counts
