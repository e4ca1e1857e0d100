"""Module-level numpy API with the names, argument order and keyword defaults of the reference's
pybind11 module `diffqcqp` (reference pybindings.cpp:74-83), for consumers that call the raw solver
instead of the autograd Functions:

    from diffqcqp_amd.diffqcqp import solveQP, solveQCQP, solveDerivativesQP, solveDerivativesQCQP
    from diffqcqp_amd.diffqcqp import solveBoxQP, solveSignedBoxQP, solveDerivativesBoxQP, solveDerivativesSignedBoxQP
    from diffqcqp_amd.diffqcqp import jvpQP, jvpQCQP, jvpBoxQP, jvpSignedBoxQP     # forward mode, an extension (end of file)

Each call solves ONE problem given as numpy arrays (vectors may be (N,) or (N,1), any float dtype --
converted to float64 like pybind11 does), on the GPU through the same C ABI as the batched path
(B = 1, host buffers staged over PCIe), and returns fresh numpy arrays shaped like the reference's:
`solveQP/solveQCQP -> (N,)`, `solveDerivativesQP -> (N,)`, `solveDerivativesQCQP -> (E1 (nc,nc),
E2 (nc,nc), blgamma (nc+N,))`, `solveBoxQP/solveSignedBoxQP -> (N,)`, `solveDerivativesBoxQP ->
(blgamma (3N,), gamma (2N,))`, `solveDerivativesSignedBoxQP` alike (the reference has no such function).  `warm_start` is accepted and ignored (dead in the reference).
The batched functions `*_batch` take stacked problems and are what you want for throughput.
"""
import numpy as np
import torch

from . import ops
from .qcqp import _device_for


def _dev():
    return _device_for(torch.empty(0))


def _t(a, shape, dev):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).reshape(shape).to(dev)


def solveQP(P, q, warm_start, epsilon=1e-10, mu_prox=1e-7, max_iter=1000, adaptative_rho=True):
    dev = _dev()
    n = np.asarray(q).size
    x = ops.qp_forward(_t(P, (1, n, n), dev), _t(q, (1, n, 1), dev), epsilon, max_iter, mu_prox,
                       adaptive_rho=adaptative_rho)
    return x.reshape(n).cpu().numpy()


def solveQCQP(P, q, l_n, mu, warm_start, epsilon=1e-10, mu_prox=1e-7, max_iter=1000, adaptative_rho=True):
    dev = _dev()
    n = np.asarray(q).size
    x = ops.qcqp_forward(_t(P, (1, n, n), dev), _t(q, (1, n, 1), dev), _t(l_n, (1, n // 2, 1), dev),
                         _t(mu, (1, n // 2, 1), dev), epsilon, max_iter, mu_prox, adaptive_rho=adaptative_rho)
    return x.reshape(n).cpu().numpy()


def solveDerivativesQP(P, q, l, grad_l, epsilon=1e-10):
    """-> bl (N,): the solution of the differentiated KKT system (grad_q = -bl, grad_P = -bl l^T)."""
    dev = _dev()
    n = np.asarray(q).size
    _, gq = ops.qp_backward(_t(P, (1, n, n), dev), _t(q, (1, n, 1), dev), _t(l, (1, n, 1), dev),
                            _t(grad_l, (1, n, 1), dev), need_P=False, need_q=True, epsilon=epsilon)
    return (-gq).reshape(n).cpu().numpy()


def solveDerivativesQCQP(P, q, l_n, mu, l, grad_l, epsilon=1e-10):
    """-> (E1, E2, blgamma) like pybindings.cpp:62-71: E1/E2 dense (nc,nc) diagonal matrices,
    blgamma = [dgamma (nc); dl (N)]."""
    dev = _dev()
    n = np.asarray(q).size
    nc = n // 2
    ln_t, mu_t = _t(l_n, (1, nc, 1), dev), _t(mu, (1, nc, 1), dev)
    gam = torch.empty((1, nc, 1), dtype=torch.float64, device=dev)
    dgam = torch.empty_like(gam)
    _, gq, _, _ = ops.qcqp_backward(_t(P, (1, n, n), dev), _t(q, (1, n, 1), dev), ln_t, mu_t, _t(l, (1, n, 1), dev),
                                    _t(grad_l, (1, n, 1), dev), need=(False, True, False, False), epsilon=epsilon,
                                    duals=(gam, dgam))
    g, ln1, mu1 = gam.reshape(nc).cpu().numpy(), ln_t.reshape(nc).cpu().numpy(), mu_t.reshape(nc).cpu().numpy()
    E1 = np.diag(2 * g * ln1 * ln1 * mu1)   # getE12QCQP, Solver.cpp:683-691
    E2 = np.diag(2 * g * ln1 * mu1 * mu1)
    blgamma = np.concatenate([dgam.reshape(nc).cpu().numpy(), (-gq).reshape(n).cpu().numpy()])
    return E1, E2, blgamma


def solveBoxQP(P, q, l_min, l_max, warm_start, epsilon=1e-10, mu_prox=1e-7, max_iter=1000, adaptative_rho=True):
    """pybindings.cpp:32-37, :77"""
    dev = _dev()
    n = np.asarray(q).size
    x = ops.boxqp_forward(_t(P, (1, n, n), dev), _t(q, (1, n, 1), dev), _t(l_min, (1, n, 1), dev),
                          _t(l_max, (1, n, 1), dev), epsilon, max_iter, mu_prox=mu_prox, adaptive_rho=adaptative_rho)
    return x.reshape(n).cpu().numpy()


def solveSignedBoxQP(P, q, l_min, l_max, v, warm_start, epsilon=1e-10, mu_prox=1e-7, max_iter=1000,
                     adaptative_rho=True):
    """pybindings.cpp:47-52, :78"""
    dev = _dev()
    n = np.asarray(q).size
    x = ops.boxqp_forward(_t(P, (1, n, n), dev), _t(q, (1, n, 1), dev), _t(l_min, (1, n, 1), dev),
                          _t(l_max, (1, n, 1), dev), epsilon, max_iter, v=_t(v, (1, n, 1), dev), mu_prox=mu_prox,
                          adaptive_rho=adaptative_rho)
    return x.reshape(n).cpu().numpy()


def solveDerivativesBoxQP(P, q, l_min, l_max, l, grad_l, epsilon=1e-10):
    """-> (blgamma (3N,), gamma (2N,)) like pybindings.cpp:39-45: blgamma = [dgamma_lower (N); dgamma_upper (N);
    dl (N)], gamma = [lower multipliers (N); upper multipliers (N)]."""
    dev = _dev()
    n = np.asarray(q).size
    gam = torch.empty((1, 2 * n), dtype=torch.float64, device=dev)
    dgam = torch.empty_like(gam)
    _, gq, _, _ = ops.boxqp_backward(_t(P, (1, n, n), dev), _t(q, (1, n, 1), dev), _t(l_min, (1, n, 1), dev),
                                     _t(l_max, (1, n, 1), dev), _t(l, (1, n, 1), dev), _t(grad_l, (1, n, 1), dev),
                                     need=(False, True, False, False), epsilon=epsilon, duals=(gam, dgam))
    blgamma = np.concatenate([dgam.reshape(2 * n).cpu().numpy(), (-gq).reshape(n).cpu().numpy()])
    return blgamma, gam.reshape(2 * n).cpu().numpy()


def solveDerivativesSignedBoxQP(P, q, l_min, l_max, v, l, grad_l, epsilon=1e-10):
    """The twin of solveDerivativesBoxQP for the signed box QP (no counterpart in the reference): -> (blgamma (3N,),
    gamma (2N,)), the multipliers being those of the effective bounds the sign constraint leaves
    (include/diffqcqp_hip.h: dqq_signedboxqp_bwd_f64)."""
    dev = _dev()
    n = np.asarray(q).size
    gam = torch.empty((1, 2 * n), dtype=torch.float64, device=dev)
    dgam = torch.empty_like(gam)
    _, gq, _, _ = ops.boxqp_backward(_t(P, (1, n, n), dev), _t(q, (1, n, 1), dev), _t(l_min, (1, n, 1), dev),
                                     _t(l_max, (1, n, 1), dev), _t(l, (1, n, 1), dev), _t(grad_l, (1, n, 1), dev),
                                     need=(False, True, False, False), epsilon=epsilon, duals=(gam, dgam),
                                     v=_t(v, (1, n, 1), dev))
    blgamma = np.concatenate([dgam.reshape(2 * n).cpu().numpy(), (-gq).reshape(n).cpu().numpy()])
    return blgamma, gam.reshape(2 * n).cpu().numpy()


# ---- forward-mode twins (an extension: the reference differentiates in reverse mode only) ------------------------------------
# One problem; `l` is the solution; a tangent left out (None) is zero.  -> dl (N,), the directional derivative of the solution
# (include/diffqcqp_hip.h: dqq_jvp_f64, the exact transpose of the solveDerivatives* call above it).
def _tan(a, shape, dev):
    return None if a is None else _t(a, shape, dev)


def jvpQP(P, q, l, dP=None, dq=None, epsilon=1e-10):
    dev = _dev()
    n = np.asarray(q).size
    dl = ops.qp_jvp(_t(P, (1, n, n), dev), _t(q, (1, n, 1), dev), _t(l, (1, n, 1), dev), _tan(dP, (1, n, n), dev),
                    _tan(dq, (1, n, 1), dev), epsilon=epsilon)
    return dl.reshape(n).cpu().numpy()


def jvpQCQP(P, q, l_n, mu, l, dP=None, dq=None, dl_n=None, dmu=None, epsilon=1e-10):
    dev = _dev()
    n = np.asarray(q).size
    nc = n // 2
    dl = ops.qcqp_jvp(_t(P, (1, n, n), dev), _t(q, (1, n, 1), dev), _t(l_n, (1, nc, 1), dev), _t(mu, (1, nc, 1), dev),
                      _t(l, (1, n, 1), dev), _tan(dP, (1, n, n), dev), _tan(dq, (1, n, 1), dev), _tan(dl_n, (1, nc, 1), dev),
                      _tan(dmu, (1, nc, 1), dev), epsilon=epsilon)
    return dl.reshape(n).cpu().numpy()


def jvpBoxQP(P, q, l_min, l_max, l, dP=None, dq=None, dl_min=None, dl_max=None, epsilon=1e-10, v=None):
    """With `v` the signed box QP's (jvpSignedBoxQP)."""
    dev = _dev()
    n = np.asarray(q).size
    extras = (_t(l_min, (1, n, 1), dev), _t(l_max, (1, n, 1), dev)) + (() if v is None else (_t(v, (1, n, 1), dev),))
    dl = ops._jvp(2 if v is None else 3, _t(P, (1, n, n), dev), _t(q, (1, n, 1), dev), extras, _t(l, (1, n, 1), dev),
                  (_tan(dP, (1, n, n), dev), _tan(dq, (1, n, 1), dev), _tan(dl_min, (1, n, 1), dev), _tan(dl_max, (1, n, 1), dev)),
                  epsilon=epsilon)
    return dl.reshape(n).cpu().numpy()


def jvpSignedBoxQP(P, q, l_min, l_max, v, l, dP=None, dq=None, dl_min=None, dl_max=None, epsilon=1e-10):
    return jvpBoxQP(P, q, l_min, l_max, l, dP, dq, dl_min, dl_max, epsilon, v)


def _polish_one(kind, P, q, extras, l, max_steps, reg=0.0):
    """-> (l polished (N,), (r before, r after), accepted steps, status) of one problem (ops._polish)."""
    dev = _dev()
    n = np.asarray(q).size
    x, resid, steps, status = ops._polish(kind, _t(P, (1, n, n), dev), _t(q, (1, n, 1), dev), extras(dev, n), _t(l, (1, n, 1), dev),
                                          max_steps, return_info=True, reg=reg)
    r = resid.cpu().numpy()[0]
    return x.reshape(n).cpu().numpy(), (float(r[0]), float(r[1])), int(steps.item()), int(status.item())


def polishQP(P, q, l, max_steps=8, reg=0.0):
    """An extension (the reference has no polish): up to max_steps Newton steps on the KKT system from l, each kept only if
    it lowers the natural residual max |l - proj(l - (P l + q))|.  -> (l, (residual before, after), steps, status 0 / 1 / 2).
    reg (here and below): the proximal weight of the step's matrix (ops._polish), for a P that is only positive semidefinite."""
    return _polish_one(0, P, q, lambda dev, n: (), l, max_steps, reg)


def polishQCQP(P, q, l_n, mu, l, max_steps=8, reg=0.0):
    return _polish_one(1, P, q, lambda dev, n: (_t(l_n, (1, n // 2, 1), dev), _t(mu, (1, n // 2, 1), dev)), l, max_steps, reg)


def polishBoxQP(P, q, l_min, l_max, l, max_steps=8, v=None, reg=0.0):
    """With `v` the signed box QP's."""
    if v is None:
        return _polish_one(2, P, q, lambda dev, n: (_t(l_min, (1, n, 1), dev), _t(l_max, (1, n, 1), dev)), l, max_steps, reg)
    return _polish_one(3, P, q, lambda dev, n: (_t(l_min, (1, n, 1), dev), _t(l_max, (1, n, 1), dev), _t(v, (1, n, 1), dev)), l,
                       max_steps, reg)
