"""How each solve of a batch ended: per-problem status and optimality residuals, computed on the device.

The solvers behind `QPFn2` / `QCQPFn2` / `BoxQPFn2` / `SignedBoxQPFn2` do not signal failure: a problem that ran into
`max_iter` or ended in NaN looks like any other in the output.  The functions here classify a batch with one streaming HIP
kernel (include/diffqcqp_hip.h: dqq_check_f64) that does not depend on which route solved a problem:

    x, info = solve_qp_checked(P, q, eps, max_iter)       # forward + check, same stream
    info = check_qp(P, q, x)                              # any x, e.g. the output of QPFn2.apply
    info.status        (B) int32: 0 converged, 1 stopped at max_iter, 2 not finite
    info.natural       (B) max |x - PI(x - (Px + q))|: zero exactly at a solution; read it against info.scale
    info.infeasibility (B) max |x - PI(x)|
    info.objective     (B) 1/2 x'Px + q'x
    info.scale         (B) max(max |P||x|, max |q|)
    info.counts        (3) int64: problems per status

Tensors are the autograd Functions' ((B,N,N), (B,N,1), (B,N/2,1)), used detached; GPU tensors are used in place and the
results stay on the device, CPU tensors are staged through the current GPU as qcqp.py stages them and the results come back on
the CPU.  Nothing here synchronises.  The four Functions of qcqp.py are untouched.
"""
from collections import namedtuple

import torch

from . import ops, qcqp

CheckInfo = namedtuple("CheckInfo", "status natural infeasibility objective scale counts")


def _stage(tensors):
    """-> (device tensors, home device): qcqp.py's staging."""
    home = tensors[1].device   # q
    if home.type == "cuda":
        return [t.detach() for t in tensors], home
    dev = qcqp._device_for(tensors[1])
    return [t.detach().to(dev) for t in tensors], home


def _layout(layout):
    if layout is None:
        return qcqp._default_layout
    return qcqp._LAYOUTS[layout] if isinstance(layout, str) else layout


def _info(kind, P, q, extras, x, iters, max_iter, layout, home):
    status, resid, counts = ops.solution_check(kind, P, q, extras, x, iters=iters, max_iter=max_iter, layout=layout)
    if home != status.device:
        status, resid, counts = status.to(home), resid.to(home), counts.to(home)
    return CheckInfo(status, resid[:, 0], resid[:, 1], resid[:, 2], resid[:, 3], counts)


def _check(kind, tensors, iters, max_iter, layout):
    (P, q, *extras, x), home = _stage(tensors)
    if iters is not None and iters.device != q.device:
        iters = iters.to(q.device)
    return _info(kind, P, q, extras, x, iters, max_iter, _layout(layout), home)


def check_qp(P, q, x, iters=None, max_iter=None, layout=None):
    """layout: None (qcqp.get_default_layout()), "auto" / "dense", or a DQQ_P_* value (DQQ_P_DIAG: P is (B,N))."""
    return _check(0, (P, q, x), iters, max_iter, layout)


def check_qcqp(P, q, l_n, mu, x, iters=None, max_iter=None, layout=None):
    return _check(1, (P, q, l_n, mu, x), iters, max_iter, layout)


def check_boxqp(P, q, l_min, l_max, x, iters=None, max_iter=None, layout=None):
    return _check(2, (P, q, l_min, l_max, x), iters, max_iter, layout)


def check_signedboxqp(P, q, l_min, l_max, v, x, iters=None, max_iter=None, layout=None):
    return _check(3, (P, q, l_min, l_max, v, x), iters, max_iter, layout)


def _solve(kind, tensors, eps, max_iter, mu_prox, layout, x0=None, scaling=None):
    """scaling: None, or "pow2" -- the forward solves the equilibrated problem (ops._forward_scaled) and eps bounds ITS residuals;
    the check runs on the caller's tensors with the unscaled x, so status and natural describe the caller's problem."""
    (P, q, *extras), home = _stage(tensors)
    layout = _layout(layout)
    if x0 is not None:   # the warm-started forward (ops.*_forward_warm), then the same check
        x0 = x0.detach().to(q.device)
    x, iters = ops._forward(kind, P, q, extras, eps, max_iter, mu_prox, layout=layout, return_iters=True, x0=x0, scaling=scaling)
    info = _info(kind, P, q, extras, x, iters, max_iter, layout, home)
    return (x if home == x.device else x.to(home)), info


def solve_qp_checked(P, q, eps, max_iter, mu_prox=1e-7, layout=None, x0=None, scaling=None):
    """The forward of QPFn2 (no autograd) with its iteration counts, then the check, on the current stream. -> (x, CheckInfo)
    x0 (B,N,1), here and in the three functions below: start the solve from it (QPWarmFn2's forward) instead of from zero."""
    return _solve(0, (P, q), eps, max_iter, mu_prox, layout, x0, scaling)


def solve_qcqp_checked(P, q, l_n, mu, eps, max_iter, mu_prox=1e-7, layout=None, x0=None, scaling=None):
    return _solve(1, (P, q, l_n, mu), eps, max_iter, mu_prox, layout, x0, scaling)


def solve_boxqp_checked(P, q, l_min, l_max, eps, max_iter, mu_prox=1e-7, layout=None, x0=None, scaling=None):
    return _solve(2, (P, q, l_min, l_max), eps, max_iter, mu_prox, layout, x0, scaling)


def solve_signedboxqp_checked(P, q, l_min, l_max, v, eps, max_iter, mu_prox=1e-7, layout=None, x0=None, scaling=None):
    return _solve(3, (P, q, l_min, l_max, v), eps, max_iter, mu_prox, layout, x0, scaling)


# halvings: the rejected trial points before the accepted steps of a damped polish (max_halvings > 0); zeros otherwise
PolishInfo = namedtuple("PolishInfo", "status before after steps halvings")


def _solve_polished(kind, tensors, eps, max_iter, max_steps, mu_prox, layout, x0=None, infinite_bounds=False, reg=0.0,
                    max_halvings=0, scaling=None):
    """Forward, polish (ops._polish, in place on the forward's own buffer) and check, three launches on the current stream.
    The check's status compares the FORWARD's iteration counts with max_iter: a solve that stopped there keeps status 1 even
    when the polish has repaired it -- `natural` and the PolishInfo say what the point is worth.  infinite_bounds (box kinds): the
    polish takes one-sided boxes (ops._polish); the check knows no such flag and reports what its own arithmetic gives.  reg: the
    polish's proximal weight (ops._polish), for a P that is only positive semidefinite.  max_halvings: the damped polish
    (ops._polish), for a forward stopped far from the solution.  scaling: as _solve's -- the forward alone sees the scaled
    problem; the polish and the check run on the caller's tensors from the unscaled x."""
    (P, q, *extras), home = _stage(tensors)
    layout = _layout(layout)
    if x0 is not None:
        x0 = x0.detach().to(q.device)
    x, iters = ops._forward(kind, P, q, extras, eps, max_iter, mu_prox, layout=layout, return_iters=True, x0=x0, scaling=scaling)
    halvings = torch.empty(q.shape[0], dtype=torch.int32, device=q.device)
    _, resid, steps, status = ops._polish(kind, P, q, extras, x, max_steps, layout, out=x, return_info=True,
                                          infinite_bounds=infinite_bounds, reg=reg, max_halvings=max_halvings, halvings=halvings)
    info = _info(kind, P, q, extras, x, iters, max_iter, layout, home)
    if home != x.device:
        x, resid, steps, status, halvings = x.to(home), resid.to(home), steps.to(home), status.to(home), halvings.to(home)
    return x, info, PolishInfo(status, resid[:, 0], resid[:, 1], steps, halvings)


def solve_qp_polished(P, q, eps, max_iter, max_steps=8, mu_prox=1e-7, layout=None, x0=None, reg=0.0, max_halvings=0,
                      scaling=None):
    """solve_qp_checked with a polish between the forward and the check: a loose eps and a few Newton steps instead of a tight
    eps.  -> (x, CheckInfo, PolishInfo: the polish's status, the natural residual before and after, accepted steps, halvings).
    max_halvings > 0: the damped polish (ops._polish), which also repairs a forward stopped outside the Newton basin."""
    return _solve_polished(0, (P, q), eps, max_iter, max_steps, mu_prox, layout, x0, reg=reg, max_halvings=max_halvings,
                           scaling=scaling)


def solve_qcqp_polished(P, q, l_n, mu, eps, max_iter, max_steps=8, mu_prox=1e-7, layout=None, x0=None, reg=0.0, max_halvings=0,
                        scaling=None):
    return _solve_polished(1, (P, q, l_n, mu), eps, max_iter, max_steps, mu_prox, layout, x0, reg=reg, max_halvings=max_halvings,
                           scaling=scaling)


def solve_boxqp_polished(P, q, l_min, l_max, eps, max_iter, max_steps=8, mu_prox=1e-7, layout=None, x0=None,
                         infinite_bounds=False, reg=0.0, max_halvings=0, scaling=None):
    return _solve_polished(2, (P, q, l_min, l_max), eps, max_iter, max_steps, mu_prox, layout, x0, infinite_bounds, reg, max_halvings,
                           scaling)


def solve_signedboxqp_polished(P, q, l_min, l_max, v, eps, max_iter, max_steps=8, mu_prox=1e-7, layout=None, x0=None,
                               infinite_bounds=False, reg=0.0, max_halvings=0, scaling=None):
    return _solve_polished(3, (P, q, l_min, l_max, v), eps, max_iter, max_steps, mu_prox, layout, x0, infinite_bounds, reg,
                           max_halvings, scaling)


# the polish path's summary (status, the first stage's r before, the last stage's r after, accepted steps and halvings over all
# stages) and its per-stage records: stage_resid (B,S,2), stage_steps (B,S)
PathInfo = namedtuple("PathInfo", "status before after steps halvings stage_resid stage_steps")


def _solve_newton(kind, tensors, kappas, stage_steps, max_halvings, reg, layout, scaling):
    """The cold start x = PI(0) (ops.cold_start: torch ops), the polish path from it (ops._polish_path, in place on the start's
    buffer) and the check, two launches on the current stream.  No ADMM: the check is given no iteration counts, so its status
    is 0 (converged) unless an entry is not finite (2); CheckInfo.natural against CheckInfo.scale, and PathInfo.after, say what
    the point is worth."""
    (P, q, *extras), home = _stage(tensors)
    layout = _layout(layout)
    x = ops.cold_start(kind, q, extras)
    _, resid, steps, status, halvings, sres, ssteps = ops._polish_path(kind, P, q, extras, x, kappas, stage_steps, max_halvings, reg,
                                                                      layout, out=x, return_info=True, scaling=scaling)
    info = _info(kind, P, q, extras, x, None, None, layout, home)
    path = PathInfo(status, resid[:, 0], resid[:, 1], steps, halvings, sres, ssteps)
    if home != x.device:
        x, path = x.to(home), PathInfo(*(t.to(home) for t in path))
    return x, info, path


def solve_qp_newton(P, q, kappas=ops.PATH_KAPPAS, stage_steps=ops.PATH_STEPS, max_halvings=8, reg=0.0, layout=None, scaling=None):
    """Solve a batch of QPs from the cold start by the polish path alone (continuation in kappa, then the hard damped polish; one
    launch) and check it.  -> (x (B,N,1), CheckInfo, PathInfo).  The schedule and the other arguments: ops._polish_path."""
    return _solve_newton(0, (P, q), kappas, stage_steps, max_halvings, reg, layout, scaling)


def solve_qcqp_newton(P, q, l_n, mu, kappas=ops.PATH_KAPPAS, stage_steps=ops.PATH_STEPS, max_halvings=8, reg=0.0, layout=None,
                      scaling=None):
    return _solve_newton(1, (P, q, l_n, mu), kappas, stage_steps, max_halvings, reg, layout, scaling)


def solve_boxqp_newton(P, q, l_min, l_max, kappas=ops.PATH_KAPPAS, stage_steps=ops.PATH_STEPS, max_halvings=8, reg=0.0, layout=None,
                       scaling=None):
    return _solve_newton(2, (P, q, l_min, l_max), kappas, stage_steps, max_halvings, reg, layout, scaling)


def solve_signedboxqp_newton(P, q, l_min, l_max, v, kappas=ops.PATH_KAPPAS, stage_steps=ops.PATH_STEPS, max_halvings=8, reg=0.0,
                             layout=None, scaling=None):
    return _solve_newton(3, (P, q, l_min, l_max, v), kappas, stage_steps, max_halvings, reg, layout, scaling)


Sensitivities = namedtuple("Sensitivities", "x jacobians polish_status jacobian_status")


ActiveInfo = namedtuple("ActiveInfo", "state mult margin where status margin_of_scale")
SensitivitiesActive = namedtuple("SensitivitiesActive", Sensitivities._fields + ("active",))   # with_active=True
# kappa > 0: x is the smoothed polish's point x_kappa, the Jacobians are the smoothed ones there; smooth_status (B) and smooth_resid
# (B,2: r_kappa before and after) are dqq_polish_smooth_f64's -- look at them before trusting a gradient
SensitivitiesSmooth = namedtuple("SensitivitiesSmooth", Sensitivities._fields + ("smooth_status", "smooth_resid"))


def _active_info(kind, P, q, extras, x, layout, home, infinite_bounds):
    act = ops._newton_active(kind, P, q, extras, x, layout, infinite_bounds=infinite_bounds)
    _, resid, _ = ops.solution_check(kind, P, q, extras, x, layout=layout)
    info = ActiveInfo(*act, act.margin / resid[:, 3])
    return info if home == x.device else ActiveInfo(*(t.to(home) for t in info))


def _active(kind, tensors, layout, infinite_bounds=False):
    (P, q, *extras, x), home = _stage(tensors)
    return _active_info(kind, P, q, extras, x, _layout(layout), home, infinite_bounds)


def active_qp(P, q, x, layout=None):
    """Which active set the Newton derivatives at x are taken on, and how far from a kink: -> ActiveInfo(state (B,N) int32: 0 free,
    3 on the bound 0;  mult (B,N): the multiplier, +0.0 where free;  margin (B): how far z = x - (P x + q) may move, in the max
    norm, before state changes;  where (B): the coordinate that is nearest;  status (B): 0 / 2 not finite;  margin_of_scale (B):
    margin over the solution check's scale (CheckInfo.scale) -- a Jacobian taken at 1e-12 of the scale from a kink is one of the
    two one-sided derivatives).  ops._newton_active and the solution check, two launches on the current stream.  layout: as
    check_qp's."""
    return _active(0, (P, q, x), layout)


def active_qcqp(P, q, l_n, mu, x, layout=None):
    """Per contact: state (B,N/2) 0 inside the disc, 1 sliding, 3 outside a disc of radius <= 0; where (B) is a contact."""
    return _active(1, (P, q, l_n, mu, x), layout)


def active_boxqp(P, q, l_min, l_max, x, layout=None, infinite_bounds=False):
    """state (B,N): 0 free, 1 on l_min, 2 on l_max.  infinite_bounds: one-sided boxes; an infinite side takes no part."""
    return _active(2, (P, q, l_min, l_max, x), layout, infinite_bounds)


def active_signedboxqp(P, q, l_min, l_max, v, x, layout=None, infinite_bounds=False):
    """state (B,N) on the effective bounds: 0 free, 1 on l_min, 2 on l_max, 3 on the sign constraint's 0."""
    return _active(3, (P, q, l_min, l_max, v, x), layout, infinite_bounds)


def _solve_sensitivities(kind, tensors, eps, max_iter, max_steps, mu_prox, layout, need, x0=None, infinite_bounds=False,
                         with_active=False, reg=0.0, scaling=None, kappa=0.0, smooth_steps=20, max_halvings=8):
    """Forward, polish (in place on the forward's own buffer) and the Newton Jacobians at the polished point
    (ops._newton_jacobian: dqq_newton_jac_f64), three launches on the current stream.  GPU tensors only when the call is captured
    into a HIP graph (CPU tensors are staged, which a capture cannot hold); N > 64 on a (B,N,N) P allocates scratch per call.
    with_active: two more launches, and the ActiveInfo of the polished point behind the Sensitivities.  reg: the proximal weight
    of the polish and of the Jacobians (ops._polish, ops._newton_jacobian), for a P that is only positive semidefinite.  scaling:
    as _solve's -- the forward alone sees the scaled problem; the polish and the Jacobians are the caller's problem's.
    kappa > 0: one more launch, the smoothed polish (ops._polish with kappa, smooth_steps, max_halvings) from the polished x, as the
    autograd backward does under set_default_smoothing; the Jacobians are the smoothed ones (dqq_newton_jac_smooth_f64) at x_kappa
    with the same kappa -> SensitivitiesSmooth.  A smoothed active set is out of scope: with_active then raises."""
    kappa = ops._kappa(kappa)
    if kappa and with_active:
        raise ValueError("with_active is not supported with kappa > 0: the active set of a smoothed solution is out of scope")
    if kappa and infinite_bounds:
        raise ValueError("infinite_bounds is not supported with kappa > 0 (include/diffqcqp_hip.h: one-sided boxes under smoothing)")
    (P, q, *extras), home = _stage(tensors)
    layout = _layout(layout)
    if x0 is not None:
        x0 = x0.detach().to(q.device)
    x = ops._forward(kind, P, q, extras, eps, max_iter, mu_prox, layout=layout, x0=x0, scaling=scaling)
    _, _, _, pstatus = ops._polish(kind, P, q, extras, x, max_steps, layout, out=x, return_info=True,
                                   infinite_bounds=infinite_bounds, reg=reg)
    sstatus = sresid = None
    if kappa:
        x, sresid, _, sstatus = ops._polish(kind, P, q, extras, x, smooth_steps, layout, return_info=True, reg=reg,
                                            max_halvings=max_halvings, kappa=kappa)
    *J, jstatus = ops._newton_jacobian(kind, P, q, extras, x, need, layout, return_status=True, infinite_bounds=infinite_bounds,
                                       reg=reg, kappa=kappa)
    active = _active_info(kind, P, q, extras, x, layout, home, infinite_bounds) if with_active else None
    if home != x.device:
        x, pstatus, jstatus = x.to(home), pstatus.to(home), jstatus.to(home)
        J = [None if j is None else j.to(home) for j in J]
        if kappa:
            sstatus, sresid = sstatus.to(home), sresid.to(home)
    if kappa:
        return SensitivitiesSmooth(x, tuple(J), pstatus, jstatus, sstatus, sresid)
    if with_active:
        return SensitivitiesActive(x, tuple(J), pstatus, jstatus, active)
    return Sensitivities(x, tuple(J), pstatus, jstatus)


def solve_qp_sensitivities(P, q, eps, max_iter, max_steps=8, mu_prox=1e-7, layout=None, x0=None, with_active=False, reg=0.0,
                           scaling=None, kappa=0.0, smooth_steps=20, max_halvings=8):
    """Solve, polish and differentiate: -> Sensitivities(x (B,N,1), jacobians (Jq,), polish_status (B): dqq_polish_f64's,
    jacobian_status (B): dqq_newton_jac_f64's).  Jq[b,i,j] = dx_i/dq_j; dx_i/dP_jk = Jq[b,i,j] x_k (ops.newton_jacobian_jvp /
    _vjp apply the Jacobians to stacked vectors).  with_active (here and in the three functions below): -> SensitivitiesActive, the
    same four fields and `active`, the ActiveInfo of the polished point (active_qp): its margin says whether the Jacobians were
    taken on a kink.  kappa > 0 (here and below): -> SensitivitiesSmooth, the smoothed Jacobians at the smoothed polish's point
    (smooth_steps, max_halvings: its budget), with that polish's status and residual; with_active then raises ValueError."""
    return _solve_sensitivities(0, (P, q), eps, max_iter, max_steps, mu_prox, layout, (True,), x0, with_active=with_active,
                                reg=reg, scaling=scaling, kappa=kappa, smooth_steps=smooth_steps, max_halvings=max_halvings)


def solve_qcqp_sensitivities(P, q, l_n, mu, eps, max_iter, max_steps=8, mu_prox=1e-7, layout=None, x0=None,
                             need=(True, True, True), with_active=False, reg=0.0, scaling=None, kappa=0.0, smooth_steps=20,
                             max_halvings=8):
    """-> Sensitivities with jacobians (Jq, Jl_n, Jmu), None where not needed."""
    return _solve_sensitivities(1, (P, q, l_n, mu), eps, max_iter, max_steps, mu_prox, layout, need, x0, with_active=with_active,
                                reg=reg, scaling=scaling, kappa=kappa, smooth_steps=smooth_steps, max_halvings=max_halvings)


def solve_boxqp_sensitivities(P, q, l_min, l_max, eps, max_iter, max_steps=8, mu_prox=1e-7, layout=None, x0=None,
                              need=(True, True, True), infinite_bounds=False, with_active=False, reg=0.0, scaling=None, kappa=0.0,
                              smooth_steps=20, max_halvings=8):
    """-> Sensitivities with jacobians (Jq, Jl_min, Jl_max), None where not needed.  infinite_bounds: one-sided boxes are polished
    and differentiated (the column of an infinite bound is zero) instead of ending with status 2."""
    return _solve_sensitivities(2, (P, q, l_min, l_max), eps, max_iter, max_steps, mu_prox, layout, need, x0, infinite_bounds,
                                with_active, reg, scaling, kappa, smooth_steps, max_halvings)


def solve_signedboxqp_sensitivities(P, q, l_min, l_max, v, eps, max_iter, max_steps=8, mu_prox=1e-7, layout=None, x0=None,
                                    need=(True, True, True), infinite_bounds=False, with_active=False, reg=0.0, scaling=None,
                                    kappa=0.0, smooth_steps=20, max_halvings=8):
    """-> Sensitivities with jacobians (Jq, Jl_min, Jl_max); v takes nothing.  infinite_bounds: as solve_boxqp_sensitivities'."""
    return _solve_sensitivities(3, (P, q, l_min, l_max, v), eps, max_iter, max_steps, mu_prox, layout, need, x0, infinite_bounds,
                                with_active, reg, scaling, kappa, smooth_steps, max_halvings)
