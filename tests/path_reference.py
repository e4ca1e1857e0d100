"""The polish path (dqq_polish_path_f64) restated in numpy: the definition of diffqcqp_amd/csrc/path_core.h a second time.  With
stages (kappa_s, steps_s), s = 0 .. S-1, the path is bit for bit the chain of S calls of the smoothed damped polish
(tests/smooth_reference.py: polish_batch, which branches to the hard damped polish's restatement at kappa == 0): call s has
kappa = kappa_s and max_steps = steps_s, all calls share reg and max_halvings, and each starts from the previous call's x_out.
That chain is written out below -- it is the definition --, with the summary the entry reports besides: resid = (stage 0's r
before, the last stage's r after), steps and halvings summed, status 2 if stage 0's is 2, else 0 if any step was accepted, else 1.
Not a test file."""
import numpy as np

import smooth_reference as S

KAPPAS = (1e-1, 1e-2, 1e-3, 1e-4, 0.0)      # the default schedule ...
STEPS = (4, 4, 4, 4, 60)                    # ... and its per-stage step budgets
MAX_HALVINGS = 8


def polish_path_batch(kind, P, q, ex, x, kappas=KAPPAS, stage_steps=STEPS, max_halvings=MAX_HALVINGS, reg=0.0):
    """P (B,n,n), q (B,n), ex each (B,.), x (B,n) -> x_out (B,n), resid (B,2), steps, status, halvings (B) int32,
    stage_resid (B,S,2), stage_steps (B,S) int32"""
    B, n = x.shape
    n_stages = len(kappas)
    assert n_stages == len(stage_steps) and 1 <= n_stages <= 8
    stage_resid = np.empty((B, n_stages, 2))
    stage_taken = np.empty((B, n_stages), dtype=np.int32)
    steps, halvings = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    cur, status0 = x, None
    for s in range(n_stages):
        cur, rs, st, status, hv = S.polish_batch(kind, P, q, ex, cur, stage_steps[s], max_halvings, reg, kappas[s])
        stage_resid[:, s], stage_taken[:, s] = rs, st
        steps, halvings = steps + st, halvings + hv
        if s == 0:
            status0 = status
    resid = np.stack([stage_resid[:, 0, 0], stage_resid[:, -1, 1]], axis=1)
    status = np.where(status0 == 2, 2, np.where(steps > 0, 0, 1)).astype(np.int32)
    return cur, resid, steps, status, halvings, stage_resid, stage_taken
