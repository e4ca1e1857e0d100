"""Batches for the signed box QP's backward (tests/test_sbox_*.py, tests/test_gpu_sbox_bwd.py): conftest.make_problem's box
distributions with the per-coordinate cases mixed in that `make_problem("sbox", ...)` never produces, and the effective bounds
of include/diffqcqp_hip.h (dqq_signedboxqp_bwd_f64) written with torch -- a second statement of the table, independent of
csrc/sbox_bounds.h.  Not a test file."""
import torch

from conftest import make_problem

# per-coordinate cases; every one is present in every batch of 8 coordinates or more
PLAIN_POS, V_PZERO, V_NZERO, LMIN_POS_V_POS, LMAX_NEG_V_NEG, LMIN_ZERO_V_NEG, LMAX_ZERO_V_POS, PLAIN_NEG = range(8)
N_CASES = 8


def make_sbox_batch(B, N, seed, structure="diag", scale=1.0):
    """-> (dict like make_problem("sbox", ...), case (B,N,1) int64).  scale multiplies the box (test_gpu_fd.py widens it by 2.5
    so that about half of the coordinates end up between their bounds); P by `structure` as make_problem, or replaced by the
    caller."""
    d = make_problem("sbox", B, N, seed, structure)
    g = torch.Generator().manual_seed(seed + 7919)
    case = torch.randint(0, N_CASES, (B, N, 1), generator=g)
    where = torch.randperm(B * N, generator=g)[:N_CASES]
    case.view(-1)[where] = torch.arange(N_CASES)            # each case at least once, at random places
    u = torch.rand(B, N, 1, generator=g, dtype=torch.float64)
    lo, hi = scale * d["l_min"], scale * d["l_max"]          # lo in -[0.3, 0.9] scale, hi in [0.3, 0.9] scale
    mag = d["v"].abs() + 0.05
    v = torch.where(case == PLAIN_NEG, -mag, mag)
    v = torch.where(case == V_PZERO, torch.zeros_like(v), v)
    v = torch.where(case == V_NZERO, -torch.zeros_like(v), v)
    # l_min > 0 with v > 0: the whole box is on the wrong side of the sign constraint
    sel = case == LMIN_POS_V_POS
    lo = torch.where(sel, 0.05 + 0.3 * u, lo)
    hi = torch.where(sel, 0.05 + 0.3 * u + hi, hi)
    # l_max < 0 with v < 0
    sel = case == LMAX_NEG_V_NEG
    hi = torch.where(sel, -(0.05 + 0.3 * u), hi)
    lo = torch.where(sel, -(0.05 + 0.3 * u) + lo, lo)
    v = torch.where(sel, -mag, v)
    # the ties: a bound that IS the sign constraint's 0
    sel = case == LMIN_ZERO_V_NEG
    lo = torch.where(sel, torch.zeros_like(lo), lo)
    v = torch.where(sel, -mag, v)
    sel = case == LMAX_ZERO_V_POS
    hi = torch.where(sel, torch.zeros_like(hi), hi)
    d["l_min"], d["l_max"], d["v"] = lo.contiguous(), hi.contiguous(), v.contiguous()
    assert bool((d["l_min"] <= d["l_max"]).all())
    assert sorted(case.unique().tolist()) == list(range(N_CASES))
    assert torch.signbit(d["v"][case == V_NZERO]).all() and not torch.signbit(d["v"][case == V_PZERO]).any()
    return d, case


def effective_bounds(l_min, l_max, v):
    """The table of include/diffqcqp_hip.h (dqq_signedboxqp_bwd_f64), in torch: -> (lo', hi', keep_lo, keep_hi)."""
    zero = torch.zeros_like(l_min)
    hi_p = torch.minimum(l_max, zero)
    lo_p = torch.minimum(l_min, hi_p)
    lo_n = torch.maximum(l_min, zero)
    hi_n = torch.maximum(l_max, lo_n)
    lo = torch.where(v > 0, lo_p, torch.where(v < 0, lo_n, zero))
    hi = torch.where(v > 0, hi_p, torch.where(v < 0, hi_n, zero))
    return lo, hi, lo == l_min, hi == l_max
