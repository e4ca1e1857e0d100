"""Inputs of the warm-start tests (tests/test_warm_reference.py on the CPU, tests/test_gpu_warm.py on the device).  Not a test
file.  The rows are tests/param_cases.py's forward rows -- the smallest batch that reaches each forward family and lane layout,
every B with a ragged last tile --, the problems row_problem's, the yardstick tests/warm_reference.py.  Everything the numpy
restatement computes for a row is computed once on the row's base batch and shared (problem b of the batch is problem b mod
base), and never modified."""
import functools

import numpy as np

import warm_reference as W
from conftest import make_problem
from param_cases import FWD, row_id, row_problem, row_seed

EXTRAS = {"qp": (), "qcqp": ("l_n", "mu"), "box": ("l_min", "l_max"), "sbox": ("l_min", "l_max", "v")}
EPS, MAX_ITER = 1e-7, 1000
# x0 = the cold solution of the batch with q perturbed by this much.  1 % for every kind: tests/test_warm_reference.py holds
# each kind to its bars at this value.
PERTURB = {"qp": 0.01, "qcqp": 0.01, "box": 0.01, "sbox": 0.01}
VARIANTS = ("perturbed", "own", "zero", "infeasible")


def well_conditioned(P):
    """The issue asks for well-conditioned inputs; make_problem's dense family (S S^T / N + 0.1 I) has a largest eigenvalue
    near N / 4 against a smallest of 0.1.  The rows keep param_cases' shapes, structures and seeds, and every P keeps its
    eigenvectors; its spectrum is mapped affinely onto [0.5, 2] (condition number <= 4).  A diagonal P stays exactly
    diagonal (its entries are mapped, nothing is rotated)."""
    import torch
    P = P.clone()
    off = P - torch.diag_embed(torch.diagonal(P, dim1=1, dim2=2))
    isdiag = (off == 0).all(dim=2).all(dim=1)
    lam, V = torch.linalg.eigh(P)
    lo, hi = lam[:, :1], lam[:, -1:]
    span = torch.where(hi > lo, hi - lo, torch.ones_like(hi))
    dense = V @ torch.diag_embed(0.5 + 1.5 * (lam - lo) / span) @ V.transpose(1, 2)
    dense = 0.5 * (dense + dense.transpose(1, 2))
    d = torch.diagonal(P, dim1=1, dim2=2)
    diag = torch.diag_embed(0.5 + 1.5 * (d - lo) / span)
    return torch.where(isdiag.view(-1, 1, 1), diag, dense).contiguous()


def problem(row):
    """row_problem's batch with every P re-conditioned (well_conditioned).  -> (base, full)"""
    base, _ = row_problem(row, make_problem)
    base = dict(base)
    base["P"] = well_conditioned(base["P"])
    B = row[3]
    reps = -(-B // base["q"].shape[0])
    full = {k: v.repeat((reps,) + (1,) * (v.dim() - 1))[:B].contiguous() for k, v in base.items()}
    return base, full


def extras_of(kind, d):
    return tuple(d[n].numpy() for n in EXTRAS[kind])


@functools.lru_cache(maxsize=4)
def reference(row):
    """-> (base, full, cold (x, it), {variant: (x0, x, it)}) on the row's base batch, by warm_reference.  The infeasible start
    is outside every kind's feasible set on about half of the coordinates: the own solution mirrored and pushed out by 2."""
    _, kind, N, B, layout, _, _ = row
    base, full = problem(row)
    P, q, ex = base["P"].numpy(), base["q"].numpy(), extras_of(kind, base)
    cold = W.solve(kind, P, q, EPS, MAX_ITER, ex)
    rng = np.random.default_rng(row_seed(row))
    starts = {"perturbed": W.perturbed_start(kind, P, q, ex, PERTURB[kind], row_seed(row)),
              "own": cold[0].copy(),
              "zero": np.zeros_like(cold[0]),
              "infeasible": -cold[0] + 2.0 * np.sign(rng.standard_normal(cold[0].shape))}
    out = {}
    for name in VARIANTS:
        x, it = W.solve(kind, P, q, EPS, MAX_ITER, ex, x0=starts[name])
        out[name] = (starts[name], x, it)
    return base, full, cold, out


def n8_rows():
    """The N = 8 rows on a diagonal and on a dense P, one of each per kind: the batches of the iteration-count conditions."""
    rows = []
    for kind in EXTRAS:
        rows.append(next(r for r in FWD if r[1] == kind and r[2] == 8 and r[5] == "diag"))
        rows.append(next(r for r in FWD if r[1] == kind and r[2] == 8 and r[5] == "dense"))
    return rows


__all__ = ["FWD", "row_id", "reference", "n8_rows", "extras_of", "VARIANTS", "PERTURB", "EPS", "MAX_ITER"]
