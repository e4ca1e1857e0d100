"""CPU check of tests/param_cases.py, the route table of tests/test_gpu_parameters.py: every row's route plan is the one the
row names, and the rows of each kind together launch every kernel family that route.cpp can pick for that kind -- so the
GPU tests cannot land on another kernel than the one they claim to test, nor leave a family out."""
import numpy as np
import pytest

from param_cases import BWD, FWD, FWD_FAMILIES, BWD_FAMILIES, KIND, families, nudge, row_id
from test_routes import AUTO, DENSE, DIAG, REF, XD, XL, _build, raw_plan, render


@pytest.fixture(scope="module")
def shipped():
    return _build(False)


@pytest.mark.parametrize("row", FWD + BWD, ids=row_id)
def test_row_takes_its_route(shipped, row):
    pas, kind, N, B, layout, _, want = row
    assert render(raw_plan(shipped, pas, KIND[kind], N, B, layout)) == want


def _reachable(lib, pas, kind):
    """Families of every plan of (pas, kind) over sizes, batch sizes on both sides of the thresholds, layouts and flags."""
    out = set()
    for N in list(range(1, 73)) + [96, 128]:
        for B in (1, 100, 300, 2051, 16383, 16384, 24575, 24576, 32768, 32769, 40960, 40961, 57343, 57344, 131072, 131073):
            for layout in (AUTO, DENSE, DIAG):
                for flags in (0, REF, XD, XL, XD | XL, XD | REF):
                    out |= families(render(raw_plan(lib, pas, KIND[kind], N, B, layout | flags)))
    return out


@pytest.mark.parametrize("pas,kind", [(0, "qp"), (0, "qcqp"), (0, "box"), (0, "sbox"), (1, "qp"), (1, "qcqp"), (1, "box")])
def test_rows_cover_every_reachable_family(shipped, pas, kind):
    reach = _reachable(shipped, pas, kind)
    assert reach <= set(FWD_FAMILIES if pas == 0 else BWD_FAMILIES), reach
    covered = set().union(*(families(r[6]) for r in (FWD if pas == 0 else BWD) if r[1] == kind))
    assert reach - covered == set(), "families of %s %s without a row" % (("fwd", "bwd")[pas], kind)
    assert covered <= reach


def test_every_family_is_covered_by_some_kind(shipped):
    fwd = set().union(*(families(r[6]) for r in FWD))
    bwd = set().union(*(families(r[6]) for r in BWD))
    assert fwd == set(FWD_FAMILIES) and bwd == set(BWD_FAMILIES)


def test_nudge_moves_constraints_inside_and_nothing_else(oracle):
    from conftest import make_problem
    for kind in ("qp", "qcqp", "box"):
        d = {k: v.numpy() for k, v in make_problem(kind, 200, 8, 5151, "mixed").items()}
        if kind == "qp":
            x = oracle.qp_fwd_batch(d["P"], d["q"], 1e-7, 1000)[0]
        elif kind == "qcqp":
            x = oracle.qcqp_fwd_batch(d["P"], d["q"], d["l_n"], d["mu"], 1e-7, 1000)[0]
        else:
            x = oracle.boxqp_fwd_batch(d["P"], d["q"], d["l_min"], d["l_max"], 1e-7, 1000)[0]
        y = nudge(kind, d, x, 1)
        assert np.array_equal(y, nudge(kind, d, x, 1)) and not np.array_equal(y, x)
        moved = (y != x)[:, :, 0]
        if kind == "qp":
            assert (x[:, :, 0][moved] == 0).all() and (y[:, :, 0][moved] > 0).all()
            share = moved.sum() / (x == 0).sum()
        elif kind == "qcqp":
            r = (d["l_n"] * d["mu"])[:, :, 0]
            nx = np.hypot(x[:, 0::2, 0], x[:, 1::2, 0])
            ny = np.hypot(y[:, 0::2, 0], y[:, 1::2, 0])
            c = moved[:, 0::2] | moved[:, 1::2]
            assert (np.abs(nx - r)[c] < 1e-6 * np.maximum(1.0, r)[c]).all() and (ny[c] < r[c]).all()
            share = c.sum() / ((np.abs(nx - r) < 1e-6 * np.maximum(1.0, r)) & (nx > 0)).sum()
        else:
            lo, hi = d["l_min"][:, :, 0], d["l_max"][:, :, 0]
            on = (x[:, :, 0] <= lo) | (x[:, :, 0] >= hi)
            assert on[moved].all() and ((y[:, :, 0] > lo) & (y[:, :, 0] < hi))[moved].all()
            share = moved.sum() / on.sum()
        assert 0.35 < share < 0.65, (kind, share)
