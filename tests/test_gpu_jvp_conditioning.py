"""dqq_jvp_f64 on the reference's ill-conditioned inputs (-m gpu): every tests/golden/rd_*.npz (rank-deficient P, duplicated
Jacobian rows, N = 8, 32, 64), the reference's own matrices ref_m2_*, ref_g2_*, ref_g4_*, ref_gblock_* (singular, cond ~1e22, a
zero-radius contact) and conditioning/qp_ill_n8.npz (a diagonal P from 4e-18 to 2.4e17; a third of its x is NaN), each with the
fixture's own x and seeded tangents.  There the refinement leaves after 3 bodies, in between, or runs all 10 steps
(tests/test_jvp_reference.py shows it on the host core), and the systems are singular: the regime the well-conditioned
batches of tests/test_gpu_jvp.py never enter.

Every family that serves the fixture's (kind, N) -- DQQ_P_AUTO and DQQ_P_DENSE through JvpTeam (QP to N = 64, QCQP to 42) or
JvpAny (QCQP N = 64), DQQ_P_DIAG where P is diagonal -- is held to its own bar, the host core bit for bit: dx equal as int64
patterns wherever the host's dx is finite, the same non-finite pattern elsewhere, ir_steps equal everywhere.

The adjoint identity against the library's backward on the same fixture (reference order), on the problems with a finite x,
within 10 x the gap the numpy restatement's two modes leave there (jvp_cases.FIXTURE_GAP_CPU).  No adjoint check where the
restatement's own gap exceeds 0.1 -- rd_lowrank_qp (0.31), ref_m2_qp (0.16), qp_ill (0.49): two Tikhonov iterates of a singular
system, regularised from different sides, need not agree, and a normalised gap of that size tells nothing."""
import numpy as np
import pytest

import jvp_cases as C
import jvp_reference as R
from test_gpu_jvp import AUTO, DENSE, DIAG, _backward, ops_jvp

pytestmark = pytest.mark.gpu


def _layouts(name):
    _, _, _, _, _, diagonal = C.fixture(name)
    return [AUTO, DENSE] + ([DIAG] if diagonal else [])


@pytest.mark.parametrize("name,layout", [(n, l) for n in C.fixture_names() for l in _layouts(n)])
def test_every_family_is_the_host_core_on_the_ill_conditioned_fixtures(name, layout):
    kind, d, x, tan, _, _ = C.fixture(name)
    if layout == DIAG:
        tan = (tan[0] * np.eye(tan[0].shape[1]),) + tan[1:]
    ref, ref_steps = C.host_jvp(kind, d, x, tan)
    dx, steps = ops_jvp(kind, d, x, tan, layout, return_steps=True)
    dx, steps = dx.cpu().numpy()[:, :, 0], steps.cpu().numpy().reshape(ref_steps.shape)
    fin = np.isfinite(ref)
    print("%s layout %d: steps %s, non-finite rows %d of %d" % (name, layout, np.unique(steps), (~fin).any(axis=1).sum(), len(ref)))
    assert np.array_equal(steps, ref_steps), "refinement step counts differ"
    assert np.array_equal(np.isnan(dx), np.isnan(ref)) and np.array_equal(np.isinf(dx), np.isinf(ref)), "non-finite pattern differs"
    assert np.array_equal(dx[~fin & np.isinf(ref)], ref[~fin & np.isinf(ref)])       # (an infinity has a sign)
    assert np.array_equal(dx.view(np.int64)[fin], ref.view(np.int64)[fin]), "max diff %g" % np.abs(dx[fin] - ref[fin]).max()


@pytest.mark.parametrize("name", [n for n in C.fixture_names() if C.FIXTURE_GAP_CPU[C.fixture_family(n)] <= C.ADJOINT_GAP_TELLS])
def test_adjoint_identity_on_the_ill_conditioned_fixtures(name):
    kind, d, x, tan, g, _ = C.fixture(name)
    rows = C.finite_rows(x)
    d, x, tan, g = {k: v[rows] for k, v in d.items()}, x[rows], tuple(t[rows] for t in tan), g[rows]
    dx = ops_jvp(kind, d, x, tan, DENSE).cpu().numpy()[:, :, 0]
    grads = _backward(kind, d, x, g, DENSE)
    gap, bar = C.adjoint_gap(g, dx, grads, tan), 10 * C.FIXTURE_GAP_CPU[C.fixture_family(name)]
    print("%s: adjoint gap %.3g (CPU record %.3g)" % (name, gap, bar / 10))
    assert gap <= bar
