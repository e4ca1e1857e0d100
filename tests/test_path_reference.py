"""CPU checks of the numpy restatement of the polish path (tests/path_reference.py; csrc/path_core.h is the same definition) on
the batches frozen under tests/golden/smooth (N = 8, 32 problems, cold starts): it is the explicit chain of smoothed polishes bit
for bit on every output; with the default schedule every problem of every frozen row converges, where the hard damped polish
alone leaves problems unsolved; and the chain with 60 steps per stage reproduces the frozen hard solutions -- it is how they were
made."""
import numpy as np
import pytest

import path_cases as PC
import path_reference as PR
import polish_ls_reference as L
import smooth_cases as SC
import smooth_reference as S

SCHEDULES = {"default": (PR.KAPPAS, PR.STEPS), "hard alone": ((0.0,), (60,)), "one smoothed stage": ((1e-2,), (12,)),
             "not monotone": ((1e-3, 1e-1, 0.0, 1e-2), (3, 2, 4, 3)), "a stage without budget": ((1e-1, 1e-2, 0.0), (4, 0, 6))}


@pytest.mark.parametrize("kind,structure", SC.ROWS)
@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_restatement_is_the_explicit_chain_bit_for_bit(kind, structure, name):
    P, q, ex, x, _, _ = SC.frozen(kind, structure)
    kappas, steps = SCHEDULES[name]
    got = PR.polish_path_batch(kind, P, q, ex, x, kappas, steps, 8, 0.0)
    # the chain, call by call, each from the last call's x_out
    cur, calls = x, []
    for kappa, n in zip(kappas, steps):
        calls.append(S.polish_batch(kind, P, q, ex, cur, n, 8, 0.0, kappa))
        cur = calls[-1][0]
    assert SC.same_bits(got[0], calls[-1][0])
    for s, c in enumerate(calls):
        assert SC.same_bits(got[5][:, s], c[1]) and SC.same_bits(got[6][:, s], c[2])
    assert SC.same_bits(got[1][:, 0], calls[0][1][:, 0]) and SC.same_bits(got[1][:, 1], calls[-1][1][:, 1])
    assert SC.same_bits(got[2], sum(c[2] for c in calls)) and SC.same_bits(got[4], sum(c[4] for c in calls))
    assert SC.same_bits(got[3], np.where(calls[0][3] == 2, 2, np.where(got[2] > 0, 0, 1)))
    assert got[2].dtype == got[3].dtype == got[4].dtype == got[6].dtype == np.int32
    PC.equal(got, PC.chain(lambda xs, kappa, n: S.polish_batch(kind, P, q, ex, xs, n, 8, 0.0, kappa), x, kappas, steps))
    if name == "a stage without budget":         # the stage evaluates its r and moves nothing
        assert not got[6][:, 1].any() and SC.same_bits(got[5][:, 1, 0], got[5][:, 1, 1])
    if len(kappas) == 1:                         # one stage: the parent itself
        parent = S.polish_batch(kind, P, q, ex, x, steps[0], 8, 0.0, kappas[0])
        assert all(SC.same_bits(g, r) for g, r in zip(got[:5], parent))


@pytest.mark.parametrize("kind,structure", SC.ROWS)
def test_default_schedule_converges_on_every_problem(kind, structure):
    """A condition, not a tolerance: r <= smooth_cases.CONVERGED on 32 of 32."""
    P, q, ex, x, _, _ = SC.frozen(kind, structure)
    out = PR.polish_path_batch(kind, P, q, ex, x)
    print("%s %s: %d of %d solved, most accepted steps %d" % (kind, structure, (out[1][:, 1] <= SC.CONVERGED).sum(), SC.B, out[2].max()))
    assert (out[1][:, 1] <= SC.CONVERGED).all() and (out[3] == 0).all()
    if (kind, structure) in (("qcqp", "dense"), ("box", "dense")):       # what the path is for: the hard damped polish alone does not
        hard = L.polish_ls_batch(kind, P, q, ex, x, 60, 8)
        assert (hard[1][:, 1] > SC.CONVERGED).sum() >= 1


@pytest.mark.parametrize("kind,structure", SC.ROWS)
def test_sixty_steps_per_stage_reproduce_the_frozen_hard_solution(kind, structure):
    P, q, ex, x, xh, _ = SC.frozen(kind, structure)
    out = PR.polish_path_batch(kind, P, q, ex, x, PR.KAPPAS, (SC.SOLVE_STEPS,) * 5, SC.SOLVE_HALVINGS)
    assert SC.same_bits(out[0], xh)


def test_a_bad_problem_keeps_x_and_records_what_the_chain_would():
    P, q, ex, x = (np.array(a) if not isinstance(a, tuple) else tuple(np.array(e) for e in a) for a in SC.problem("box", 5, 4, "dense"))
    x[1, 2] = np.nan
    q[2, 0] = np.inf
    out = PR.polish_path_batch("box", P, q, ex, x, (1e-2, 0.0), (3, 3))
    assert list(out[3]) == [0, 2, 2, 0] and SC.same_bits(out[0][1:3], x[1:3]) and not out[2][1:3].any() and not out[6][1:3].any()
