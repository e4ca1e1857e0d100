"""One-sided boxes (DQQ_F_INFINITE_BOUNDS) on the CPU: csrc/polish_core.h and csrc/newton_core.h with the flag
(tests/hostcore/inf_bounds_check.cpp, a stand-alone program) against the numpy restatement tests/inf_bounds_reference.py bit for
bit, against the UNFLAGGED cores on large finite bounds bit for bit, against numpy.linalg.solve on a fully unbounded box, against
the QP kind on [0, +inf), and the status rules.  The same program under the address and undefined-behaviour sanitizers runs over
the same batches."""
import numpy as np
import pytest

import inf_bounds_cases as C
import inf_bounds_reference as IR
import jac_cases as JC
import polish_reference as R

INF = C.INF
B = 16
BATCHES = [(k, N, s) for k in C.KINDS for N in (3, 8) for s in ("diag", "dense")]


def _host(kind, N, structure, ex=None, flag=True, compact=False, sanitized=False, bad_row=None):
    P, q, ex0, x, gx, tan = C.problem(kind, B, N, structure, bad_row=bad_row)
    ex = ex0 if ex is None else ex
    if compact:
        P, tan = C.compact(P), (C.compact(tan[0]),) + tan[1:]
    return C.host_all(kind, P, q, ex, x, gx, tan, diag=compact, flag=flag, sanitized=sanitized)


@pytest.mark.parametrize("kind,N,structure", BATCHES)
def test_host_core_equals_the_restatement(kind, N, structure):
    """Case 1: polish (x_out, both residuals, steps, status), backward, JVP and Jacobians, bit for bit."""
    P, q, ex, x, gx, tan = C.problem(kind, B, N, structure)
    assert all(np.isinf(ex[0]).any() and np.isinf(ex[1]).any() and np.isfinite(e).any() for e in ex[:2])
    host = _host(kind, N, structure)
    ref = IR.run_batch(kind, P, q, ex, x, gx, tan)
    for k in C.INT_KEYS:
        assert np.array_equal(host[k], ref[k]), k
    assert not host["st_jvp"].any() and not host["st_bwd"].any() and not host["st_jac"].any()
    assert (host["st_polish"] != 2).all() and (host["st_polish"] == 0).any()      # nothing refused, and steps were accepted
    for k in C.FLOAT_KEYS:
        assert C.same_bits(host[k], ref[k]), k
    # an infinite side is never sat on: +0.0 gradients, zero columns
    for g, J, e in (("ga", "Ja", ex[0]), ("gb", "Jb", ex[1])):
        inf = np.isinf(e)
        assert (host[g][inf] == 0.0).all() and not np.signbit(host[g][inf]).any()
        assert (host[J].transpose(0, 2, 1)[inf] == 0.0).all()
    if structure == "diag":   # the block form on the compact diagonal: the full form's bits on the blocks
        ch = _host(kind, N, structure, compact=True)
        for k in C.INT_KEYS + ("x_out", "resid", "dx", "gq", "ga", "gb"):
            assert C.same_bits(ch[k], host[k]), k
        for k in ("gP", "Jq", "Ja", "Jb"):
            assert C.same_bits(ch[k], C.compact(host[k])), k


@pytest.mark.parametrize("kind,N,structure", BATCHES)
def test_large_finite_bounds_through_the_unflagged_path_give_the_same_bits(kind, N, structure):
    """Case 2: every infinite bound replaced by -+1e300, run WITHOUT the flag -- the code as it stood -- equals the flagged run
    on the infinite bounds in every output, signed zeros included.  No iterate comes near 1e300: max |x + d| < 1e6."""
    P, q, ex, x, gx, tan = C.problem(kind, B, N, structure)
    reach = IR.run_batch(kind, P, q, ex, x, gx, tan)["reach"]
    assert reach.max() < 1e6 and reach.max() > 0.0
    for compact in ((False, True) if structure == "diag" else (False,)):
        flagged = _host(kind, N, structure, compact=compact)
        plain = _host(kind, N, structure, ex=C.large_finite(ex), flag=False, compact=compact)
        for k in C.INT_KEYS + C.FLOAT_KEYS:
            assert C.same_bits(flagged[k], plain[k]), (k, compact)
        # ... and the flag changes nothing on finite bounds
        also = _host(kind, N, structure, ex=C.large_finite(ex), flag=True, compact=compact)
        for k in C.INT_KEYS + C.FLOAT_KEYS:
            assert C.same_bits(also[k], plain[k]), (k, compact)


@pytest.mark.parametrize("structure", ["diag", "dense"])
def test_fully_unbounded_box(structure):
    """Case 3: all bounds infinite: from x = 0 the polish ends at -P^-1 q and Jq = -P^-1, against numpy.linalg.solve within 16 x
    jac_cases.SOLVE_GAP_CPU's box record of the check's scale.  (The box kind only: the sign constraint of the signed box bounds
    every coordinate on one side, it has no unbounded problem.)"""
    N = 8
    P, q, _, _, gx, _ = C.problem("box", B, N, structure)
    ex = (np.full((B, N), -INF), np.full((B, N), INF))
    x0 = np.zeros((B, N))
    out = C.host_all("box", P, q, ex, x0, gx, None, flag=True)
    assert (out["st_polish"] == 0).all() and not out["st_jac"].any()
    want_x = np.stack([np.linalg.solve(P[b], -q[b]) for b in range(B)])
    want_J = np.stack([-np.linalg.inv(P[b]) for b in range(B)])
    scale = R.scale(P, q, out["x_out"])
    gap_x = float((np.abs(out["x_out"] - want_x).max(axis=1) / scale).max())
    gap_J = float((np.abs(out["Jq"] - want_J).max(axis=(1, 2)) / scale).max())
    print("fully unbounded box, %s: gap x %.2e, gap Jq %.2e (record %.2e)" % (structure, gap_x, gap_J, JC.SOLVE_GAP_CPU["box"]))
    assert gap_x <= JC.BAR * JC.SOLVE_GAP_CPU["box"] and gap_J <= JC.BAR * JC.SOLVE_GAP_CPU["box"]
    assert (out["Ja"] == 0.0).all() and (out["Jb"] == 0.0).all() and (out["ga"] == 0.0).all() and (out["gb"] == 0.0).all()


@pytest.mark.parametrize("structure", ["diag", "dense"])
def test_box_on_the_nonnegative_orthant_is_the_qp_kind(structure):
    """Case 4: l_min = 0, l_max = +inf.  The two paths share their evaluation order -- polish_bounds<0> IS (0, +inf),
    check_proj<0> and check_proj<2> select the same value for lo = +0.0 and hi = +inf, polish_free and M are one code -- so the
    bits are equal: x_out, residuals, steps, statuses, grad_P, grad_q, dx along (dP, dq), Jq."""
    N = 8
    P, q, _, x, gx, tan = C.problem("box", B, N, structure)
    ex = (np.zeros((B, N)), np.full((B, N), INF))
    for compact in ((False, True) if structure == "diag" else (False,)):
        Pa = C.compact(P) if compact else P
        dPa, zero, none = (C.compact(tan[0]) if compact else tan[0]), np.zeros((B, N)), np.zeros((B, 0))
        box = C.host_all("box", Pa, q, ex, x, gx, (dPa, tan[1], zero, zero), diag=compact, flag=True)
        qp = C.host_all("qp", Pa, q, (), x, gx, (dPa, tan[1], none, none), diag=compact, flag=False)
        assert (box["st_polish"] == 0).any() and not box["st_bwd"].any()
        for k in C.INT_KEYS + ("x_out", "resid", "gP", "gq", "dx", "Jq"):
            assert C.same_bits(box[k], qp[k]), (k, compact)


def _rows_equal_but(a, b, rows):
    keep = np.ones(a.shape[0], dtype=bool)
    keep[list(rows)] = False
    return C.same_bits(a[keep], b[keep])


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("structure", ["diag", "dense"])
def test_status_rules(kind, structure):
    """Case 5: with the flag l_min = +inf, l_max = -inf, a NaN bound, an infinite q and an infinite db tangent are status 2 -- NaN
    outputs (the polish: x_out = x), no other row touched; without it an infinite bound is status 2 as before."""
    N = 8
    P, q, ex, x, gx, tan = C.problem(kind, B, N, structure)
    clean = C.host_all(kind, P, q, ex, x, gx, tan, flag=True)
    ex2, q2, tan2 = tuple(e.copy() for e in ex), q.copy(), tuple(t.copy() for t in tan)
    ex2[0][1, 2] = INF
    ex2[1][3, 0] = -INF
    ex2[0][5, 1] = np.nan
    ex2[1][6, 7] = np.nan
    q2[8, 4] = -INF
    tan2[3][10, 3] = INF          # db, at a coordinate whose l_max may well be +inf: a tangent stays finite-only
    bad_all, bad_jvp = [1, 3, 5, 6, 8], [1, 3, 5, 6, 8, 10]
    for compact in ((False, True) if structure == "diag" else (False,)):
        Pa, dPa = (C.compact(P), C.compact(tan[0])) if compact else (P, tan[0])
        ref = clean if not compact else C.host_all(kind, Pa, q, ex, x, gx, (dPa,) + tan[1:], diag=True, flag=True)
        out = C.host_all(kind, Pa, q2, ex2, x, gx, (dPa,) + tan2[1:], diag=compact, flag=True)
        for k in ("st_polish", "st_bwd", "st_jac"):
            want = ref[k].copy()
            want[bad_all] = 2
            assert np.array_equal(out[k], want), k
        want = ref["st_jvp"].copy()
        want[bad_jvp] = 2
        assert np.array_equal(out["st_jvp"], want)
        assert C.same_bits(out["x_out"][bad_all], x[bad_all]) and not out["steps"][bad_all].any()
        for k in ("gP", "gq", "ga", "gb", "Jq", "Ja", "Jb"):
            assert np.isnan(out[k][bad_all]).all() and _rows_equal_but(out[k], ref[k], bad_all), k
        assert np.isnan(out["dx"][bad_jvp]).all() and _rows_equal_but(out["dx"], ref["dx"], bad_jvp)
        assert _rows_equal_but(out["x_out"], ref["x_out"], bad_all) and _rows_equal_but(out["resid"], ref["resid"], bad_all)
        if not compact:
            r = IR.run_batch(kind, P, q2, ex2, x, gx, (tan[0],) + tan2[1:])
            for k in C.INT_KEYS + C.FLOAT_KEYS:
                assert C.same_bits(out[k], r[k]), k
    # without the flag: every problem with an infinite bound is refused, as before
    plain = C.host_all(kind, P, q, ex, x, gx, tan, flag=False)
    has_inf = np.isinf(ex[0]).any(axis=1) | np.isinf(ex[1]).any(axis=1)
    assert has_inf.any()
    for k in ("st_polish", "st_jvp", "st_bwd", "st_jac"):
        assert (plain[k][has_inf] == 2).all(), k
    assert C.same_bits(plain["x_out"][has_inf], x[has_inf]) and np.isnan(plain["gq"][has_inf]).all()


@pytest.mark.parametrize("structure", ["diag", "dense"])
def test_an_infinite_radius_is_status_2_with_and_without_the_flag(structure):
    N = 8
    P, q, _, x, gx, _ = C.problem("box", B, N, structure)
    r = np.random.default_rng(5)
    ln, mu = r.uniform(0.5, 1.5, (B, N // 2)), r.uniform(0.3, 1.0, (B, N // 2))
    ln[2, 1] = INF
    for flag in (False, True):
        out = C.host_all("qcqp", P, q, (ln, mu), x, gx, None, flag=flag)
        for k in ("st_polish", "st_jvp", "st_bwd", "st_jac"):
            assert out[k][2] == 2 and (np.delete(out[k], 2) != 2).all(), (k, flag)
        assert np.isnan(out["gq"][2]).all() and C.same_bits(out["x_out"][2], x[2])


def test_sanitized_stand_alone_program_over_the_same_batches():
    """Case 6: the program built with -fsanitize=address,undefined (its own main, no Python in the process) runs the flagged cores
    over case 1's batches clean and gives the plain build's bits."""
    for kind, N, structure in BATCHES:
        for compact in ((False, True) if structure == "diag" else (False,)):
            san = _host(kind, N, structure, compact=compact, sanitized=True, bad_row=B // 2)
            plain = _host(kind, N, structure, compact=compact, bad_row=B // 2)
            assert plain["st_polish"][B // 2] == 2
            for k in C.INT_KEYS + C.FLOAT_KEYS:
                assert C.same_bits(san[k], plain[k]), (kind, N, structure, k)
