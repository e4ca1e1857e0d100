"""GPU tests on the reference's ill-conditioned QP workload (test_script.py:140-157: P = diag(exp(4 U(-10,10))), p from
4e-18 to 2.4e17, q ~ U(-1,1), eps = 1e-10) and on well-conditioned batches scaled by 2^+-40 -- the regimes that the
parity suite (p in [0.1, 1.1], |x - x_oracle| <= 1e-6 absolute) cannot see.

Every comparison goes through `compare`: per problem, against that problem's own max|x_oracle| (no floor at 1); a NaN
problem is a class of its own (NaN must meet NaN, and a NaN problem is NaN in every coordinate); an infinity fails.

On this workload the reference itself ends ~36 % of the problems in NaN: rho starts near 6e14 and falls, the shifted
diagonal p + rho + mu loses positivity (Solver.cpp:112), llt() yields NaN, the residual max skips it and the loop stops in
the next iteration.  The workload is chaotic: a 1-ulp change of rho's schedule (rho * (1/tau) for rho / tau) changes the
outcome of a few problems.  Hence three contracts:
  * routes in the reference's arithmetic (LDS kernel, workgroup kernel) end the same problems in NaN as the oracle and
    follow it on most of the others, not all (`reference_order`);
  * the fast routes give the same bits on every layout of the diagonal kernel, whatever a problem's neighbours;
  * the fast routes agree with the oracle on the outcome class (NaN / capped / converged) of most problems, and a problem
    that lost positivity stops at the oracle's iteration on nearly all of them; x itself is not comparable there.
On the well-conditioned batches (magnitude sweep, subnormal norm) x is checked on every problem, as in the parity suite.
"""
import os

import numpy as np
import pytest
import torch

from conftest import KNOB_DEFAULTS, knob, make_problem

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS, MAX_ITER = 1e-10, 1000000
NAN, CAPPED, CONVERGED = 2, 1, 0


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from diffqcqp_amd import build, ops as _ops, _capi
    build.build()
    _capi.lib()
    yield _ops
    for name, value in KNOB_DEFAULTS.items():
        knob(name, value)


def ill(B, N, seed):
    """The fixture's distribution (tests/golden/make_golden.py: ill_conditioned_qp) at any size."""
    g = torch.Generator().manual_seed(seed)
    p = torch.exp(4 * (torch.rand(B, N, generator=g, dtype=torch.float64) * 20 - 10))
    return {"P": torch.diag_embed(p).contiguous(), "q": torch.rand(B, N, 1, generator=g, dtype=torch.float64) * 2 - 1,
            "grad_x": torch.randn(B, N, 1, generator=g, dtype=torch.float64)}


def npy(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def classes(x, it, max_iter):
    nan = np.isnan(x.reshape(x.shape[0], -1)).any(1)
    return np.where(nan, NAN, np.where(np.asarray(it) >= max_iter, CAPPED, CONVERGED))


def rel_err(xh, xo):
    """max|xh - xo| / max|xo| per problem (0 / 0 = 0; anything / 0 = inf)."""
    B = xo.shape[0]
    err = np.abs(xh - xo).reshape(B, -1).max(1)
    scale = np.abs(xo).reshape(B, -1).max(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), np.where(err == 0, 0.0, np.inf))


def compare(xh, ith, xo, ito, max_iter, min_class=1.0, min_iters=0.0, tol=None, well=False, median_tol=1e-11):
    """The one comparison of this file (module docstring).  tol: on x where the class is "converged" on both sides and the
    iteration counts agree (None: reported, not asserted).  well=True (well-conditioned batches, where nothing excuses a
    different answer): tol on EVERY problem that is not NaN or capped on both sides, and the median error <= 1e-11 as in
    the parity suite (test_gpu_parity.check_forward).  Returns the measured figures."""
    xh, ith, xo, ito = npy(xh), npy(ith), np.asarray(xo), np.asarray(ito)
    B = xo.shape[0]
    assert not np.isinf(xh).any(), "an infinity in x"
    hn = np.isnan(xh.reshape(B, -1))
    assert (hn.any(1) == hn.all(1)).all(), "a problem that is NaN in some coordinates only"
    ch, co = classes(xh, ith, max_iter), classes(xo, ito, max_iter)
    same_class = ch == co
    agree = same_class & (ith == ito) & (co == CONVERGED)   # (a capped x is where a trajectory happens to be)
    if well:
        agree = ~(((ch == NAN) & (co == NAN)) | ((ch == CAPPED) & (co == CAPPED)))
    err = rel_err(xh[agree], xo[agree]) if agree.any() else np.zeros(0)
    out = {"class": float(same_class.mean()), "iters": float((ith == ito).mean()), "max_rel": float(err.max(initial=0.0)),
           "nan": (int((ch == NAN).sum()), int((co == NAN).sum())), "capped": (int((ch == CAPPED).sum()), int((co == CAPPED).sum()))}
    print("compare", out)
    assert same_class.mean() >= min_class, out
    assert (ith == ito).mean() >= min_iters, out
    assert tol is None or out["max_rel"] <= tol, out
    if well:
        assert np.median(err) <= median_tol, out
    return out


def reference_order(xh, ith, xo, ito, min_iters=0.90, min_bits=0.70):
    """What the reference-order routes keep on this workload (measured on MI355X, 2026-10-16): the oracle's NaN set exactly;
    its iteration counts on 0.906-0.969 of the problems, its bits on 0.703-0.813 -- not all: the device's pow() (rho and
    tau from L / mu, Solver.cpp:72-73) may differ from the host libm's by an ulp, and on this chaotic workload an ulp of
    rho changes a long trajectory."""
    xh, ith = npy(xh), npy(ith)
    B = xo.shape[0]
    same = (ith == ito) & (np.isnan(xh) == np.isnan(xo)).all(axis=(1, 2))
    bits = np.array([np.array_equal(a, b, equal_nan=True) for a, b in zip(xh, xo)])
    print("exact: nan sets %s, iters %.4f, bits %.4f, first differing iters %s" % (
        np.array_equal(np.isnan(xh), np.isnan(xo)), same.mean(), bits.mean(), list(zip(ith[~same], ito[~same]))[:6]))
    assert np.array_equal(np.isnan(xh), np.isnan(xo)), "NaN sets differ"
    assert same.mean() >= min_iters and bits.mean() >= min_bits


def nan_stops(xh, ith, xo, ito, max_iter, min_same):
    """A problem whose shifted diagonal lost positivity stops in the iteration after the rho update, as the reference does:
    never at max_iter, and -- where both sides end it in NaN -- at the oracle's iteration on at least `min_same` of them
    (a problem can lose positivity at another update when its trajectory differed before)."""
    xh, ith = npy(xh), npy(ith)
    nan_h, nan_o = np.isnan(xh).any(axis=(1, 2)), np.isnan(xo).any(axis=(1, 2))
    assert (ith[nan_h] < max_iter).all(), "NaN problems ran to max_iter: %s" % np.sort(ith[nan_h])[-5:]
    both = nan_h & nan_o
    same = float((ith[both] == ito[both]).mean())
    print("NaN problems: %d / %d, the oracle's iteration count on %.4f" % (nan_h.sum(), nan_o.sum(), same))
    assert both.sum() >= 0.8 * nan_o.sum() and same >= min_same, (both.sum(), nan_o.sum(), same)
    return same


def oracle_qp(O, d, max_iter=MAX_ITER, eps=EPS):
    return O.qp_fwd_batch(d["P"].numpy(), d["q"].numpy(), eps, max_iter, nthreads=16)


def hip_qp(ops, d, layout, max_iter=MAX_ITER, eps=EPS):
    P = d["P"].cuda()
    if layout & 0xff == 2:
        P = torch.diagonal(P, dim1=1, dim2=2).contiguous()
    x, it = ops.qp_forward(P, d["q"].cuda(), eps, max_iter, layout=layout, return_iters=True)
    torch.cuda.synchronize()
    return x, it


def check_grads(got, ref, x, exact_bits):
    """Backward on the oracle's x: per problem against the oracle's gradient scale; a gradient entry is finite wherever the
    oracle's is (a NaN x must not reach another problem's gradients)."""
    *gref, sref = ref
    *gh, st = got
    fin = ~np.isnan(x.reshape(x.shape[0], -1)).any(1)
    assert np.array_equal(npy(st)[fin], sref[fin]), "refinement step counts differ"
    for a, b in zip(gh, gref):
        a = npy(a)
        assert (np.isfinite(a) | ~np.isfinite(b))[fin].all(), "a gradient that the oracle has finite is not finite"
        fin = fin & np.isfinite(b.reshape(b.shape[0], -1)).all(1)
        if exact_bits:
            assert np.array_equal(a[fin], b[fin]), "max diff %g" % np.abs(a[fin] - b[fin]).max()
        else:
            assert (rel_err(a[fin], b[fin]) <= 1e-9).all(), rel_err(a[fin], b[fin]).max()


# ---------------------------------------------------------------- the fixture
def test_fixture_on_the_diagonal_route(oracle, ops):
    """golden/conditioning/qp_ill_n8.npz through AUTO (the diagonal kernel): outcome classes, NaN problems stopped as the
    reference stops them; the fixture's gradients (on the oracle's x, NaN problems kept) through the diagonal and the
    team backward."""
    from diffqcqp_amd import _capi
    d = np.load(os.path.join(GOLDEN, "conditioning", "qp_ill_n8.npz"))
    t = {k: torch.from_numpy(d[k]) for k in ("P", "q", "grad_x")}
    # the oracle of THIS host reproduces the fixture (the CPU test pins it bit for bit)
    xo, ito = oracle_qp(oracle, t, int(d["max_iter"]), float(d["eps"]))
    assert np.array_equal(xo, d["x"], equal_nan=True) and np.array_equal(ito, d["iters"])
    xh, ith = hip_qp(ops, t, _capi.P_AUTO)
    r = compare(xh, ith, d["x"], d["iters"], MAX_ITER, min_class=0.90)   # measured 0.906 (2026-10-16)
    assert r["nan"][0] >= 15
    nan_stops(xh, ith, d["x"], d["iters"], MAX_ITER, min_same=NAN_SAME_FIXTURE)
    # backward on the oracle's x (NaN problems kept) through the diagonal, team and lane-per-problem kernels
    P, q, g, x = t["P"].cuda(), t["q"].cuda(), t["grad_x"].cuda(), torch.from_numpy(d["x"]).cuda()
    ref = (d["grad_P"], d["grad_q"], d["ir_steps"])
    check_grads(ops.qp_backward(P, q, x, g, layout=_capi.P_AUTO, return_steps=True), ref, d["x"], True)
    check_grads(ops.qp_backward(torch.diagonal(P, dim1=1, dim2=2).contiguous(), q, x, g, layout=_capi.P_DIAG,
                                return_steps=True), (np.diagonal(d["grad_P"], axis1=1, axis2=2), d["grad_q"], d["ir_steps"]),
                d["x"], True)
    check_grads(ops.qp_backward(P, q, x, g, layout=_capi.P_DENSE, return_steps=True), ref, d["x"], False)


# ---------------------------------------------------------------- 2a: reference arithmetic
@pytest.mark.parametrize("N,layout,max_iter", [(7, 0, MAX_ITER), (9, 0, MAX_ITER), (15, 0, MAX_ITER),
                                               (24, 0x101, MAX_ITER), (32, 0x101, MAX_ITER), (65, 1, 100000)])
def test_reference_order_routes_follow_the_oracle(oracle, ops, N, layout, max_iter):
    """FwdLds (AUTO at odd N <= 16, DENSE | DQQ_F_REFERENCE_ORDER at 16 < N <= 64) and FwdAny (N > 64): the oracle's NaN
    set, most of its iteration counts and bits (reference_order); the backward on the oracle's x within 1e-9 of each
    problem's scale."""
    d = ill(64, N, 3000 + N)
    xo, ito = oracle_qp(oracle, d, max_iter)
    xh, ith = hip_qp(ops, d, layout, max_iter)
    reference_order(xh, ith, xo, ito)
    P, q, g = d["P"].cuda(), d["q"].cuda(), d["grad_x"].cuda()
    ref = oracle.qp_bwd_batch(d["P"].numpy(), d["q"].numpy(), xo, d["grad_x"].numpy(), nthreads=16)
    check_grads(ops.qp_backward(P, q, torch.from_numpy(xo).cuda(), g, layout=layout, return_steps=True), ref, xo,
                False)


@pytest.mark.parametrize("N,knob_name", [(8, "lane_dense"), (12, "small_fwd")])
def test_reference_order_with_the_fast_general_kernels_off(oracle, ops, N, knob_name):
    """Developer build: DENSE N = 8 / 12 without the lane-per-problem / team kernel is the LDS kernel (measured: iteration
    counts on 0.922, bits on 0.766 / 0.797)."""
    from diffqcqp_amd import _capi
    d = ill(64, N, 3100 + N)
    xo, ito = oracle_qp(oracle, d)
    knob(knob_name, 0)
    try:
        xh, ith = hip_qp(ops, d, _capi.P_DENSE)
    finally:
        knob(knob_name, 1)
    reference_order(xh, ith, xo, ito)


# ---------------------------------------------------------------- 2b: every layout, the same bits
def layouts_reference(ops, B, mi):
    d = ill(B, 8, 3200 + B)
    x0, i0 = (npy(t) for t in hip_qp(ops, d, 0, mi))
    assert np.isnan(x0).any() and (i0 >= mi).any()   # the workload's three classes are all there
    if B >= 57344:
        # two lanes per problem, 32 problems per wave: the first re-spread moves a tile's survivors once at most 16 still
        # run, the second once at most 8 do (from iteration 48 on).  Both happen in most tiles of this batch:
        t = -np.sort(-i0[: B // 32 * 32].reshape(-1, 32), axis=1)   # iteration counts of each tile, descending
        assert (t[:, 16] < t[:, 0]).mean() > 0.9 and ((t[:, 8] < t[:, 0]) & (t[:, 0] > 48)).mean() > 0.9
    return d, x0, i0


def same_bits(ops, d, x0, i0, mi, what):
    from diffqcqp_amd import _capi
    for layout in (_capi.P_AUTO, _capi.P_AUTO | _capi.F_EXPECT_DENSE, _capi.P_DIAG):
        x, it = hip_qp(ops, d, layout, mi)
        assert np.array_equal(npy(x), x0, equal_nan=True) and np.array_equal(npy(it), i0), (what, layout)


@pytest.mark.parametrize("B", [4096, 60000])
def test_diag_forward_is_the_same_whatever_the_neighbours(ops, B):
    """AUTO, AUTO | DQQ_F_EXPECT_DENSE (one lane per problem) and DIAG, and the batch in another order: the same x,
    iteration counts and NaN positions."""
    mi = 100000
    d, x0, i0 = layouts_reference(ops, B, mi)
    same_bits(ops, d, x0, i0, mi, "hints")
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(B))
    x, it = hip_qp(ops, {k: v[perm] for k, v in d.items()}, 0, mi)
    assert np.array_equal(npy(x), x0[perm.numpy()], equal_nan=True) and np.array_equal(npy(it), i0[perm.numpy()])


@pytest.mark.parametrize("B", [4096, 60000])
@pytest.mark.parametrize("variant", [{"fwd_lpp": 1}, {"fwd_lpp": 2}, {"fwd_lpp": 4}, {"fuse_fallback": 0},
                                     {"fuse_fallback": 1}, {"fwd_respread": 0}, {"fwd_respread2": 0},
                                     {"fwd_respread2_from": 0}], ids=lambda v: "%s=%s" % next(iter(v.items())))
def test_diag_forward_is_the_same_on_every_layout(ops, B, variant):
    """Developer build: fwd_diag at 1, 2 and 4 lanes per problem, fused and queued fallback, the re-spreads off or from
    the first iteration: DESIGN section 3's "every variant gives the same bits" on the workload where the tails are long."""
    mi = 100000
    for name, value in variant.items():   # (skips here on the shipped build, before any GPU work)
        knob(name, value)
    for name in variant:
        knob(name, KNOB_DEFAULTS[name])
    d, x0, i0 = layouts_reference(ops, B, mi)
    try:
        for name, value in variant.items():
            knob(name, value)
        same_bits(ops, d, x0, i0, mi, variant)
    finally:
        for name in variant:
            knob(name, KNOB_DEFAULTS[name])


# ---------------------------------------------------------------- 2c: the fast routes against the oracle
# (N, layout, B): DIAG and AUTO on the diagonal kernel; DENSE N = 8 up to B = 32768 the group solve inside it, beyond the
# lane-per-problem kernel (also N = 2 / 4 / 6); N = 12 / 16 the team kernel; N = 32 the wave kernel on the matrix cores.
FAST = [(N, lay, 2048) for N in (2, 4, 8, 16, 32, 64) for lay in (0, 2)] + [
    (8, 1, 2048), (8, 1, 32769), (2, 1, 2048), (4, 1, 2048), (6, 1, 2048), (12, 1, 1024), (16, 1, 1024), (32, 1, 256)]
# Measured on MI355X (2026-10-16), max_iter = 1e5: the outcome class (NaN / capped / converged) agrees with the oracle's on
# 0.923 (DENSE N = 8, B = 32769, lane per problem) to 1.0 of the problems, iteration counts on 0.24 - 0.97.  Where both
# converged in the same number of iterations x still differs by up to 53x the problem's scale (lane per problem; diagonal
# kernel 0.93): at rho ~ 1e-4 the dual test rho |dx| < 1e-10 passes wherever the trajectory is, so x is compared only
# by class here.
MIN_CLASS = 0.92
# Problems NaN on both sides that stop at the oracle's iteration: measured 0.981 (N = 4 lane per problem) - 1.0
# (2026-10-16); the 64-problem fixture 1.0
NAN_SAME, NAN_SAME_FIXTURE = 0.98, 1.0


@pytest.mark.parametrize("N,layout,B", [(8, 2, 2048), (8, 0, 2048), (8, 1, 2048), (4, 1, 2048), (12, 1, 1024)],
                         ids=lambda v: str(v))
def test_fast_routes_box_qp_against_the_oracle(oracle, ops, N, layout, B):
    """The box QP takes the same exit on `bad` (QP_LIKE): the workload with bounds of the size of x (|x| up to 2.5e17;
    bounds +-U(0.5, 1.5) 1e12, active on part of the coordinates)."""
    mi = 100000
    d = ill(B, N, 3900 + N + B)
    g = torch.Generator().manual_seed(3950 + N)
    lo = -1e12 * (torch.rand(B, N, 1, generator=g, dtype=torch.float64) + 0.5)
    hi = 1e12 * (torch.rand(B, N, 1, generator=g, dtype=torch.float64) + 0.5)
    xo, ito = oracle.boxqp_fwd_batch(d["P"].numpy(), d["q"].numpy(), lo.numpy(), hi.numpy(), EPS, mi, nthreads=16)
    P = torch.diagonal(d["P"], dim1=1, dim2=2).contiguous() if layout == 2 else d["P"]
    xh, ith = ops.boxqp_forward(P.cuda(), d["q"].cuda(), lo.cuda(), hi.cuda(), EPS, mi, layout=layout, return_iters=True)
    assert np.isnan(xo).any() and ((xo == lo.numpy()) | (xo == hi.numpy())).any()
    compare(xh, ith, xo, ito, mi, min_class=MIN_CLASS)
    nan_stops(xh, ith, xo, ito, mi, min_same=NAN_SAME)


@pytest.mark.parametrize("N,layout,B", FAST, ids=lambda v: str(v))
def test_fast_routes_against_the_oracle(oracle, ops, N, layout, B):
    mi = 100000
    d = ill(B, N, 3300 + N + B)
    xo, ito = oracle_qp(oracle, d, mi)
    xh, ith = hip_qp(ops, d, layout, mi)
    compare(xh, ith, xo, ito, mi, min_class=MIN_CLASS)
    nan_stops(xh, ith, xo, ito, mi, min_same=NAN_SAME)


@pytest.mark.parametrize("N,layout", [(8, 0), (8, 2), (8, 1), (4, 1), (16, 1), (12, 1), (16, 0)])
def test_bad_problems_do_not_poison_their_neighbours(oracle, ops, N, layout):
    """Ill-conditioned problems interleaved with well-conditioned ones: the latter as in the parity suite."""
    a, b = ill(96, N, 3400 + N), make_problem("qp", 96, N, 3500 + N)
    d = {k: torch.stack([a[k], b[k]], 1).reshape((192,) + a[k].shape[1:]) for k in ("P", "q", "grad_x")}
    xo, ito = oracle_qp(oracle, d, 20000, 1e-7)
    xh, ith = (npy(t) for t in hip_qp(ops, d, layout, 20000, 1e-7))
    assert np.isnan(xo[0::2]).any()
    well = slice(1, None, 2)
    assert (npy(ith)[well] == ito[well]).mean() >= 0.99
    assert np.abs(npy(xh)[well] - xo[well]).max() <= 1e-6
    compare(xh[0::2], ith[0::2], xo[0::2], ito[0::2], 20000, min_class=MIN_CLASS)


@pytest.mark.parametrize("N,layout,B", [(8, 2, 256), (8, 1, 256), (8, 1, 24576), (12, 1, 256), (4, 1, 16384)])
def test_backward_with_nan_x(oracle, ops, N, layout, B):
    """bwd_diag, bwd_small (team per problem), bwd_lane_dense: a NaN x makes only that problem's gradients NaN."""
    d = ill(B, N, 3600 + N + B)
    xo, _ = oracle_qp(oracle, d, 2000)
    assert np.isnan(xo).any()
    P, q, g = d["P"].cuda(), d["q"].cuda(), d["grad_x"].cuda()
    if layout == 2:
        P = torch.diagonal(P, dim1=1, dim2=2).contiguous()
    got = ops.qp_backward(P, q, torch.from_numpy(xo).cuda(), g, layout=layout, return_steps=True)
    ref = list(oracle.qp_bwd_batch(d["P"].numpy(), d["q"].numpy(), xo, d["grad_x"].numpy(), nthreads=16))
    if layout == 2:
        ref[0] = np.diagonal(ref[0], axis1=1, axis2=2)
    check_grads(got, ref, xo, layout == 2)


# ---------------------------------------------------------------- 2d: magnitudes
SCALES = [(40, 0), (-40, 0), (0, 40), (0, -40), (40, 40), (-40, -40), (40, -40), (-40, 40)]
ROUTES = [(8, 2, 256), (8, 0, 256), (8, 1, 256), (8, 1, 32769), (4, 1, 512), (12, 1, 256), (32, 1, 64), (32, 2, 64),
          (7, 0, 128), (65, 1, 16)]


def scaled(kind, N, B, seed, k, j):
    d = make_problem("box" if kind == "box" else kind, B, N if kind != "qcqp" or N % 2 == 0 else N + 1, seed)
    d["P"] = d["P"] * 2.0 ** k
    d["q"] = d["q"] * 2.0 ** j
    for name in ("l_n", "l_min", "l_max"):   # constraints on x, whose scale is q / p
        if name in d:
            d[name] = d[name] * 2.0 ** (j - k)
    return d


def run_kind(O, ops, kind, d, layout, eps, mi, mu_prox=1e-7):
    P = d["P"]
    Ph = torch.diagonal(P, dim1=1, dim2=2).contiguous() if layout == 2 else P
    Ph, q = Ph.cuda(), d["q"].cuda()
    if kind == "qp":
        xo, ito = O.qp_fwd_batch(P.numpy(), d["q"].numpy(), eps, mi, mu_prox=mu_prox, nthreads=16)
        xh, ith = ops.qp_forward(Ph, q, eps, mi, mu_prox=mu_prox, layout=layout, return_iters=True)
    elif kind == "qcqp":
        xo, ito = O.qcqp_fwd_batch(P.numpy(), d["q"].numpy(), d["l_n"].numpy(), d["mu"].numpy(), eps, mi, mu_prox=mu_prox,
                                   nthreads=16)
        xh, ith = ops.qcqp_forward(Ph, q, d["l_n"].cuda(), d["mu"].cuda(), eps, mi, mu_prox=mu_prox, layout=layout,
                                   return_iters=True)
    else:
        xo, ito = O.boxqp_fwd_batch(P.numpy(), d["q"].numpy(), d["l_min"].numpy(), d["l_max"].numpy(), eps, mi,
                                    mu_prox=mu_prox, nthreads=16)
        xh, ith = ops.boxqp_forward(Ph, q, d["l_min"].cuda(), d["l_max"].cuda(), eps, mi, mu_prox=mu_prox, layout=layout,
                                    return_iters=True)
    return xh, ith, xo, ito


SWEEP = [(k,) + r for r in ROUTES for k in ("qp", "qcqp", "box") if k != "qcqp" or r[0] % 2 == 0]


@pytest.mark.parametrize("kind,N,layout,B", SWEEP, ids=lambda v: str(v))
def test_magnitude_sweep(oracle, ops, kind, N, layout, B):
    """make_problem batches with P * 2^k, q * 2^j, the constraints scaled with x (q / p) and eps with q; mu_prox = 1e-7 as
    the reference's callers pass it.  Against the oracle as the parity suite does, relative to each problem's scale: x on
    every problem that is not capped on both sides, the median error, iteration counts on >= 99 %.
    P * 2^-40 (P ~ 1e-12, far below mu_prox): L / mu_prox ~ 1e-5, so tau_inc = tau_dec = (L / mu_prox)^0.15 ~ 0.18 < 1
    and the rho adaptation runs backwards (an "increase" multiplies rho by 0.18).  There the QP's outcome class agrees on
    >= 0.994 (a few problems capped in the oracle only) and its iteration counts on >= 0.932 (N = 4 lane per problem;
    measured 2026-10-16), x within 1.4e-13 of the scale on every problem; the QCQP and the box QP do not follow the
    oracle -- the test after the next."""
    for k, j in SCALES:
        if k < 0 and kind != "qp":
            continue
        d = scaled(kind, N, B, 3700 + N + (k + 64) * 3 + j, k, j)
        xh, ith, xo, ito = run_kind(oracle, ops, kind, d, layout, 1e-7 * 2.0 ** j, 1000)
        print(kind, N, layout, B, k, j, end=" ")
        compare(xh, ith, xo, ito, 1000, min_class=1.0 if k >= 0 else 0.99, min_iters=0.99 if k >= 0 else 0.93, tol=1e-6,
                well=True)


@pytest.mark.parametrize("kind,N,layout,B", [r for r in SWEEP if r[0] != "qp"], ids=lambda v: str(v))
def test_prox_dominated_results_are_whole(oracle, ops, kind, N, layout, B):
    """P * 2^-40, QCQP and box QP: whatever the outcome, no infinity and no problem NaN in some coordinates only.  A contact
    whose norm^2 overflowed used to come out NaN (fast_rsqrt(inf) was NaN) where the reference projects it to (+-0, +-0)."""
    for j in (0, 40, -40):
        d = scaled(kind, N, B, 3700 + N + (-40 + 64) * 3 + j, -40, j)
        xh, ith, xo, ito = run_kind(oracle, ops, kind, d, layout, 1e-7 * 2.0 ** j, 1000)
        compare(xh, ith, xo, ito, 1000, min_class=0.0)


# Open finding: P * 2^-40 with mu_prox fixed, QCQP and box QP.  The oracle caps on about half of the
# problems and no route follows it (the reference-order one included: box, N = 7).  Pinned as a strict expected failure:
# a change of behaviour -- a fix -- turns it into an unexpected pass.
PINNED = [("qcqp", 8, 1, 32769), ("qcqp", 4, 1, 512), ("qcqp", 8, 2, 256), ("box", 8, 2, 256), ("box", 8, 1, 256),
          ("box", 7, 0, 128), ("qcqp", 32, 1, 64)]


@pytest.mark.xfail(strict=True, reason="open: P * 2^-40 below mu_prox, QCQP / box QP (DESIGN section 6)")
@pytest.mark.parametrize("kind,N,layout,B", PINNED, ids=lambda v: str(v))
def test_prox_dominated_qcqp_and_box_do_not_follow_the_oracle(oracle, ops, kind, N, layout, B):
    d = scaled(kind, N, B, 3700 + N + (-40 + 64) * 3, -40, 0)
    xh, ith, xo, ito = run_kind(oracle, ops, kind, d, layout, 1e-7, 1000)
    compare(xh, ith, xo, ito, 1000, min_class=0.99, min_iters=0.93, tol=1e-6, well=True)


@pytest.mark.parametrize("N,layout", [(8, 2), (8, 0), (8, 1), (12, 1), (32, 1), (4, 1)])
def test_subnormal_contact_norm(oracle, ops, N, layout):
    """QCQP with q and l_n scaled by 2^-520: the contact norm^2 of prox_circle is subnormal, where fast_rsqrt's seed
    (v_rsq_f64) may flush."""
    d = make_problem("qcqp", 256, N, 3800 + N)
    d["q"] = d["q"] * 2.0 ** -520
    d["l_n"] = d["l_n"] * 2.0 ** -520
    xh, ith, xo, ito = run_kind(oracle, ops, "qcqp", d, layout, 1e-7 * 2.0 ** -520, 1000)
    n2 = (xo.reshape(256, -1, 2) ** 2).sum(-1)
    assert ((n2 > 0) & (n2 < np.finfo(np.float64).tiny)).any()
    # measured (2026-10-16): x within 4.6e-7 of the scale, iteration counts on 0.977 (N = 4 lane per problem) to 1.0, median
    # error up to 2.6e-10: a norm^2 near 2^-1040 keeps ~34 significant bits (2^-34 = 6e-11), on either side.  The seeded
    # rsqrt does not flush it.
    compare(xh, ith, xo, ito, 1000, min_class=1.0, min_iters=0.97, tol=1e-6, well=True, median_tol=1e-9)
