"""The signed box QP's backward, dqq_signedboxqp_bwd_f64, on every box backward route (-m gpu).

The signed box QP is the box QP on the effective bounds (lo', hi') the sign constraint leaves (include/diffqcqp_hip.h), so the
yardstick is the library's own box backward at (lo', hi') -- lo', hi' and the keep masks computed here with torch
(tests/sbox_cases.py), never by the code under test -- bit for bit; then the oracle, the call contract, the autograd Function and
finite differences of the signed FORWARD.  x always comes from the signed forward of the same batch.  The batches mix in the
coordinates `make_problem("sbox", ...)` never produces: v = +-0.0, a box on the wrong side of the sign constraint, bounds that
are 0 themselves (tests/sbox_cases.py)."""
import numpy as np
import pytest
import torch

from conftest import make_problem
from sbox_cases import N_CASES, effective_bounds, make_sbox_batch
from test_gpu_worklist_guard import _header_is_idle

pytestmark = pytest.mark.gpu

AUTO, DENSE, DIAG = 0, 1, 2
E_NULLPTR, E_WORKSPACE = -1, -5
OUTS = ("grad_P", "grad_q", "grad_l_min", "grad_l_max", "gamma", "dgamma", "ir_steps")
SENTINEL, STEP_SENTINEL, PAD = -7.25, -77, 3


@pytest.fixture(scope="module")
def ops():
    from diffqcqp_amd import build, ops as _ops, _capi
    build.build()
    _capi.lib()
    return _ops


def npy(t):
    return t.detach().cpu().numpy()


# ---- one row per route: (N, B, p_layout, structure); tests/test_sbox_routes.py pins the kernels they reach
ROWS = {"a": (8, 97, DIAG, "compact"), "b": (8, 97, AUTO, "diag+cache"), "c": (8, 193, AUTO, "third-tile"),
        "d": (2, 97, DENSE, "dense"), "e": (5, 97, DENSE, "dense"), "f": (16, 97, DENSE, "dense"),
        "g": (21, 33, DENSE, "dense"), "h": (22, 17, DENSE, "dense"), "i": (32, 65, AUTO, "some-dense")}
_batches = {}


def batch(ops, row):
    """-> dict of device tensors for a row, computed once: inputs, x of the signed forward, (lo', hi', keep_lo, keep_hi),
    the forward's (pdiag, flags) where the row uses them, and the P (B,N,N) the oracle reads."""
    if row in _batches:
        return _batches[row]
    N, B, layout, structure = ROWS[row]
    d, case = make_sbox_batch(B, N, 4200 + ord(row), "dense" if structure == "dense" else "diag")
    P = d["P"]
    if structure in ("third-tile", "some-dense"):
        dense = make_problem("box", B, N, 4300 + ord(row), "dense")["P"]
        T = 128 // N                                   # problems per wave tile of bwd_diag_kernel
        sel = ((torch.arange(B) // T) % 3 == 1) if structure == "third-tile" else (torch.arange(B) % 7 == 1)
        P = torch.where(sel.view(B, 1, 1), dense, P)
    t = {k: d[k].cuda().contiguous() for k in ("q", "l_min", "l_max", "v", "grad_x")}
    t["P_full"] = P.contiguous().cuda()
    t["P"] = torch.diagonal(P, dim1=1, dim2=2).contiguous().cuda() if structure == "compact" else t["P_full"]
    cache = ops.diag_cache(t["q"]) if structure == "diag+cache" else None
    t["x"] = ops.boxqp_forward(t["P"], t["q"], t["l_min"], t["l_max"], 1e-7, 1000, v=t["v"], layout=layout, cache=cache)
    t["lo_eff"], t["hi_eff"], t["keep_lo"], t["keep_hi"] = effective_bounds(t["l_min"], t["l_max"], t["v"])
    t["cache"] = cache
    # the batch holds every case, and the forward obeys the effective bounds
    assert sorted(case.unique().tolist()) == list(range(N_CASES))
    assert bool(((t["x"] >= t["lo_eff"] - 1e-9) & (t["x"] <= t["hi_eff"] + 1e-9)).all())
    if cache is not None:
        assert bool((cache[1] == 1).all())
    torch.cuda.synchronize()
    _batches[row] = t
    return t


def workspace(ops, N, B, layout, scratch=True):
    from diffqcqp_amd import _capi
    lib = _capi.lib()
    need = lib.dqq_workspace_bytes(B) + (lib.dqq_scratch_bytes(2, 1, N, B, layout) if scratch else 0)   # the KIND-2 query
    return torch.zeros((need + 3) // 4 + 16, dtype=torch.int32, device="cuda"), need


def call(ops, t, N, layout, signed, rows=None, want=OUTS, ws=None, ws_bytes=None, v_null=False, cache=None, expect=0):
    """One raw C-ABI call on rows [rows[0], rows[1]) of the batch: dqq_signedboxqp_bwd_f64(l_min, l_max, v) when `signed`,
    else dqq_boxqp_bwd_f64(lo', hi').  Every output buffer has PAD rows more than the call's B, filled with a sentinel; the
    rows behind B must still hold it afterwards.  -> {name: tensor of B rows} for the outputs in `want`."""
    from diffqcqp_amd import _capi
    lib = _capi.lib()
    r0, r1 = rows if rows is not None else (0, t["q"].shape[0])
    B = r1 - r0
    compact = layout == DIAG
    shapes = {"grad_P": (N,) if compact else (N, N), "grad_q": (N, 1), "grad_l_min": (N, 1), "grad_l_max": (N, 1),
              "gamma": (2 * N,), "dgamma": (2 * N,), "ir_steps": (2,)}
    out = {}
    for k in want:
        if k == "ir_steps":
            out[k] = torch.full((B + PAD,) + shapes[k], STEP_SENTINEL, dtype=torch.int32, device="cuda")
        else:
            out[k] = torch.full((B + PAD,) + shapes[k], SENTINEL, dtype=torch.float64, device="cuda")
    if ws is None:
        ws, ws_bytes = workspace(ops, N, max(B, 1), layout)

    def p(x):
        return None if x is None else x.data_ptr()

    def sl(k):
        return t[k][r0:r1]

    o = [p(out.get(k)) for k in OUTS]
    pd, fl = (None, None) if cache is None else (p(cache[0][r0:r1]), p(cache[1][r0:r1]))
    tail = [p(sl("x")), p(sl("grad_x"))] + o[:6] + [B, N, 1e-10, layout, o[6], pd, fl, p(ws), ws_bytes, ops._raw_stream(0)]
    if signed:
        rc = lib.dqq_signedboxqp_bwd_f64(p(sl("P")), p(sl("q")), p(sl("l_min")), p(sl("l_max")), None if v_null else p(sl("v")),
                                         *tail)
    else:
        rc = lib.dqq_boxqp_bwd_f64(p(sl("P")), p(sl("q")), p(sl("lo_eff")), p(sl("hi_eff")), *tail)
    torch.cuda.synchronize()
    assert rc == expect, rc
    for k, buf in out.items():
        pad = buf[B:]
        assert bool((pad == (STEP_SENTINEL if k == "ir_steps" else SENTINEL)).all()), "%s: written beyond B rows" % k
        if rc != 0:
            assert bool((buf == (STEP_SENTINEL if k == "ir_steps" else SENTINEL)).all()), "%s: written by a refused call" % k
    return {k: buf[:B] for k, buf in out.items()}


def same_bits(a, b):
    a, b = npy(a), npy(b)
    if a.dtype.kind == "f":
        return np.array_equal(a.view(np.int64), b.view(np.int64))
    return np.array_equal(a, b)


def masked(box, keep_lo, keep_hi):
    """What the signed call must return for the bound gradients, from the box call's: its values where the mask holds, +0.0
    elsewhere."""
    zero = torch.zeros_like(box["grad_l_min"])
    return torch.where(keep_lo, box["grad_l_min"], zero), torch.where(keep_hi, box["grad_l_max"], zero)


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", sorted(ROWS))
def test_signed_backward_is_the_box_backward_on_the_effective_bounds(ops, row):
    """Bit for bit, every problem of every row: grad_P, grad_q, gamma, dgamma, ir_steps array_equal; grad_l_min / grad_l_max
    the box call's where the mask holds and +0.0 (not -0.0) elsewhere."""
    from diffqcqp_amd import _capi
    N, B, layout, _ = ROWS[row]
    t = batch(ops, row)
    ws, ws_bytes = workspace(ops, N, B, layout)
    signed = call(ops, t, N, layout, True, ws=ws, ws_bytes=ws_bytes, cache=t["cache"])
    assert _header_is_idle(ws) and not _capi.workspace_status(ws)
    box = call(ops, t, N, layout, False, ws=ws, ws_bytes=ws_bytes, cache=t["cache"])
    for k in ("grad_P", "grad_q", "gamma", "dgamma", "ir_steps"):
        assert np.array_equal(npy(signed[k]), npy(box[k])), (row, k)
        assert not np.isnan(npy(signed[k])).any() and not (npy(signed[k]) == SENTINEL).any(), (row, k)
    glo, ghi = masked(box, t["keep_lo"], t["keep_hi"])
    assert same_bits(signed["grad_l_min"], glo) and same_bits(signed["grad_l_max"], ghi), row
    assert (npy(signed["ir_steps"]) >= 1).all()
    # the masks bite on both sides, and some kept bound gradients are not zero
    for keep, g in ((t["keep_lo"], signed["grad_l_min"]), (t["keep_hi"], signed["grad_l_max"])):
        assert 0.1 < float(keep.double().mean()) < 0.9
        assert float(g.abs().max()) > 1e-3
        assert not bool(torch.signbit(g[~keep]).any()) and bool((g[~keep] == 0).all())
    # and they do something: the box call's own bound gradients are not zero everywhere the mask drops them
    dropped = torch.cat([box["grad_l_min"][~t["keep_lo"]], box["grad_l_max"][~t["keep_hi"]]])
    assert float(dropped.abs().max()) > 1e-3, row


@pytest.mark.parametrize("row", ["a", "e", "f"])
def test_signed_backward_against_the_oracle(oracle, ops, row):
    """The reference-order routes (diagonal fast path, LDS team kernel) against oracle.boxqp_bwd_batch at (lo', hi') on
    identical x: the same bits."""
    N, B, layout, _ = ROWS[row]
    t = batch(ops, row)
    out = call(ops, t, N, layout, True)
    gP, gq, glo, ghi, gam, st, dgam = oracle.boxqp_bwd_batch(npy(t["P_full"]), npy(t["q"]), npy(t["lo_eff"]), npy(t["hi_eff"]),
                                                              npy(t["x"]), npy(t["grad_x"]), nthreads=8, duals=True)
    klo, khi = npy(t["keep_lo"]), npy(t["keep_hi"])
    if layout == DIAG:
        gP = np.ascontiguousarray(np.diagonal(gP, axis1=1, axis2=2))
    for name, ref in (("grad_P", gP), ("grad_q", gq), ("gamma", gam), ("dgamma", dgam), ("ir_steps", st),
                      ("grad_l_min", np.where(klo, glo, 0.0)), ("grad_l_max", np.where(khi, ghi, 0.0))):
        got = npy(out[name])
        print(row, name, "max |diff| %g" % np.abs(got - ref).max())
        assert np.array_equal(got, ref), (row, name, float(np.abs(got - ref).max()))


@pytest.mark.parametrize("row", ["a", "c", "h"])
def test_call_contract(ops, row):
    from diffqcqp_amd import _capi
    N, B, layout, _ = ROWS[row]
    t = batch(ops, row)
    ws, ws_bytes = workspace(ops, N, B, layout)
    full = call(ops, t, N, layout, True, ws=ws, ws_bytes=ws_bytes)
    # each single-output request is the full call's output
    for k in OUTS:
        one = call(ops, t, N, layout, True, want=(k,), ws=ws, ws_bytes=ws_bytes)
        assert same_bits(one[k], full[k]), (row, k)
    # the slice [1:] of every argument gives the unsliced call's rows
    part = call(ops, t, N, layout, True, rows=(1, B), ws=ws, ws_bytes=ws_bytes)
    for k in OUTS:
        assert same_bits(part[k], full[k][1:]), (row, k)
    # B = 0: nothing is launched, nothing is read (not even a workspace)
    assert call(ops, t, N, layout, True, rows=(0, 0), ws=ws, ws_bytes=0, v_null=True)["grad_q"].shape[0] == 0
    # v is required
    call(ops, t, N, layout, True, ws=ws, ws_bytes=ws_bytes, v_null=True, expect=E_NULLPTR)
    # a row of x set to NaN leaves the other problems' outputs as they were (row c: one in a diagonal tile, one in a dense one)
    bad = [5, 20] if row == "c" else [5]
    tn = dict(t, x=t["x"].clone())
    tn["x"][bad] = float("nan")
    nan = call(ops, tn, N, layout, True, ws=ws, ws_bytes=ws_bytes)
    others = [b for b in range(B) if b not in bad]
    for k in OUTS:
        assert same_bits(nan[k][others], full[k][others]), (row, k)
    # the workspace is left as it was found: an idle, clean work-list header
    assert _header_is_idle(ws) and not _capi.workspace_status(ws)
    assert (_capi.lib().dqq_scratch_bytes(2, 1, N, B, layout) > 0) == (row == "h")


def test_too_small_a_workspace_is_refused(ops):
    """N = 22 takes the global-memory kernel: without the scratch of the KIND-2 query behind the work-list the call is refused
    (DQQ_E_WORKSPACE) before anything is launched; with no workspace at all too."""
    from diffqcqp_amd import _capi
    N, B, layout, _ = ROWS["h"]
    t = batch(ops, "h")
    lib = _capi.lib()
    assert lib.dqq_scratch_bytes(3, 1, N, B, layout) == 0 and lib.dqq_scratch_bytes(2, 1, N, B, layout) > 0
    ws, head = workspace(ops, N, B, layout, scratch=False)
    call(ops, t, N, layout, True, ws=ws, ws_bytes=head, expect=E_WORKSPACE)
    call(ops, t, N, layout, True, ws=ws, ws_bytes=head + lib.dqq_scratch_bytes(2, 1, N, B, layout) - 8, expect=E_WORKSPACE)
    call(ops, t, N, layout, True, ws=ws, ws_bytes=0, expect=E_WORKSPACE)
    assert _header_is_idle(ws) and not _capi.workspace_status(ws)


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("structure", ["diag", "dense"])
def test_autograd_function_and_module_api(ops, structure):
    from diffqcqp_amd import diffqcqp as M
    from diffqcqp_amd.qcqp import BoxQPFn2, SignedBoxQPDiffFn2, SignedBoxQPFn2
    B, N = 64, 8
    d, _ = make_sbox_batch(B, N, 4400 + len(structure), structure)
    names = ("P", "q", "l_min", "l_max", "v")
    g = {k: d[k].cuda().requires_grad_(True) for k in names}
    gx = d["grad_x"].cuda()
    warm = torch.zeros_like(gx)
    x = SignedBoxQPDiffFn2.apply(g["P"], g["q"], g["l_min"], g["l_max"], g["v"], warm, 1e-7, 1000)
    assert x.shape == (B, N, 1)
    assert torch.equal(x.detach(), SignedBoxQPFn2.apply(*(g[k].detach() for k in names), warm, 1e-7, 1000))
    (x * gx).sum().backward()
    assert g["v"].grad is None
    # BoxQPFn2's backward on (lo', hi') given the same x
    lo, hi, klo, khi = effective_bounds(g["l_min"].detach(), g["l_max"].detach(), g["v"].detach())
    ref = ops.boxqp_backward(g["P"].detach(), g["q"].detach(), lo, hi, x.detach(), gx)
    want = (ref[0], ref[1], torch.where(klo, ref[2], torch.zeros_like(lo)), torch.where(khi, ref[3], torch.zeros_like(hi)))
    for k, w in zip(names[:4], want):
        assert same_bits(g[k].grad, w), k
    # ... and through BoxQPFn2 itself, whose forward on (lo', hi') is the same problem: x agrees to the solver's tolerance, so the
    # gradients agree to the same (a sanity check on the transform, not on bits)
    bl = {k: g[k].detach().clone().requires_grad_(True) for k in ("P", "q")}
    xb = BoxQPFn2.apply(bl["P"], bl["q"], lo, hi, warm, 1e-7, 1000)
    assert float((xb.detach() - x.detach()).abs().max()) < 1e-5
    # needs_input_grad subsets: only what is asked for comes back, with the same bits
    for subset in (("q",), ("P", "l_max"), ("l_min",)):
        s = {k: d[k].cuda().requires_grad_(k in subset) for k in names}
        xs = SignedBoxQPDiffFn2.apply(s["P"], s["q"], s["l_min"], s["l_max"], s["v"], warm, 1e-7, 1000)
        (xs * gx).sum().backward()
        for k in names:
            assert (s[k].grad is not None) == (k in subset), (subset, k)
            if k in subset:
                assert same_bits(s[k].grad, g[k].grad), (subset, k)
    # CPU tensors are staged and everything comes back on the CPU
    c = {k: d[k].clone().requires_grad_(k != "v") for k in names}
    xc = SignedBoxQPDiffFn2.apply(c["P"], c["q"], c["l_min"], c["l_max"], c["v"], torch.zeros_like(d["q"]), 1e-7, 1000)
    assert not xc.is_cuda and torch.equal(xc.detach(), x.detach().cpu())
    (xc * d["grad_x"]).sum().backward()
    for k in names[:4]:
        assert not c[k].grad.is_cuda and same_bits(c[k].grad, g[k].grad.cpu()), k
    # the module-level twin of solveDerivativesBoxQP, on problem 3 of the batch
    duals = (torch.empty(B, 2 * N, dtype=torch.float64, device="cuda"), torch.empty(B, 2 * N, dtype=torch.float64, device="cuda"))
    gq = ops.boxqp_backward(g["P"].detach(), g["q"].detach(), g["l_min"].detach(), g["l_max"].detach(), x.detach(), gx,
                            duals=duals, v=g["v"].detach())[1]
    blg, gam = M.solveDerivativesSignedBoxQP(*(d[k][3].numpy() for k in names), npy(x)[3], d["grad_x"][3].numpy())
    assert blg.shape == (3 * N,) and gam.shape == (2 * N,)
    if structure == "diag":      # (B = 1 and B = 64 take the same kernel: the same bits; a dense P may take another team width)
        assert np.array_equal(gam, npy(duals[0])[3]) and np.array_equal(blg[:2 * N], npy(duals[1])[3])
        assert np.array_equal(blg[2 * N:], -npy(gq)[3, :, 0])
    else:
        assert np.allclose(gam, npy(duals[0])[3], rtol=1e-9, atol=1e-12)
        assert np.allclose(blg, np.concatenate([npy(duals[1])[3], -npy(gq)[3, :, 0]]), rtol=1e-9, atol=1e-12)
    # SignedBoxQPFn2 itself is what it was: no backward
    xs = SignedBoxQPFn2.apply(g["P"], g["q"], g["l_min"], g["l_max"], g["v"], warm, 1e-7, 1000)
    with pytest.raises(NotImplementedError):
        xs.sum().backward()


# ------------------------------------------------------------------------------------------------------------------
FD_SEED = 9209   # (chosen on the CPU with oracle.boxqp_fwd_batch(..., v=...): 232 pairs survive; free 34, original bound 50, sign bound 148)


def fd_problem_states(P, q, lo_e, hi_e, klo, khi, l_min, l_max, v, x):
    """The differentiability filter of test_gpu_fd.py's box test on the effective bounds, plus what is new here: a bound
    entry that sits on a kink of the bound transform while its effective bound is active.  numpy, one batch.
    -> (problem_ok (B), pair_ok (B,N), free, at_orig, at_sign (B,N), at_lo, at_hi (B,N), r (B,N))"""
    r = np.einsum("bij,bj->bi", P, x) + q
    at_lo, at_hi = np.abs(x - lo_e) < 1e-9, np.abs(x - hi_e) < 1e-9
    free = ~(at_lo | at_hi)
    ok = np.where(free, np.minimum(x - lo_e, hi_e - x) > 1e-4, np.abs(r) > 1e-4)
    problem_ok = ok.all(axis=1)
    kink = np.zeros_like(free)
    for dlo, dhi in ((1e-4, 0.0), (-1e-4, 0.0), (0.0, 1e-4), (0.0, -1e-4)):
        _, _, klo2, khi2 = (npy(a) for a in effective_bounds(torch.from_numpy(l_min + dlo), torch.from_numpy(l_max + dhi),
                                                             torch.from_numpy(v)))
        kink |= (at_lo & (klo2 != klo)) | (at_hi & (khi2 != khi))
    pair_ok = problem_ok[:, None] & ~kink
    at_orig = (at_lo & klo) | (at_hi & khi)
    at_sign = (at_lo & ~klo) | (at_hi & ~khi)
    return problem_ok, pair_ok, free, at_orig & ~at_sign, at_sign, at_lo, at_hi, r


def fd_batch():
    d, _ = make_sbox_batch(32, 8, FD_SEED, "dense", scale=2.5)
    return d


def check_fd_counts(pair_ok, free, at_orig, at_sign):
    """Conditions on the seeded batch (not measurements): half of all (problem, coordinate) pairs survive, and at
    least 20 surviving coordinates sit in each state."""
    assert pair_ok.sum() >= 0.5 * pair_ok.size, int(pair_ok.sum())
    for name, m in (("free", free), ("at an original bound", at_orig), ("at the sign bound 0", at_sign)):
        assert (m & pair_ok).sum() >= 20, (name, int((m & pair_ok).sum()))


def test_gradients_match_central_differences(ops):
    """test_gpu_fd.py's box QP check (same harness, steps and bars: central differences at 1e-6, eps = 1e-12, 5e-5 + 1e-3 |exact|
    against the exact active-set derivative, its Tikhonov bound for analytic against exact) on 32 seeded dense N = 8 signed
    problems through SignedBoxQPDiffFn2, for q, P, l_min, l_max.  Exact derivative: with F the coordinates strictly between
    their EFFECTIVE bounds, dl_F = P_FF^-T g_F, d/d(bound coordinate i sits on) = g_i - P_Fi . dl_F -- credited to l_min / l_max
    only where the effective bound still is that bound, 0 where the sign constraint has replaced it.
    Filter: that test's own, per problem (every coordinate > 1e-4 inside its bounds or with |multiplier| > 1e-4); and per
    (problem, coordinate), new here: the l_min / l_max entries of a coordinate that sits at an effective bound within 1e-4 of
    a kink of the bound transform (a bound that is 0 itself: min(l_max, 0), max(l_min, 0) have no derivative there) are left
    out -- its q and P entries are differentiable and stay.  Tikhonov bound: smin is the smallest NON-ZERO singular value of
    the reference's system; a coordinate pinned at lo' = hi' has two dependent multiplier columns, a null direction the
    refinement iterate (started at 0, it stays in the row space) has no component in."""
    import test_gpu_fd as fdm
    from diffqcqp_amd.qcqp import SignedBoxQPDiffFn2
    nb, N = 32, 8
    d = fd_batch()
    names = ("P", "q", "l_min", "l_max", "v")
    t = {k: d[k].cuda().contiguous() for k in names}
    g = d["grad_x"].cuda()

    def solve(tt):
        with torch.no_grad():
            return SignedBoxQPDiffFn2.apply(tt["P"], tt["q"], tt["l_min"], tt["l_max"], tt["v"], torch.zeros_like(tt["q"]),
                                            fdm.EPS, fdm.MAX_ITER)

    leaves = {k: t[k].clone().requires_grad_(k != "v") for k in names}
    x = SignedBoxQPDiffFn2.apply(*(leaves[k] for k in names), torch.zeros_like(t["q"]), fdm.EPS, fdm.MAX_ITER)
    (x * g).sum().backward()
    x = x.detach()
    grads = {k: leaves[k].grad for k in names[:4]}
    steps = npy(ops.boxqp_backward(t["P"], t["q"], t["l_min"], t["l_max"], x, g, return_steps=True, v=t["v"])[-1])
    entries = fdm.entries_for("box", N)
    # central differences: every perturbed copy of every problem in one forward launch (test_gpu_fd.central_differences, with v)
    m = len(entries)
    rep = {k: v.repeat_interleave(2 * m, dim=0).clone() for k, v in t.items()}
    base = torch.arange(nb, device=g.device) * (2 * m)
    for e, (name, idx) in enumerate(entries):
        for s, sign in enumerate((1.0, -1.0)):
            for ix in idx:
                rep[name][(base + 2 * e + s,) + tuple(ix)] += sign * fdm.H
    val = (solve(rep) * g.repeat_interleave(2 * m, dim=0)).sum(dim=(1, 2)).view(nb, m, 2)
    fd = npy((val[:, :, 0] - val[:, :, 1]) / (2 * fdm.H))
    an = npy(fdm.gather_analytic(grads, entries))
    lo_e, hi_e, klo, khi = (npy(a)[:, :, 0] for a in effective_bounds(t["l_min"], t["l_max"], t["v"]))
    h = {k: npy(v) for k, v in t.items()}
    xs, gs = npy(x)[:, :, 0], npy(g)[:, :, 0]
    problem_ok, pair_ok, free, at_orig, at_sign, at_lo, at_hi, r = fd_problem_states(
        h["P"], h["q"][:, :, 0], lo_e, hi_e, klo, khi, h["l_min"][:, :, 0], h["l_max"][:, :, 0], h["v"][:, :, 0], xs)
    print("surviving pairs %d of %d; free %d, at an original bound %d, at the sign bound %d" %
          (pair_ok.sum(), pair_ok.size, (free & pair_ok).sum(), (at_orig & pair_ok).sum(), (at_sign & pair_ok).sum()))
    check_fd_counts(pair_ok, free, at_orig, at_sign)
    n_q, n_P = N, N * (N + 1) // 2
    replaced_checked, worst_fd, worst_replaced = 0, 0.0, 0.0
    for b in np.where(problem_ok)[0]:
        P = h["P"][b]
        F = np.where(free[b])[0]
        dl = np.zeros(N)
        if F.size:
            dl[F] = np.linalg.solve(P[np.ix_(F, F)].T, gs[b, F])
        gP = -np.outer(dl, xs[b])
        gb = gs[b] - P[F, :].T @ dl[F]
        ex = [-dl[i] for i in range(N)]
        ex += [gP[i, j] if i == j else gP[i, j] + gP[j, i] for i in range(N) for j in range(i + 1)]
        ex += [gb[i] if (at_lo[b, i] and klo[b, i]) else 0.0 for i in range(N)]
        ex += [gb[i] if (at_hi[b, i] and khi[b, i]) else 0.0 for i in range(N)]
        ex = np.array(ex)
        use = np.concatenate([np.ones(n_q + n_P, dtype=bool), pair_ok[b], pair_ok[b]])
        e1 = (np.abs(fd[b] - ex) - (5e-5 + 1e-3 * np.abs(ex)))[use]
        assert e1.max() <= 0, ("FD vs exact derivative", b, float(np.abs(fd[b] - ex)[use].max()))
        worst_fd = max(worst_fd, float(np.abs(fd[b] - ex)[use].max()))
        # a bound the sign constraint has replaced: the analytic gradient is +0.0 and the forward does not move with it
        for off, keep in ((n_q + n_P, klo[b]), (n_q + n_P + N, khi[b])):
            for i in np.where(~keep & pair_ok[b])[0]:
                gname = "l_min" if off == n_q + n_P else "l_max"
                a = float(grads[gname][b, i, 0])
                assert a == 0.0 and not np.signbit(a), (b, i, gname, a)
                assert abs(fd[b, off + i]) <= 5e-5, (b, i, gname, fd[b, off + i])
                worst_replaced = max(worst_replaced, abs(fd[b, off + i]))
                replaced_checked += 1
        # the reference's system for this active set (Solver.cpp:341-350) and its smallest non-zero singular value
        act = [(i, -1.0) for i in range(N) if at_lo[b, i]] + [(i, 1.0) for i in range(N) if at_hi[b, i]]
        both = at_lo[b] & at_hi[b]
        na = len(act)
        A = np.zeros((na + N, na + N))
        for k, (i, sg) in enumerate(act):
            A[k, na + i] = abs(r[b, i]) * (0.5 if both[i] else 1.0)
            A[na + i, k] = sg
        A[na:, na:] = P
        sv = np.linalg.svd(A, compute_uv=False)
        smin = sv[sv > 1e-9 * sv.max()].min()
        damp = (fdm.MU_IR / (smin ** 2 + fdm.MU_IR)) ** int(steps[b, 1])
        scale = max(1.0, float(np.abs(ex).max()))
        bound = 2.0 * damp * scale * np.sqrt(N + na) + 1e-6 * scale
        e2 = float(np.abs(an[b] - ex)[use].max())
        assert e2 <= bound, ("analytic vs exact beyond the Tikhonov bound", b, e2, bound, smin, steps[b].tolist())
    print("worst |FD - exact| %g, worst |FD| w.r.t. a replaced bound %g over %d entries" % (worst_fd, worst_replaced, replaced_checked))
    assert replaced_checked >= 20
