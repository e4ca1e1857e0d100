"""-m gpu: the solution check (dqq_check_f64, diffqcqp_amd/csrc/check.hip) on the device -- against the host-compiled core bit
for bit (any NaN equals any NaN: check_ref.same_bits), against the numpy restatement of the definitions within the bound derived
from the inputs (tests/check_ref.py), inside guard bands, end to end behind diagnostics.solve_*_checked, and captured into a graph.

The host reference of a (kind, N, layout) is computed once for 257 problems and shared: the results of a problem do not depend on
the batch around it, so every B <= 257 and every slice is compared with rows of the same arrays."""
import functools
import os

import numpy as np
import pytest
import torch

import check_ref as R
from conftest import make_problem

pytestmark = pytest.mark.gpu

NS = (2, 3, 8, 16, 17, 32, 64, 65, 130)
BS = (1, 63, 64, 65, 257)
BMAX = 257
KN = [(k, N) for k in R.KINDS for N in NS if not (k == "qcqp" and N % 2)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def faces():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from diffqcqp_amd import build, _capi
    build.build()
    mod = _capi.pybind_lib()
    assert mod is not None, "the pybind11 module was not built"
    return {"pybind11": mod, "ctypes": _capi.ctypes_lib()}


@functools.lru_cache(maxsize=None)
def host(kind, N, diag):
    """(inputs, iters, max_iter, status, resid) of the shared 257-problem batch: a random x, a NaN, an Inf, every iters case."""
    P, q, extras, x = R.make_batch(kind, BMAX, N, 900 + N, diag)
    x[5, N - 1] = np.nan
    x[70, 0] = np.inf
    if diag:
        P[9, N // 2] = np.inf
    else:
        P[9, N - 1, N // 2] = np.inf
    iters = np.random.default_rng(N).integers(1, 14, BMAX).astype(np.int32)   # max_iter = 10: below, at, above
    iters[11] = -1
    st, rs = R.host_check(R.hostcore(), kind, P, q, extras, x, iters, 10, diag)
    st0, rs0 = R.reference(kind, P, q, extras, x, iters, 10, diag)
    assert np.array_equal(st, st0) and set(st) == {0, 1, 2}
    R.assert_close(rs, rs0, P, q, x, diag, "host core")
    return (P, q, extras, x), iters, 10, st, rs


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def run(lib, kind, P, q, extras, x, iters, max_iter, layout, want_resid=True, want_status=True, want_counts=True, stream=None):
    """One dqq_check_f64 call on device tensors through a face of the library -> (status, resid, counts) numpy (or None)."""
    B, N = x.shape
    ex = list(extras) + [None] * (3 - len(extras))
    resid = torch.full((B, 4), -7.0, dtype=torch.float64, device="cuda") if want_resid else None
    status = torch.full((B,), -7, dtype=torch.int32, device="cuda") if want_status else None
    counts = torch.zeros(3, dtype=torch.int64, device="cuda") if want_counts else None
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = lib.dqq_check_f64(R.KIND_ID[kind], ptr(P), ptr(q), ptr(ex[0]), ptr(ex[1]), ptr(ex[2]), ptr(x), ptr(iters),
                           max_iter, B, N, layout, ptr(resid), ptr(status), ptr(counts), s.cuda_stream or None)
    assert rc == 0, rc
    s.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (status, resid, counts))


def expect(got, st, rs, what):
    status, resid, counts = got
    if status is not None:
        assert np.array_equal(status, st), what
    if resid is not None:
        assert R.same_bits(resid, rs), "%s: device and host core differ in %d of %d entries" % (
            what, (resid.view(np.uint64) != rs.view(np.uint64)).sum(), rs.size)
    if counts is not None:
        assert counts.sum() == len(st) and np.array_equal(counts, np.bincount(st, minlength=3)), (what, counts)


@pytest.mark.parametrize("kind,N", KN)
def test_device_equals_host_core(faces, kind, N):
    """Every layout, every B (partial waves and partial tiles), and the batch slice t[1:] of every input."""
    lib = faces["pybind11"]
    for layout in (R.DENSE, R.AUTO, R.DIAG):
        diag = layout == R.DIAG
        (P, q, extras, x), iters, max_iter, st, rs = host(kind, N, diag)
        tP, tq, tx, ti = dev(P), dev(q), dev(x), dev(iters)
        te = [dev(e) for e in extras]
        for B in BS:
            got = run(lib, kind, tP[:B], tq[:B], [e[:B] for e in te], tx[:B], ti[:B], max_iter, layout)
            expect(got, st[:B], rs[:B], "%s N=%d layout=%d B=%d" % (kind, N, layout, B))
        got = run(lib, kind, tP[1:], tq[1:], [e[1:] for e in te], tx[1:], ti[1:], max_iter, layout)
        expect(got, st[1:], rs[1:], "%s N=%d layout=%d slice" % (kind, N, layout))


@pytest.mark.parametrize("face", ["ctypes", "pybind11"])
@pytest.mark.parametrize("kind,N,layout", [("qp", 3, R.AUTO), ("qcqp", 8, R.AUTO), ("box", 64, R.DENSE), ("sbox", 130, R.DIAG),
                                           ("sbox", 17, R.DENSE), ("qcqp", 130, R.DENSE)])
def test_both_faces_outputs_streams_and_the_empty_batch(faces, face, kind, N, layout):
    lib = faces[face]
    diag = layout == R.DIAG
    (P, q, extras, x), iters, max_iter, st, rs = host(kind, N, diag)
    B = 65
    t = [dev(P[:B]), dev(q[:B]), [dev(e[:B]) for e in extras], dev(x[:B]), dev(iters[:B])]
    what = "%s %s N=%d" % (face, kind, N)
    expect(run(lib, kind, *t, max_iter, layout), st[:B], rs[:B], what)
    expect(run(lib, kind, *t, max_iter, layout, want_resid=False), st[:B], rs[:B], what + " status only")
    expect(run(lib, kind, *t, max_iter, layout, want_status=False, want_counts=False), st[:B], rs[:B], what + " resid only")
    side = torch.cuda.Stream()                       # a non-default stream
    side.wait_stream(torch.cuda.current_stream())
    expect(run(lib, kind, *t, max_iter, layout, stream=side), st[:B], rs[:B], what + " side stream")
    # without iters nothing is capped
    t[4] = None
    st_free = np.where(st[:B] == 1, 0, st[:B])
    expect(run(lib, kind, *t, 0, layout), st_free, rs[:B], what + " no iters")
    # B = 0: returns 0 without a launch, whatever the pointers
    assert lib.dqq_check_f64(R.KIND_ID[kind], None, None, None, None, None, None, None, 0, 0, N, layout, None, None, None,
                             None) == 0


@pytest.mark.parametrize("kind,N,layout", [(k, N, l) for k in R.KINDS for N in (3, 8, 130) for l in (R.AUTO, R.DIAG)
                                           if not (k == "qcqp" and N % 2)])
def test_nothing_is_written_outside_the_outputs(faces, kind, N, layout):
    """resid, status and counts inside one poisoned arena: B * 32, B * 4 and 24 bytes change, nothing else."""
    lib = faces["pybind11"]
    (P, q, extras, x), iters, max_iter, st, rs = host(kind, N, layout == R.DIAG)
    B, GAP, POISON = 65, 512, 0xA5
    at_resid, at_status = GAP, GAP + B * 32 + GAP
    at_counts = (at_status + B * 4 + GAP + 7) // 8 * 8
    size = at_counts + 24 + GAP
    arena = torch.full((size,), POISON, dtype=torch.uint8, device="cuda")
    arena[at_counts:at_counts + 24] = 0              # counts is the caller's to zero
    base = arena.data_ptr()
    assert base % 8 == 0
    ex = [dev(e[:B]) for e in extras] + [None] * (3 - len(extras))
    tP, tq, tx, ti = dev(P[:B]), dev(q[:B]), dev(x[:B]), dev(iters[:B])
    rc = lib.dqq_check_f64(R.KIND_ID[kind], ptr(tP), ptr(tq), ptr(ex[0]), ptr(ex[1]), ptr(ex[2]), ptr(tx), ptr(ti), max_iter,
                           B, N, layout, base + at_resid, base + at_status, base + at_counts, None)
    assert rc == 0
    torch.cuda.synchronize()
    a = arena.cpu().numpy()
    outside = np.ones(size, dtype=bool)
    for lo, n in ((at_resid, B * 32), (at_status, B * 4), (at_counts, 24)):
        outside[lo:lo + n] = False
    assert (a[outside] == POISON).all(), "bytes outside the outputs changed at %s" % np.nonzero(outside & (a != POISON))[0][:8]
    got = (a[at_status:at_status + B * 4].view(np.int32), a[at_resid:at_resid + B * 32].view(np.float64).reshape(B, 4),
           a[at_counts:at_counts + 24].view(np.int64))
    expect(got, st[:B], rs[:B], "arena")


# ---------------------------------------------------------------- end to end: diagnostics.solve_*_checked
def _batch(kind, B=256, N=8):
    """A well-conditioned batch (conftest.make_problem: P = diag(U(0.1, 1.1)) with every third problem dense) whose q has a
    negative entry in every problem that the constraints let x follow: x = 0 is not the solution, so no solve ends in its first
    iteration."""
    d = make_problem(kind, B, N, 4200 + R.KIND_ID[kind], "mixed")
    d["q"][:, 0, 0] = -d["q"][:, 0, 0].abs() - 0.05
    if kind == "sbox":   # ... nor may the sign constraint pin that coordinate to 0: sign(v) x <= 0 leaves it x >= 0
        d["v"][:, 0, 0] = -d["v"][:, 0, 0].abs() - 0.05
    names = {"qp": (), "qcqp": ("l_n", "mu"), "box": ("l_min", "l_max"), "sbox": ("l_min", "l_max", "v")}[kind]
    return d["P"], d["q"], [d[n] for n in names]


def _solve(kind, P, q, extras, eps, max_iter):
    from diffqcqp_amd import diagnostics as D
    f = {"qp": D.solve_qp_checked, "qcqp": D.solve_qcqp_checked, "box": D.solve_boxqp_checked,
         "sbox": D.solve_signedboxqp_checked}[kind]
    return f(P.cuda(), q.cuda(), *[e.cuda() for e in extras], eps, max_iter)


def _natural_matches_numpy(kind, P, q, extras, x, info, rows=slice(None)):
    Pn, qn, xn = P.numpy()[rows], q.numpy()[rows, :, 0], x.cpu().numpy()[rows, :, 0]
    en = tuple(e.numpy()[rows, :, 0] for e in extras)
    _, ref = R.reference(kind, Pn, qn, en, xn)
    resid = torch.stack([info.natural, info.infeasibility, info.objective, info.scale], 1).cpu().numpy()[rows]
    R.assert_close(resid, ref, Pn, qn, xn, False, kind)


@pytest.mark.parametrize("kind", R.KINDS)
def test_solve_checked_converged_and_capped(faces, kind):
    P, q, extras = _batch(kind)
    x, info = _solve(kind, P, q, extras, 1e-7, 1000)
    st = info.status.cpu().numpy()
    print("%s: natural residual max %.3e, relative to the scale max %.3e" % (
        kind, info.natural.max().item(), (info.natural / info.scale).max().item()))
    assert (st == 0).all(), np.bincount(st, minlength=3)
    assert info.counts.tolist() == [256, 0, 0]
    _natural_matches_numpy(kind, P, q, extras, x, info)   # (no absolute bound on `natural` itself: none is derived from eps)
    x, info = _solve(kind, P, q, extras, 1e-7, 2)
    assert (info.status.cpu().numpy() == 1).all() and info.counts.tolist() == [0, 256, 0]


@pytest.mark.parametrize("kind", R.KINDS)
def test_solve_checked_flags_exactly_the_nan_problems(faces, kind):
    P, q, extras = _batch(kind)
    bad = np.array([0, 3, 17, 64, 100, 101, 255])
    P = P.clone()
    P[torch.from_numpy(bad), 2, :] = float("nan")
    x, info = _solve(kind, P, q, extras, 1e-7, 1000)
    st = info.status.cpu().numpy()
    want = np.zeros(256, dtype=np.int32)
    want[bad] = 2
    assert np.array_equal(st, want), "status 2 at %s, expected %s; others %s" % (np.nonzero(st == 2)[0], bad, np.nonzero(st == 1)[0])
    good = np.setdiff1d(np.arange(256), bad)
    _natural_matches_numpy(kind, P, q, extras, x, info, good)


def test_ill_conditioned_fixture_classes(faces):
    """golden/conditioning/qp_ill_n8.npz: the status classes equal the classes the forward's own x and iters spell out (NaN /
    capped / converged) on 64 of 64 problems -- the kernel against its definition, not against the oracle."""
    from diffqcqp_amd import diagnostics as D
    d = np.load(os.path.join(GOLDEN, "conditioning", "qp_ill_n8.npz"))
    max_iter = int(d["max_iter"])
    P, q = torch.from_numpy(d["P"]).cuda(), torch.from_numpy(d["q"]).cuda()
    x, info = D.solve_qp_checked(P, q, float(d["eps"]), max_iter)
    from diffqcqp_amd import ops
    x2, iters = ops.qp_forward(P, q, float(d["eps"]), max_iter, return_iters=True)
    assert torch.equal(x.view(torch.int64), x2.view(torch.int64))
    xn, it = x.cpu().numpy().reshape(64, -1), iters.cpu().numpy()
    classes = np.where(np.isnan(xn).any(1), 2, np.where(it >= max_iter, 1, 0))
    st = info.status.cpu().numpy()
    print("classes (converged, capped, NaN):", np.bincount(classes, minlength=3))
    assert np.array_equal(st, classes), "differ at %s" % np.nonzero(st != classes)[0]
    assert info.counts.tolist() == list(np.bincount(classes, minlength=3))


def test_forward_and_check_captured_into_a_graph(faces):
    """Forward + check captured into a HIP graph (warm-up on the capture stream first): the replay equals the eager run bit for
    bit, on the captured inputs and on new ones."""
    from diffqcqp_amd import ops
    B, N = 2051, 8
    d1, d2 = make_problem("qcqp", B, N, 8400, "mixed"), make_problem("qcqp", B, N, 8401, "mixed")
    keys = ("P", "q", "l_n", "mu")
    t = {k: d1[k].cuda().clone() for k in keys}
    x = torch.empty(B, N, 1, dtype=torch.float64, device="cuda")
    out = (torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, 4, dtype=torch.float64, device="cuda"),
           torch.empty(3, dtype=torch.int64, device="cuda"))
    iters = []

    def step():
        _, it = ops.qcqp_forward(t["P"], t["q"], t["l_n"], t["mu"], 1e-7, 40, out=x, return_iters=True)
        iters.append(it)
        ops.solution_check("qcqp", t["P"], t["q"], (t["l_n"], t["mu"]), x, iters=it, max_iter=40, out=out)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager = [o.clone() for o in out]
    assert eager[2].sum().item() == B
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        step()
    for o in out:
        o.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    for o, e in zip(out, eager):
        assert torch.equal(o.view(-1).view(torch.uint8), e.view(-1).view(torch.uint8)), "replay differs from the eager call"
    for k in keys:
        t[k].copy_(d2[k])
    graph.replay()
    torch.cuda.synchronize()
    replayed = [o.clone() for o in out]
    with torch.cuda.stream(s):
        step()
    torch.cuda.synchronize()
    for o, e in zip(out, replayed):
        assert torch.equal(o.view(-1).view(torch.uint8), e.view(-1).view(torch.uint8)), "second replay differs (new inputs)"
    assert replayed[2].sum().item() == B
