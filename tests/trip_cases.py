"""The cases of tests/test_gpu_trips.py, as data: one row per persistent general-P kernel, at a batch that sends every worker
of its fixed grid through the batch (or the work-list) at least twice and leaves the last trip ragged.

A row is (pass, kind, N, B, p_layout | flags, structure, expected route, per_trip, where per_trip is set).  The route is
written as tests/test_routes.py renders a plan.  per_trip: the problems ONE launch of the row's persistent kernel holds at a
time -- its grid times the problems per workgroup --, read from the launcher named beside it (files of diffqcqp_amd/csrc,
lines as footprint_cases.py cites them: the loop's stride, then the grid).  per_trip() below is the same number as a function
of (launch, kind, N, direct or work-list mode); tests/test_trip_cases.py holds the table against it, against route.cpp and,
for the global-memory kernels, against the library's own count of scratch slices.

The rule for B: n >= 2 * per_trip + 1 and n is no multiple of per_trip, where n = B for a kernel that walks the batch and the
length of the work-list for one that drains it (list_len(): the fast kernels queue whole tiles, one entry per problem, when
any problem of the tile has a non-diagonal P).

Families without a row (CITED): their per_trip, and the test that already takes a list or batch past 2 * per_trip and
compares values.  fsmall has no second trip to test: its grid grows with the batch and with the list in both modes (one
problem per team, fwd_small.hip:125-131,275-276).  The diagonal kernels, the lane-per-problem kernels and the direct mode of
the matrix-core kernels have grids that grow with B or are covered at B = 65536.

Inputs: make_problem's 'mixed' data (problem b has a dense P when b % 3 == 1, a diagonal one otherwise -- the general kernels
take both) on a base batch of 61 problems for N <= 32 and 37 beyond: both prime, so that a worker meets other problems on its
second trip than on its first.  The kernel's batch is the base tiled (problem b is base problem b mod base).  Two problems of
the base are shaped so that what a worker keeps between trips differs as much as the solver allows (no seed gives an empty
active set at N = 70):
  * problem 0: q = 0 -- x = 0 after one iteration, no rho update, nothing active (the signed box: everything active);
  * problem 3: an interior solution of its diagonal P -- q = -|q| (QP), q / 50 (box), sign(v) |q| / 50 (signed box),
    q / 1000 with l_n = mu = 1 (QCQP): no constraint active.
check_heterogeneous() asserts, from the oracle's outputs on the base: iteration counts that differ by 2x and more, a problem
whose rho changes and one whose rho does not (adaptive_rho on and off give other / the same bits), and for the backward rows
active sets of 0 and of >= N / 2 entries (QP, box) or problems with and without active contacts (QCQP)."""
import functools

import numpy as np

from footprint_cases import launch_g, launches
from param_cases import AUTO, DENSE, KIND, REF, F, Bw

K4 = ("qp", "qcqp", "box", "sbox")
ANY_F, ANY_B = "general_any.hip:33,72-75", "general_any.hip:59,72-75"
LDS_F = "dense.hip:25-26,76-78, dense_core.h:101"
TEAM_B = "dense.hip:49-50,111-114, dense_core.h:102-107"
SMALL_B = "bwd_small.hip:41-42,56-58,65-67, small_bwd_core.h:37-52"

ROWS = (
    # ---- fany: 512 workgroups, a problem each.  LDS variant (N <= 98) and global-memory variant
    [(F, k, 70, 1027, DENSE, "mixed", "fany scr", 512, ANY_F) for k in K4] +
    [(F, k, 100, 1027, DENSE, "mixed", "fany scr", 512, ANY_F) for k in ("qp", "qcqp")] +
    # ---- flds: 2 * 1024 workgroups of 4 waves directly, 512 workgroups of wpb waves behind a work-list
    [(F, k, 5, 16387, AUTO, "mixed", "flds", 8192, LDS_F) for k in ("qp", "box", "sbox")] +
    [(F, "qcqp", 18, 16387, DENSE | REF, "mixed", "flds", 8192, LDS_F)] +
    [(F, "qcqp", 32, 3079, AUTO | REF, "mixed", "fdiag/16 + flds ws keep", 1536, LDS_F)] +
    # ---- bany: LDS variant (systems of up to 98 rows), global-memory variant, drain of a work-list
    [(Bw, "qp", 70, 1027, DENSE, "mixed", "bany scr", 512, ANY_B),
     (Bw, "qcqp", 44, 1027, DENSE | REF, "mixed", "bany scr", 512, ANY_B),
     (Bw, "box", 22, 1027, DENSE, "mixed", "bany scr", 512, ANY_B),
     (Bw, "sbox", 22, 1027, DENSE, "mixed", "bany scr", 512, ANY_B),
     (Bw, "qp", 100, 1027, DENSE, "mixed", "bany scr", 512, ANY_B),
     (Bw, "qcqp", 66, 1027, DENSE, "mixed", "bany scr", 512, ANY_B),
     (Bw, "box", 34, 1027, DENSE, "mixed", "bany scr", 512, ANY_B),
     (Bw, "box", 32, 1027, AUTO, "mixed", "bdiag + bany ws scr", 512, ANY_B),
     (Bw, "qcqp", 64, 1583, AUTO | REF, "mixed", "bdiag + bany ws scr", 512, ANY_B)] +
    # ---- bteam: 2048 workgroups of wpb waves of 64 / T teams directly, 512 behind a work-list
    [(Bw, "qp", 5, 131075, DENSE, "mixed", "bteam", 65536, TEAM_B),
     (Bw, "qcqp", 18, 8195, DENSE | REF, "mixed", "bteam", 4096, TEAM_B),
     (Bw, "box", 8, 4099, AUTO, "mixed", "bdiag + bteam ws", 2048, TEAM_B)] +
    # ---- bsmall, direct mode: 4096 workgroups of 4 waves of 6 teams (N = 10)
    [(Bw, "qp", 10, 196613, DENSE, "mixed", "bsmall", 98304, SMALL_B)]
)

# (family, mode): (per_trip, where it is set, the test that takes it past 2 * per_trip and compares values)
CITED = {
    ("fsmall", "both"): (None, "fwd_small.hip:125-131,275-276", "no second trip: the grid is ceil(n / 16), n = B or the list"),
    ("bsmall", "list"): ("512 * launch_g: 16384 (QP N = 8), 10240 (QCQP N = 8)", "bwd_small.hip:41-42,65-67",
                         "test_gpu_parity.py::test_full_size_b65536_n8_dense_p_through_auto[dense-*]: a list of 65536, every "
                         "gradient bit-equal to the DQQ_P_DENSE route's"),
    ("fwave64", "list"): ("2048 (N > 48), 3072 (N > 32), 4096 waves, claimed one entry at a time", "dense_wave64.hip:153,293-294",
                          "test_gpu_parity.py::test_segmented_worklist_uneven_segments[64-4097-dense-*]: x and iters bit-equal "
                          "to the direct launch's; test_worklist_header_is_rezeroed_by_large_drains[32-8195-*]"),
    ("bchol", "list"): ("2048 (N > 32), 3072 waves", "dense_wave64.hip:350,441-442",
                        "test_gpu_parity.py::test_segmented_worklist_uneven_segments[64-4097-dense-qp]: gradients bit-equal to "
                        "the direct launch's; test_worklist_header_is_rezeroed_by_large_drains[32-8195-qp]"),
    ("bqcqp", "list"): ("2048 waves", "bwd_wave_qcqp.hip:38,176",
                        "test_gpu_parity.py::test_worklist_header_is_rezeroed_by_large_drains[32-8195-qcqp]: gradients against "
                        "the direct launch's and bit-equal over three calls"),
    ("bqcqpbig", "list"): ("2048 waves", "bwd_wave_qcqp_big.hip:141,303",
                           "test_gpu_parity.py::test_segmented_worklist_uneven_segments[64-4097-dense-qcqp]: gradients "
                           "bit-equal to the direct launch's"),
}

# rows whose first seed missed a condition of check_heterogeneous
SEED = {}


def row_id(row):
    pas, kind, N, B, layout, structure = row[:6]
    return "%s-%s-N%d-B%d-L%#x-%s" % ("fwd" if pas == F else "bwd", kind, N, B, layout, structure)


def row_seed(row):
    pas, kind, N, B, layout = row[:5]
    return SEED.get(row_id(row), 31000 + 1000 * KIND[kind] + 100 * pas + N + (layout >> 8) * 7 + (layout & 0xff) * 3)


def base_size(N):
    return 61 if N <= 32 else 37


def persistent_launch(row):
    """(launch, listed): the launch of the row that the row is about -- the drain when the route has one."""
    ls = launches(row[6])
    return ls[-1], len(ls) > 1


def per_trip(launch, kind, N, listed):
    """Problems one launch of a persistent general kernel holds at a time: workgroups of its fixed grid x problems each."""
    g = launch_g(launch, kind, N)[0]
    if launch in ("fany", "bany"):
        return 512                                               # any_grid: min(B, 512) workgroups (N in the thousands: fewer)
    if launch == "flds":                                         # g = waves per workgroup
        return (512 if listed else 256 * 16 // g * (2 if g > 1 else 1)) * g
    if launch == "bteam":
        return (512 if listed else 256 * 8) * g
    if launch == "bsmall":
        return (512 if listed else 256 * 16) * g
    raise KeyError(launch)


def listed_mask(row, n):
    """Which problems of a batch of n problems (the base tiled to n) the row's first launch leaves on the work-list: those of
    every wave tile (a quarter of the workgroup's problems) that holds a non-diagonal P.  Problem b is base problem b mod
    base, dense when that is 1 mod 3."""
    pas, kind, N = row[:3]
    T = launch_g(launches(row[6])[0], kind, N)[0] // 4
    nb = base_size(N)
    out = []
    for f in range(0, n, T):
        tile_ = range(f, min(f + T, n))
        out += [any((b % nb) % 3 == 1 for b in tile_)] * len(tile_)
    return out


def list_len(row):
    """Entries on the work-list of the row's batch: one per problem of every queued tile."""
    return sum(listed_mask(row, row[3]))


def one_trip_size(row):
    """The batch of the one-trip call that (2)-(4) of tests/test_gpu_trips.py compare with: the base -- behind a work-list the
    base tiled a few problems further when that puts the base's last, partial tile on the list too, so that a diagonal
    problem of the base is solved by the drain in both calls (the fast kernel's bits are not the general kernel's in the
    forward).  Where no such size exists (tiles of two problems, N = 64) it is the base."""
    nb = base_size(row[2])
    if not persistent_launch(row)[1]:
        return nb
    for n in range(nb, nb + 8):
        if all(listed_mask(row, n)[:nb]):
            return n
    return nb


def covered(row):
    """n of the rule on B: what the persistent launch walks."""
    return list_len(row) if persistent_launch(row)[1] else row[3]


def make_base(row, make_problem):
    """The base batch as a dict of CPU tensors: make_problem's mixed data with problems 0 and 3 shaped (module docstring)."""
    import torch
    pas, kind, N = row[:3]
    d = make_problem(kind, base_size(N), N, row_seed(row), row[5])
    d["q"][0] = 0.0
    if kind == "qp":
        d["q"][3] = -d["q"][3].abs()
    elif kind == "box":
        d["q"][3] = d["q"][3] / 50
    elif kind == "sbox":
        d["q"][3] = torch.sign(d["v"][3]) * d["q"][3].abs() / 50
    else:
        d["q"][3] = d["q"][3] / 1000
        d["l_n"][3] = 1.0
        d["mu"][3] = 1.0
    return d


def tiled(base, B):
    """The base repeated to B problems (tensors on any device)."""
    reps = -(-B // base["q"].shape[0])
    return {k: v.repeat((reps,) + (1,) * (v.dim() - 1))[:B].contiguous() for k, v in base.items()}


def _ofwd(O, kind, a, adaptive=True):
    kw = dict(nthreads=8, adaptive=adaptive)
    if kind == "qp":
        return O.qp_fwd_batch(a["P"], a["q"], 1e-7, 1000, **kw)
    if kind == "qcqp":
        return O.qcqp_fwd_batch(a["P"], a["q"], a["l_n"], a["mu"], 1e-7, 1000, **kw)
    return O.boxqp_fwd_batch(a["P"], a["q"], a["l_min"], a["l_max"], 1e-7, 1000, v=a.get("v"), **kw)


def effective(a):
    """(lo', hi', keep_lo, keep_hi) of a signed box batch, numpy (include/diffqcqp_hip.h: dqq_signedboxqp_bwd_f64)."""
    import torch
    from sbox_cases import effective_bounds
    return tuple(t.numpy() for t in effective_bounds(*(torch.from_numpy(a[k]) for k in ("l_min", "l_max", "v"))))


def _obwd(O, kind, a, x):
    """-> ([grad_P, grad_q, third, fourth], steps, (gamma, dgamma) or None) of the oracle on x, the duals in the C ABI's layout."""
    if kind == "qp":
        gP, gq, st = O.qp_bwd_batch(a["P"], a["q"], x, a["grad_x"], nthreads=8)
        return [gP, gq], st, None
    if kind == "qcqp":
        gP, gq, gl, gm, st, gam, dgam = O.qcqp_bwd_batch(a["P"], a["q"], a["l_n"], a["mu"], x, a["grad_x"], nthreads=8, duals=True)
        return [gP, gq, gl, gm], st, (gam, dgam)
    lo, hi, klo, khi = (a["l_min"], a["l_max"], True, True) if kind == "box" else effective(a)
    gP, gq, glo, ghi, gam, st, dgam = O.boxqp_bwd_batch(a["P"], a["q"], lo, hi, x, a["grad_x"], nthreads=8, duals=True)
    return [gP, gq, np.where(klo, glo, 0.0), np.where(khi, ghi, 0.0)], st, (gam, dgam)


@functools.lru_cache(maxsize=None)
def reference(row):
    """The oracle on the row's base, solved once per session: dict with base (CPU tensors), x, iters, x and iters without the
    rho adaptation, and for a backward row grads, steps, duals on the oracle's x."""
    from conftest import make_problem
    from oracle import oracle as O
    O.build()
    O.lib()
    pas, kind = row[:2]
    base = make_base(row, make_problem)
    a = {k: v.numpy() for k, v in base.items()}
    x, it = _ofwd(O, kind, a)
    xf, itf = _ofwd(O, kind, a, adaptive=False)
    out = {"base": base, "x": x, "iters": it, "x_fixed_rho": xf, "iters_fixed_rho": itf}
    if pas == Bw:
        out["grads"], out["steps"], out["duals"] = _obwd(O, kind, a, x)
    return out


def active_sizes(row, ref):
    """Per problem of the base, from the oracle's x at the backward's thresholds (csrc/common.h: 1e-10): entries of the QP's
    active set, of the box QP's not_null list (lower and upper), active contacts of the QCQP."""
    kind = row[1]
    a = {k: v.numpy() for k, v in ref["base"].items()}
    x = ref["x"][:, :, 0]
    if kind == "qp":
        gam = -(np.einsum("bij,bj->bi", a["P"], x) + a["q"][:, :, 0])
        gam[x > 1e-10] = 0.0
        return (gam < -1e-10).sum(1)
    if kind == "qcqp":
        r = (a["l_n"] * a["mu"])[:, :, 0]
        S = x[:, 0::2] ** 2 + x[:, 1::2] ** 2 - r * r
        return ((S > -1e-10) & (r > 1e-10)).sum(1)
    lo, hi = (a["l_min"], a["l_max"]) if kind == "box" else effective(a)[:2]
    return (~(x - lo[:, :, 0] > 1e-10)).sum(1) + (~(x - hi[:, :, 0] < -1e-10)).sum(1)


def check_heterogeneous(row):
    pas, kind, N = row[:3]
    ref = reference(row)
    it = ref["iters"].astype(np.int64)
    assert (it < 1000).all() and np.isfinite(ref["x"]).all(), row_id(row)
    assert it.max() >= 2 * it.min(), (row_id(row), it.min(), it.max())
    moved = (ref["x"] != ref["x_fixed_rho"]).any(axis=(1, 2)) | (it != ref["iters_fixed_rho"])
    assert moved.any() and not moved.all(), (row_id(row), int(moved.sum()))
    if pas == Bw:
        na = active_sizes(row, ref)
        if kind == "qcqp":
            assert (na == 0).any() and (na > 0).any(), (row_id(row), na)
        else:   # (signed box: the interior problem 3 has none active, q = 0 sits on every sign bound)
            assert (na == 0).any() and (na >= (N + 1) // 2).any(), (row_id(row), na)
    return ref
