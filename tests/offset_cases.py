"""The cases of tests/test_gpu_offsets.py, as data: one row per launch family and mode, at a batch whose largest buffer -- P,
and grad_P on the backward rows -- is longer than 2^32 bytes, 2^31 elements or 2^32 elements, so that the kernel under test
forms addresses there.  tests/test_offset_cases.py holds the table to account on the CPU.

A row is (pass, kind, N, B, p_layout | flags, structure, expected route, mark, the test whose bar replica 0 is held to).  The
route is written as tests/test_routes.py renders a plan; a check row's is 'check/<lanes per problem>' (plan_check); a warm row's
is the cold plan (tests/test_warm_routes.py: plan_fwd_warm is plan_fwd).  pass: F, Bw as everywhere, W = dqq_fwd_warm_f64,
C = dqq_check_f64, J = dqq_jvp_f64, Pl = dqq_polish_f64.  A J or Pl row's route is its plan's family (plan_jvp / plan_polish),
' scr' when it runs on scratch; replica 0 is held bit-equal to the family's host core, step counts and status words included.

Marks, counted in doubles of P (B N N; dP of a JVP row is the same size):
    M32  more than 2^29 doubles = 2^32 bytes      E31  more than 2^31 doubles (16 GiB)      E32  more than 2^32 doubles (32 GiB)
and for the rows that pass P as the compact diagonal (B,N) -- DQQ_P_DIAG, the only layout of JvpDiag and PolishDiag and a public
one of the cold forward and backward --
    V32  the longest per-problem VECTOR buffer -- (B,N): P, q, x, dx / x_out, grad_q, the box kinds' bounds, their tangents and
         gradients, the compact dP / grad_P -- holds more than 2^29 doubles = 2^32 bytes: B = ceil(2^29 / N) + 2 nb + 1.
         (An int ELEMENT index does not wrap there, a 32-bit BYTE offset does.  Compact buffers of 2^31 elements are out of
         scope: at N = 64 eleven such buffers of the JVP row, with the test's index and key tensors, are about 100 GiB a call.)
The rule for B: B = ceil(mark / N^2) + 2 nb + 1, nb = trip_cases.base_size(N) (61 or 37, both prime): at least two whole
replicas of the base lie entirely above the mark and the batch ends ragged.  Inputs: make_problem's data on a base of nb
problems, tiled on the device (problem b is base problem b mod nb; 'mixed': P dense when (b mod nb) mod 3 == 1, so that the
entries a fast kernel queues reach indices above the mark).

Families and modes (footprint_cases.launches names them; `direct`: the first launch walks the batch, `listed`: the launch
drains a work-list): fdiag, bdiag, the fused group solve (GROUP: fdiag/.../fuse on a 'mixed' batch, group_dense.h), flane,
blane, fsmall, bsmall, flds, bteam, fwave64, bchol, bqcqp, bqcqpbig, fany, bany, check.  fdiag, bdiag, the group solve, fany
and check have no listed mode (fany: no N > 64 has a diagonal fast path in front of it, route.cpp diag_n); blane's listed
mode is m1, its whole-batch mode m2 is counted as direct.  STREAMING, the families that must also reach E31: fdiag, bdiag,
flane, blane, fwave64, bchol, bqcqp (N = 32), bqcqpbig, check -- in one mode at least.  fdiag and fwave64 at N = 64 have a forward row at E32.

Left at M32, with what the call under test took there on an MI355X: fany 0.24 s and bany 0.08 s directly, bany as a drain
0.51 s (general_any.hip:70-76: 512 workgroups, a problem each at a time); flds 0.11 s directly and 0.20 s as a drain, bteam
0.25 s directly and 0.27 s as a drain (dense.hip:76-78, 111-114: 2048 / 512 workgroups); bsmall, fsmall directly, blane/m2,
the hint's one-lane group solve and the warm lane kernel (milliseconds; their E31 rows would only repeat the family's other
mode).  bqcqp DIRECTLY is at M32 because its E31 row (B = 2 097 275, N = 32) took 5.9 s for the one call, measured once -- 2.8 us per problem,
where the same kernel takes 8 ms for 524 411 problems directly, drains 2 097 275 queued ones in 32 ms, and bqcqpbig takes 0.05 s for 524 363 problems of N = 64 directly;
the launcher (bwd_wave_qcqp.hip:175-176) gives it a grid of B one-wave workgroups up to 2^22.  The values were right at every
index; the time is a finding about that launch, not about its addressing.  bqcqp's E31 row is the one behind the segmented list.

Out of scope, as the issue states: vectors of B N >= 2^31 elements (q, x: at N = 64 that is B = 33.5 M and a 1 TB P) and
B >= 2^31 (the plan rejects it, tests/test_routes.py).

TIMES -- the call under test on an MI355X, seconds, rows in the table's order (tiling the inputs takes 0.01-0.6 s, once 5 s for
the first 33 GiB allocation; the comparisons 0.00-0.08 s; the whole file 17.5 s, peak device memory 46.8 GiB):
    forward   0.040 0.054 0.104 0.008 0.202 | 0.032 0.009 | 0.071 0.028 0.020 0.106 0.237        warm  0.008 0.004
    backward  0.013 0.010 0.032 0.515 0.026 0.016 0.268 | 0.008 0.029 0.006 0.248 0.013 0.008 0.051 0.076   check 0.006 0.007
    jvp       0.635 0.060 0.372    polish  0.193 0.056 0.327    compact (V32)  jvp 0.025  polish 0.021  forward 0.020  backward 0.027
The ten rows of the last line (the six one-launch families of dqq_jvp_f64 and dqq_polish_f64, and DQQ_P_DIAG) add 5 s to the
file; its peak device memory with them is 56.9 GiB (the compact backward row: 58.7 GiB asked for, well under half the card).  No
row took more than about 1 s, none was moved down a mark: JvpTeam and PolishTeam stream N = 8 at E31 in 0.06 s (33.5 M problems),
and the slowest, JvpTeam at the QCQP's limit N = 42 (a wave per problem, 304 424 problems, 0.64 s), is at M32 as the issue set it.
"""
from footprint_cases import launches
from param_cases import AUTO, DENSE, KIND, REF, XD, XL, F, Bw
from trip_cases import base_size

W, C, J, Pl = 2, 3, 4, 5                        # pass: warm forward, solution check, dqq_jvp_f64, dqq_polish_f64
M32, E31, E32 = 1 << 29, 1 << 31, 1 << 32    # marks, in doubles
V32 = M32                                    # ... of the longest per-problem VECTOR buffer of a compact-layout row
MARK_NAME = {M32: "M32", E31: "E31", E32: "E32"}
DIAG = 2                                     # DQQ_P_DIAG: P, dP and grad_P are (B,N)

T_FWD = "test_gpu_parameters.py::test_forward_parameters"      # check_forward: X_TOL, equal counts on _min_match(N, route)
T_BWD = "test_gpu_footprint.py::test_footprint"                 # _check_rows, min_same = 0 (batches of 1 to 130 problems)
T_WARM = "test_gpu_warm.py::test_warm_forward_against_the_restatement"
T_CHECK = "test_gpu_check.py::test_device_equals_host_core"
T_JVP = "test_gpu_jvp.py::test_*_is_the_host_core"             # bit-equal to the host core, step counts included
T_POLISH = "test_gpu_polish.py::test_*_is_the_host_core"       # bit-equal to the host core: x_out, resid, steps, status


def compact(row):
    """The row passes P (and dP, grad_P) as the compact diagonal (B,N): its mark counts a (B,N) buffer's doubles."""
    return (row[4] & 0xff) == DIAG


def per_problem(N, layout):
    """Doubles per problem of the buffer a row's mark is counted in."""
    return N if (layout & 0xff) == DIAG else N * N


def batch(N, mark, layout=0):
    return -(-mark // per_problem(N, layout)) + 2 * base_size(N) + 1


def mark_name(row):
    return "V32" if compact(row) else MARK_NAME[row[7]]


def _r(pas, kind, N, mark, layout, structure, route, test):
    return (pas, kind, N, batch(N, mark, layout), layout, structure, route, mark, test)


ROWS = (
    # ---- forward: the diagonal kernel in front of a drain (segmented list, N >= 32; plain list, N <= 16), and alone
    _r(F, "qp", 64, E32, AUTO, "mixed", "fdiag/32 + fwave64 ws keep", T_FWD),
    _r(F, "qcqp", 32, E31, AUTO, "mixed", "fdiag/16 + fwave64 ws keep", T_FWD),
    _r(F, "box", 16, E31, AUTO, "mixed", "fdiag/4 + fsmall ws keep", T_FWD),
    _r(F, "sbox", 4, M32, AUTO, "mixed", "fdiag/1 + flane ws keep", T_FWD),
    _r(F, "qcqp", 32, M32, AUTO | REF, "mixed", "fdiag/16 + flds ws keep", T_FWD),
    # the fused group solve (group_dense.h): two lanes per problem, and the hint's one lane with the tile staged in LDS
    _r(F, "qp", 8, E31, AUTO, "mixed", "fdiag/2/fuse ws keep", T_FWD),
    _r(F, "qcqp", 8, M32, AUTO | XD, "mixed", "fdiag/1/fuse ws keep #feedback", T_FWD),
    # ---- forward, direct
    _r(F, "qcqp", 64, E32, DENSE, "dense", "fwave64", T_FWD),
    _r(F, "qcqp", 8, E31, DENSE, "dense", "flane", T_FWD),
    _r(F, "sbox", 12, M32, DENSE, "dense", "fsmall", T_FWD),
    _r(F, "box", 18, M32, DENSE | REF, "dense", "flds", T_FWD),
    _r(F, "qp", 70, M32, DENSE, "dense", "fany scr", T_FWD),
    # ---- warm forward: the diagonal route at E31, a dense route at M32
    _r(W, "qp", 8, E31, AUTO, "diag", "fdiag/2/fuse ws keep", T_WARM),
    _r(W, "box", 8, M32, DENSE, "dense", "flane", T_WARM),
    # ---- backward: the diagonal kernel in front of a drain
    _r(Bw, "qp", 64, E31, AUTO, "mixed", "bdiag + bchol ws", T_BWD),
    _r(Bw, "qcqp", 64, M32, AUTO, "mixed", "bdiag + bqcqpbig ws", T_BWD),
    _r(Bw, "qcqp", 32, E31, AUTO, "mixed", "bdiag + bqcqp ws", T_BWD),
    _r(Bw, "box", 32, M32, AUTO, "mixed", "bdiag + bany ws scr", T_BWD),
    _r(Bw, "qp", 8, E31, AUTO | XL, "mixed", "bdiag + blane/m1 ws #drains", T_BWD),
    _r(Bw, "qcqp", 8, M32, AUTO, "mixed", "bdiag + bsmall ws", T_BWD),
    _r(Bw, "sbox", 8, M32, AUTO, "mixed", "bdiag + bteam ws", T_BWD),
    # ---- backward, direct
    _r(Bw, "qcqp", 8, M32, AUTO | XD, "mixed", "blane/m2 ws #whole", T_BWD),
    _r(Bw, "qcqp", 8, E31, DENSE, "dense", "blane/m0", T_BWD),
    _r(Bw, "qp", 12, M32, DENSE, "dense", "bsmall", T_BWD),
    _r(Bw, "box", 8, M32, DENSE, "dense", "bteam", T_BWD),
    _r(Bw, "qp", 64, E31, DENSE, "dense", "bchol", T_BWD),
    _r(Bw, "qcqp", 32, M32, DENSE, "dense", "bqcqp", T_BWD),
    _r(Bw, "qcqp", 64, E31, DENSE, "dense", "bqcqpbig", T_BWD),
    _r(Bw, "qp", 70, M32, DENSE, "dense", "bany scr", T_BWD),
    # ---- the solution check
    _r(C, "sbox", 64, E31, AUTO, "mixed", "check/32", T_CHECK),
    _r(C, "qcqp", 8, M32, AUTO, "mixed", "check/4", T_CHECK),
    # ---- the forward-mode derivative: JvpTeam at its QCQP limit and as one small team per problem, JvpAny on the scratch
    _r(J, "qcqp", 42, M32, DENSE, "dense", "JvpTeam", T_JVP),
    _r(J, "qp", 8, E31, DENSE, "dense", "JvpTeam", T_JVP),
    _r(J, "box", 22, M32, DENSE, "dense", "JvpAny scr", T_JVP),
    # ---- the polish: PolishTeam a wave per problem and 8 lanes per problem, PolishAny on dqq_polish_scratch_bytes
    _r(Pl, "qcqp", 64, M32, DENSE, "dense", "PolishTeam", T_POLISH),
    _r(Pl, "box", 8, E31, AUTO, "dense", "PolishTeam", T_POLISH),
    _r(Pl, "qp", 66, M32, DENSE, "dense", "PolishAny scr", T_POLISH),
    # ---- DQQ_P_DIAG, every (B,N) buffer of the call past 2^32 bytes: the two compact-only families, the cold forward and backward
    _r(J, "sbox", 64, V32, DIAG, "diag", "JvpDiag", T_JVP),
    _r(Pl, "qcqp", 64, V32, DIAG, "diag", "PolishDiag", T_POLISH),
    _r(F, "qp", 64, V32, DIAG, "diag", "fdiag/32", T_FWD),
    _r(Bw, "box", 64, V32, DIAG, "diag", "bdiag", T_BWD),
)

# (family, mode) pairs no call can reach, and why
NO_SUCH_MODE = {
    ("fdiag", "listed"): "always the first launch", ("bdiag", "listed"): "always the first launch",
    ("GROUP", "listed"): "solved inside the fdiag launch", ("check", "listed"): "one launch, no work-list",
    ("fany", "listed"): "no N > 64 has a diagonal fast path in front of it (route.cpp diag_n)",
}
ONE_LAUNCH = ("JvpDiag", "JvpTeam", "JvpAny", "PolishDiag", "PolishTeam", "PolishAny")
NO_SUCH_MODE.update({(f, "listed"): "one launch, no work-list" for f in ONE_LAUNCH})
FAMILIES = ("fdiag", "bdiag", "GROUP", "flane", "blane", "fsmall", "bsmall", "flds", "bteam", "fwave64", "bchol", "bqcqp",
            "bqcqpbig", "fany", "bany", "check") + ONE_LAUNCH
STREAMING = ("fdiag", "bdiag", "flane", "blane", "fwave64", "bchol", "bqcqp", "bqcqpbig", "check")


def row_id(row):
    pas, kind, N, B, layout, structure = row[:6]
    return "%s-%s-N%d-B%d-L%#x-%s-%s" % (("fwd", "bwd", "warm", "check", "jvp", "polish")[pas], kind, N, B, layout, structure,
                                         mark_name(row))


def row_seed(row):
    """As trip_cases.row_seed, on another thousand."""
    pas, kind, N, B, layout = row[:5]
    return 41000 + 1000 * KIND[kind] + 100 * pas + N + (layout >> 8) * 7 + (layout & 0xff) * 3


def modes(row):
    """The (family, mode) pairs a row covers.  A fused diagonal forward on a batch with non-diagonal problems also runs the
    group solve."""
    pas, route, structure = row[0], row[6], row[5]
    if pas == C:
        return {("check", "direct")}
    if pas in (J, Pl):
        return {(route.split(" ")[0], "direct")}
    ls = [l.split("/")[0] for l in launches(route)]
    out = {(ls[0], "direct")} | {(l, "listed") for l in ls[1:]}
    if "/fuse" in route and structure != "diag":
        out.add(("GROUP", "direct"))
    return out


def largest_doubles(row):
    """Doubles in the buffer the row's mark is counted in: P -- and grad_P / dP of the same shape on a backward / JVP row --, (B,N,N);
    on a compact-layout row (B,N), which q, x, x_out, dx, dq, grad_q and the box kinds' bounds, their gradients and tangents equal."""
    return row[3] * per_problem(row[2], row[4])


def above_mark(row):
    """Problems whose P lies wholly above the mark: those from ceil(mark / doubles per problem) on."""
    N, B, mark = row[2], row[3], row[7]
    return B - -(-mark // per_problem(N, row[4]))


# ---- the comparison the GPU test rests on (works on CPU tensors too: tests/test_offset_cases.py proves that it can fail)
def replica_keys(row, B, device="cpu"):
    """-> (key (B), ref (K), queued (B) or None).  Problem b must come back with the bits of problem ref[key[b]], the first problem
    of the batch that is the same base problem solved by the same kernel: key = b mod nb, and behind a work-list + nb when b's
    wave tile of the first launch holds a non-diagonal problem -- whole tiles are queued, and the drain's bits are not the fast
    kernel's (trip_cases.listed_mask is the same rule, tile by tile in Python).  Keys without a problem have ref = B."""
    import torch
    from footprint_cases import launch_g
    pas, kind, N, route = row[0], row[1], row[2], row[6]
    nb = base_size(N)
    b = torch.arange(B, device=device)
    key, queued, K = b % nb, None, nb
    ls = launches(route) if pas in (F, Bw) else []
    if len(ls) > 1:
        T = launch_g(ls[0], kind, N)[0] // 4
        dense = key % 3 == 1
        tiles = torch.cat([dense, dense.new_zeros((-B) % T)]).view(-1, T).any(1)
        queued = tiles.repeat_interleave(T)[:B]
        key, K = key + nb * queued, 2 * nb
    ref = torch.full((K,), B, dtype=torch.int64, device=device).scatter_reduce_(0, key, b, "amin")
    return key, ref, queued


def _bits(t):
    import torch
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def first_unequal_replica(t, key, ref, chunk_elems=1 << 25):
    """t: (B, ...) tensor.  None when every problem b is bit-equal to problem ref[key[b]]; else (b, how many problems differ)
    with b the first problem that differs.  Compared in chunks of about chunk_elems elements: no temporary approaches the size
    of t.  One synchronisation when all is equal."""
    import torch
    B = t.shape[0]
    flat = _bits(t).reshape(B, -1)
    want = flat[ref.clamp(max=B - 1)]
    rows = max(1, chunk_elems // max(1, flat.shape[1]))
    spans = [(lo, min(B, lo + rows)) for lo in range(0, B, rows)]
    flags = [(flat[lo:hi] != want[key[lo:hi]]).any() for lo, hi in spans]
    if not flags or not bool(torch.stack(flags).any()):
        return None
    first, count = None, 0
    for (lo, hi), f in zip(spans, torch.stack(flags).tolist()):
        if f:
            diff = (flat[lo:hi] != want[key[lo:hi]]).any(1)
            count += int(diff.sum())
            if first is None:
                first = lo + int(torch.nonzero(diff)[0, 0])
    return first, count


def count_equal_bits(t, lo, value_bits):
    """How many elements of t[lo:] still hold the sentinel's bit pattern."""
    return int((_bits(t[lo:]) == value_bits).sum())


# ---- the documented sizes, in Python integers (include/diffqcqp_hip.h, DESIGN.md section 2, general_any.hip)
def workspace_bytes(B):
    ints = 3104 + 32 * (max(B, 0) // 32 + 512)
    return 4 * ((ints + 63) // 64 * 64)


def scratch_bytes(kind, pas, N, B, layout):
    """kind 0..3, pas 0 / 1.  One slice per workgroup of the global-memory kernels' persistent grid -- min(B, 512), fewer when 512
    slices would pass 4 GiB --; a slice holds the vectors, K in the backward, and the two matrices of the O(n^3) loops when they
    do not fit 152 KiB of LDS."""
    ref = (layout & REF) != 0
    if B <= 0 or N < 1 or (pas == 1 and kind == 3):
        return 0
    limit = 64 if pas == 0 else {0: 64, 1: 42 if ref else 64, 2: 21}[kind]
    if N <= limit:
        return 0
    rows = N if (pas == 0 or kind == 0) else (N + N // 2 if kind == 1 else 3 * N)
    mat = rows * (rows | 1)
    in_lds = 8 * 2 * mat <= 152 * 1024
    if pas == 0:
        vec = 8 * N + 8
        stride = (vec + 1) & ~1 if in_lds else (2 * mat + vec + 1) & ~1
    else:
        vec = 16 * rows + 8 * N + 16
        stride = (mat + vec + 1) & ~1 if in_lds else (3 * mat + vec + 1) & ~1
    grid = max(1, min(512, (4 << 30) // (8 * stride)))
    return 8 * stride * min(B, grid)


def jvp_scratch_bytes(kind, N, B, layout):
    """dqq_jvp_f64's scratch behind the work-list: the backward's reference-order slice, the signed box QP sized as the box QP."""
    return 0 if (layout & 0xff) == DIAG else scratch_bytes(min(kind, 2), 1, N, B, layout | REF)


def polish_scratch_bytes(N, B, layout):
    """dqq_polish_scratch_bytes: nothing up to N = 64 or on the compact layout; beyond, a slice of the matrix N (N|1) and 7 N
    doubles of vectors (rounded up to even) per workgroup of the same persistent grid."""
    if B <= 0 or N <= 64 or (layout & 0xff) == DIAG:
        return 0
    stride = (N * (N | 1) + 7 * N + 1) & ~1
    return 8 * stride * min(B, max(1, min(512, (4 << 30) // (8 * stride))))
