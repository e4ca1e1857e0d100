"""The cases of tests/test_gpu_footprint.py, as data, and the tile sizes they are built around.

A case is (pass, kind, N, B, p_layout, structure, route): one call of the C ABI whose every device buffer the GPU test carves
out of one guarded arena (tests/footprint_arena.py).  GROUPS is the table; each group is
    (pass, kinds, N, Bs, p_layout, structure, route, g, where g is set, drain g, where that is set, "B < g")
g: the problems one workgroup of the route's FIRST launch covers, read from the launcher named beside it (files of
diffqcqp_amd/csrc); drain g: the same for the launch that drains the work-list, when the route has one -- a drain covers
the list, not B: the CPU test counts the tile edges of a drain by the length of the list the batch produces (empty at B = 1,
where the only problem of a 'mixed' batch is diagonal, and for the 'diag' batches).  launch_g() below is
the same geometry as a function of (launch, kind, N) -- tests/test_footprint_cases.py holds the table against it, every case
against route.cpp, and checks what the cases cover.

The groups follow param_cases.FWD / BWD, one per row (rows that differ in the kind only share a group):
  * a route that a batch of one problem already takes: B in {1, g - 1, g + 1, 2 g + 1} -- below one tile, one short of a
    tile, one past it, one past two;
  * a route that exists from a batch size upward ("none: ..." in the last column: no B < g takes it, which the CPU test
    proves by scanning the plans): the row's own B and the next B that is no multiple of g (bdiag + blane/m1: B + 2,
    because problem 24576 is diagonal and alone in its tile, so that at B + 1 the drain's list is still 24576 long);
  * N >= 32 through DQQ_P_AUTO on mixed batches (the segmented work-list, csrc/worklist.h): also B = 31 g + g / 2 + 1, at which
    the workgroup that pushes to the last of the 32 segments is a partial one; B = g + 1 is the B < 32 case;
  * kernels of one problem per workgroup (g = 1) have no partial tile: B in {1, 2, 3}.
EXTRA_GROUPS: what no row of param_cases reaches at a small batch -- fdiag/1 and fdiag/2 below one tile (N = 2 and 4), the
group solve of a batch declared dense (N = 8, DQQ_P_DENSE), and the fast kernels' own stores at N >= 16, where every tile of
a 'mixed' batch holds a non-diagonal problem and goes to the drain ('diag' batches through DQQ_P_AUTO).
B = 0: one case per (pass, kind)."""
from param_cases import AUTO, DENSE, DIAG, KIND, REF, XD, XL, F, Bw, row_seed  # noqa: F401

GROUPS = [
    (F, ('qp', 'qcqp', 'box', 'sbox'), 8, (1, 63, 65, 129), 0x0, 'mixed', 'fdiag/4/fuse ws keep', 64, 'fwd_diag.hip:298-300,350', None, None, 'yes'),
    (F, ('qp', 'qcqp', 'box', 'sbox'), 8, (57344, 57345), 0x0, 'mixed', 'fdiag/2/fuse ws keep', 128, 'fwd_diag.hip:298-300,350', None, None, 'none: the route starts at B = 57344'),
    (F, ('qp', 'qcqp', 'box', 'sbox'), 4, (131073, 131074), 0x0, 'mixed', 'fdiag/1 + flane ws keep', 256, 'fwd_diag.hip:298-300,350', 64, 'fwd_lane_dense.hip:442', 'none: the route starts at B = 131073'),
    (F, ('qp', 'qcqp'), 8, (57344, 57345), 0x200, 'mixed', 'fdiag/1/fuse ws keep #feedback', 256, 'fwd_diag.hip:298-300,350', None, None, 'none: the route starts at B = 57344'),
    (F, ('qp', 'qcqp', 'box', 'sbox'), 8, (1, 63, 65, 129), 0x2, 'diag', 'fdiag/4', 64, 'fwd_diag.hip:298-300,350', None, None, 'yes'),
    (F, ('qp', 'qcqp', 'box', 'sbox'), 16, (1, 31, 33, 65), 0x0, 'mixed', 'fdiag/8 + fsmall ws keep', 32, 'fwd_diag.hip:298-300,350', 16, 'fwd_small.hip:26,259-262', 'yes'),
    (F, ('qp', 'qcqp', 'box', 'sbox'), 32, (1, 15, 17, 33, 505), 0x0, 'mixed', 'fdiag/16 + fwave64 ws keep', 16, 'fwd_diag.hip:298-300,350', 1, 'dense_wave64.hip:276', 'yes'),
    (F, ('qp', 'qcqp', 'box', 'sbox'), 64, (1, 7, 9, 17, 253), 0x0, 'mixed', 'fdiag/32 + fwave64 ws keep', 8, 'fwd_diag.hip:298-300,350', 1, 'dense_wave64.hip:276', 'yes'),
    (F, ('qp', 'qcqp', 'box', 'sbox'), 32, (1, 15, 17, 33, 505), 0x100, 'mixed', 'fdiag/16 + flds ws keep', 16, 'fwd_diag.hip:298-300,350', 3, 'dense.hip:74-83, dense_core.h:101', 'yes'),
    (F, ('qp', 'qcqp'), 8, (32769, 32770), 0x1, 'dense', 'flane', 64, 'fwd_lane_dense.hip:442', None, None, 'none: the route starts at B = 32769'),
    (F, ('box', 'sbox'), 8, (1, 63, 65, 129), 0x1, 'dense', 'flane', 64, 'fwd_lane_dense.hip:442', None, None, 'yes'),
    (F, ('qp', 'qcqp', 'box', 'sbox'), 6, (1, 63, 65, 129), 0x0, 'dense', 'flane', 64, 'fwd_lane_dense.hip:442', None, None, 'yes'),
    (F, ('qp', 'qcqp', 'box', 'sbox'), 12, (1, 15, 17, 33), 0x0, 'dense', 'fsmall', 16, 'fwd_small.hip:26,259-262', None, None, 'yes'),
    (F, ('qp', 'qcqp', 'box', 'sbox'), 24, (1, 2, 3), 0x0, 'dense', 'fwave64', 1, 'dense_wave64.hip:276', None, None, 'yes'),
    (F, ('qp', 'box', 'sbox'), 5, (1, 3, 5, 9), 0x0, 'dense', 'flds', 4, 'dense.hip:74-83, dense_core.h:101', None, None, 'yes'),
    (F, ('qp', 'qcqp', 'box', 'sbox'), 18, (1, 3, 5, 9), 0x100, 'dense', 'flds', 4, 'dense.hip:74-83, dense_core.h:101', None, None, 'yes'),
    (F, ('qp', 'qcqp', 'box', 'sbox'), 70, (1, 2, 3), 0x0, 'dense', 'fany scr', 1, 'general_any.hip:31,73', None, None, 'yes'),
    (Bw, ('qp',), 8, (1, 63, 65, 129), 0x0, 'mixed', 'bdiag + bsmall ws', 64, 'bwd_diag.hip:347-349,388', 32, 'bwd_small.hip:52-55, small_bwd_core.h:37-52', 'yes'),
    (Bw, ('qcqp',), 8, (1, 63, 65, 129), 0x0, 'mixed', 'bdiag + bsmall ws', 64, 'bwd_diag.hip:347-349,388', 20, 'bwd_small.hip:52-55, small_bwd_core.h:37-52', 'yes'),
    (Bw, ('box',), 8, (1, 63, 65, 129), 0x0, 'mixed', 'bdiag + bteam ws', 64, 'bwd_diag.hip:347-349,388', 4, 'dense.hip:114-120,135-141, dense_core.h:102-107', 'yes'),
    (Bw, ('qp', 'qcqp', 'box'), 8, (1, 63, 65, 129), 0x2, 'diag', 'bdiag', 64, 'bwd_diag.hip:347-349,388', None, None, 'yes'),
    (Bw, ('qp', 'qcqp'), 8, (24576, 24577), 0x1, 'dense', 'blane/m0', 64, 'bwd_lane_dense.hip:740', None, None, 'none: the route starts at B = 24576'),
    (Bw, ('qp', 'qcqp'), 8, (24576, 24578), 0x400, 'mixed', 'bdiag + blane/m1 ws #drains', 64, 'bwd_diag.hip:347-349,388', 64, 'bwd_lane_dense.hip:740', 'none: the route starts at B = 24576'),
    (Bw, ('qp', 'qcqp'), 8, (24576, 24577), 0x200, 'mixed', 'blane/m2 ws #whole', 64, 'bwd_lane_dense.hip:740', None, None, 'none: the route starts at B = 24576'),
    (Bw, ('qp',), 12, (1, 19, 21, 41), 0x1, 'dense', 'bsmall', 20, 'bwd_small.hip:52-55, small_bwd_core.h:37-52', None, None, 'yes'),
    (Bw, ('qcqp',), 12, (1, 5, 7, 13), 0x1, 'dense', 'bsmall', 6, 'bwd_small.hip:52-55, small_bwd_core.h:37-52', None, None, 'yes'),
    (Bw, ('box',), 2, (1, 255, 257, 513), 0x0, 'mixed', 'bdiag + bsmall ws', 256, 'bwd_diag.hip:347-349,388', 40, 'bwd_small.hip:52-55, small_bwd_core.h:37-52', 'yes'),
    (Bw, ('qp',), 24, (1, 2, 3), 0x1, 'dense', 'bchol', 1, 'dense_wave64.hip:422', None, None, 'yes'),
    (Bw, ('qcqp',), 24, (1, 2, 3), 0x1, 'dense', 'bqcqp', 1, 'bwd_wave_qcqp.hip:176', None, None, 'yes'),
    (Bw, ('qp',), 48, (1, 2, 3), 0x1, 'dense', 'bchol', 1, 'dense_wave64.hip:422', None, None, 'yes'),
    (Bw, ('qcqp',), 48, (1, 2, 3), 0x1, 'dense', 'bqcqpbig', 1, 'bwd_wave_qcqp_big.hip:302', None, None, 'yes'),
    (Bw, ('qp',), 5, (1, 31, 33, 65), 0x1, 'dense', 'bteam', 32, 'dense.hip:114-120,135-141, dense_core.h:102-107', None, None, 'yes'),
    (Bw, ('qcqp',), 18, (1, 3, 5), 0x101, 'dense', 'bteam', 2, 'dense.hip:114-120,135-141, dense_core.h:102-107', None, None, 'yes'),
    (Bw, ('box',), 16, (1, 31, 33, 65), 0x0, 'mixed', 'bdiag + bteam ws', 32, 'bwd_diag.hip:347-349,388', 1, 'dense.hip:114-120,135-141, dense_core.h:102-107', 'yes'),
    (Bw, ('box',), 4, (1, 127, 129, 257), 0x0, 'mixed', 'bdiag + bteam ws', 128, 'bwd_diag.hip:347-349,388', 12, 'dense.hip:114-120,135-141, dense_core.h:102-107', 'yes'),
    (Bw, ('qp', 'qcqp'), 70, (1, 2, 3), 0x1, 'dense', 'bany scr', 1, 'general_any.hip:57,73', None, None, 'yes'),
    (Bw, ('box',), 32, (1, 15, 17, 33, 505), 0x0, 'mixed', 'bdiag + bany ws scr', 16, 'bwd_diag.hip:347-349,388', 1, 'general_any.hip:57,73', 'yes'),
]

EXTRA_GROUPS = [
    (F, ('qp', 'qcqp'), 2, (1, 255, 257, 513), 0x0, 'mixed', 'fdiag/1/fuse ws keep', 256, 'fwd_diag.hip:298-300,350', None, None, 'yes'),
    (F, ('qp', 'qcqp'), 4, (1, 127, 129, 257), 0x0, 'mixed', 'fdiag/2/fuse ws keep', 128, 'fwd_diag.hip:298-300,350', None, None, 'yes'),
    (F, ('qp', 'qcqp'), 8, (1, 63, 65, 129), 0x1, 'dense', 'fdiag/4/fuse', 64, 'fwd_diag.hip:298-300,350', None, None, 'yes'),
    (F, ('qp', 'qcqp'), 16, (1, 31, 33, 65), 0x0, 'diag', 'fdiag/8 + fsmall ws keep', 32, 'fwd_diag.hip:298-300,350', 16, 'fwd_small.hip:26,259-262', 'yes'),
    (F, ('qp', 'qcqp'), 32, (1, 15, 17, 33), 0x0, 'diag', 'fdiag/16 + fwave64 ws keep', 16, 'fwd_diag.hip:298-300,350', 1, 'dense_wave64.hip:276', 'yes'),
    (F, ('qp', 'qcqp'), 64, (1, 7, 9, 17), 0x0, 'diag', 'fdiag/32 + fwave64 ws keep', 8, 'fwd_diag.hip:298-300,350', 1, 'dense_wave64.hip:276', 'yes'),
    (Bw, ('qcqp',), 32, (1, 15, 17, 33), 0x0, 'diag', 'bdiag + bqcqp ws', 16, 'bwd_diag.hip:347-349,388', 1, 'bwd_wave_qcqp.hip:176', 'yes'),
    (Bw, ('qp',), 64, (1, 7, 9, 17), 0x0, 'diag', 'bdiag + bchol ws', 8, 'bwd_diag.hip:347-349,388', 1, 'dense_wave64.hip:422', 'yes'),
    (Bw, ('box',), 4, (1, 127, 129, 257), 0x0, 'diag', 'bdiag + bteam ws', 128, 'bwd_diag.hip:347-349,388', 12, 'dense.hip:114-120,135-141, dense_core.h:102-107', 'yes'),
]

# families no B < g reaches: the lane-per-problem backward runs from 16384 problems on (24576 at N = 8: route.cpp
# bwd_lane_fills_chip), a tile is 64.  (Families of g = 1 have no B < g at all.)
NO_B_BELOW_G = ("blane/m0", "blane/m1", "blane/m2")

ZERO = [(F, k, 8, 0, AUTO, "mixed", "- keep") for k in ("qp", "qcqp", "box", "sbox")] + \
       [(Bw, k, 8, 0, AUTO, "mixed", "-") for k in ("qp", "qcqp", "box")]


def launch_g(launch, kind, N):
    """Problems per workgroup of one launch ('fdiag/4/fuse', 'bsmall', ...) of a (kind, N) call, and where the source says so."""
    fam = launch.split("/")[0]
    k = KIND[kind]
    if fam == "fdiag":      # 64 / lpp problems per wave, four waves per workgroup
        return 4 * 64 // int(launch.split("/")[1]), "fwd_diag.hip:298-300,350"
    if fam == "flane":
        return 64, "fwd_lane_dense.hip:442"
    if fam == "fsmall":     # teams of 16 lanes, four waves
        return 16, "fwd_small.hip:26,259-262"
    if fam == "fwave64":
        return 1, "dense_wave64.hip:276"
    if fam == "flds":       # a wave per problem, as many waves (<= 4) as 64 KiB of LDS hold
        per = (2 * N * (N | 1) + 2 * N + 2 + 1) & ~1
        return max(1, min(4, 65536 // (8 * per))), "dense.hip:74-83, dense_core.h:101"
    if fam == "fany":
        return 1, "general_any.hip:31,73"
    if fam == "bdiag":      # 128 / N problems per wave, four waves
        return 4 * 128 // N, "bwd_diag.hip:347-349,388"
    if fam == "blane":
        return 64, "bwd_lane_dense.hip:740"
    if fam == "bsmall":     # teams of M lanes (M unknowns; 4 for M = 3), four waves or two
        M = N if k == 0 else (N + N // 2 if k == 1 else 3 * N)
        T = 4 if M == 3 else M
        lds = 2 * M * ((M + 1) & ~1) + 8 * M
        wpb = 4 if lds * (64 // T) * 8 * 4 <= 65536 else 2
        return wpb * (64 // T), "bwd_small.hip:52-55, small_bwd_core.h:37-52"
    if fam == "bchol":
        return 1, "dense_wave64.hip:422"
    if fam == "bqcqp":
        return 1, "bwd_wave_qcqp.hip:176"
    if fam == "bqcqpbig":
        return 1, "bwd_wave_qcqp_big.hip:302"
    if fam == "bteam":      # teams of 8 / 16 / 32 / 64 lanes, as many waves (<= 4) as 64 KiB of LDS hold
        rows = N if k == 0 else (3 * N if k == 2 else N + N // 2)
        T = 8 if rows <= 8 else 16 if rows <= 16 else 32 if rows <= 32 else 64
        lds = (3 * rows * (rows | 1) + 5 * N + 4 * rows + 2 + (rows + 3) // 2 + 1 + 1) & ~1
        return max(1, min(4, 65536 // (8 * lds * (64 // T)))) * (64 // T), "dense.hip:114-120,135-141, dense_core.h:102-107"
    if fam == "bany":
        return 1, "general_any.hip:57,73"
    raise KeyError(launch)


def launches(route):
    """'bdiag + bsmall ws' -> ['bdiag', 'bsmall']."""
    parts = route.split(" + ")
    return [parts[0].split(" ")[0]] + [p.split(" ")[0] for p in parts[1:]]


def _expand(groups):
    out = []
    for pas, kinds, N, Bs, layout, structure, route, g, _, gd, _, _ in groups:
        for kind in kinds:
            for B in Bs:
                out.append((pas, kind, N, B, layout, structure, route))
    return out


CASES = _expand(GROUPS) + _expand(EXTRA_GROUPS) + ZERO
assert len(set(c[:6] for c in CASES)) == len(CASES)
_GROUP_OF = {(g[0], k, g[2], B, g[4], g[5]): g for g in GROUPS + EXTRA_GROUPS for k in g[1] for B in g[3]}


def case_g(case):
    """(g of the first launch, g of the drain or None) of a case; (1, None) for B = 0."""
    g = _GROUP_OF.get(case[:6])
    return (1, None) if g is None else (g[7], g[9])


def case_id(case):
    pas, kind, N, B, layout, structure, _ = case
    return "%s-%s-N%d-B%d-L%#x-%s" % ("fwd" if pas == F else "bwd", kind, N, B, layout, structure)


def case_seed(case):
    """The seed of the param_cases row of the same (pass, kind, N, p_layout, structure)."""
    return row_seed(case[:3] + (1,) + case[4:])
