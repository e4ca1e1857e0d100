"""CPU check of the route plan (diffqcqp_amd/csrc/route.cpp): which kernels a call of (kind, pass, N, B, p_layout | flags)
launches, against an explicit table -- DESIGN.md section 3, both sides of every size threshold the routes use, every kind,
layout and flag, and the developer build's non-default knob values.  route.cpp is compiled for the host behind a small
extern "C" shim (tests/hostcore/route_check.cpp), once as shipped and once with -DDQQ_TUNING.  The three queries of the C
ABI that describe routes (dqq_scratch_bytes, dqq_max_n, dqq_hint_flags) are checked against the same plans."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "diffqcqp_amd", "csrc")

AUTO, DENSE, DIAG = 0, 1, 2
REF, XD, XL = 0x100, 0x200, 0x400          # DQQ_F_REFERENCE_ORDER, DQQ_F_EXPECT_DENSE, DQQ_F_EXPECT_LONG_LIST
QP, QCQP, BOX, SBOX = 0, 1, 2, 3
KNOBS = ("fwd_lpp", "fuse_fallback", "lane_dense", "small_fwd", "small_bwd", "lane_bwd", "fwd_feedback", "bwd_skip_classify")
SHIPPED = {"fwd_lpp": 0, "fuse_fallback": -1, "lane_dense": 1, "small_fwd": 1, "small_bwd": 1, "lane_bwd": 1,
           "fwd_feedback": 1, "bwd_skip_classify": 1}
FAMILY = ["-", "fdiag", "flane", "fsmall", "fwave64", "flds", "fany",
          "bdiag", "blane", "bsmall", "bchol", "bqcqp", "bqcqpbig", "bteam", "bany"]
COUNTER = ["", "#feedback", "#whole", "#drains"]


def _build(tuning):
    src = os.path.join(HERE, "hostcore", "route_check.cpp")
    so = os.path.join(HERE, "hostcore", "libroute%s.so" % ("_tuning" if tuning else ""))
    deps = [src, os.path.join(ROOT, "include", "diffqcqp_hip.h")] + [os.path.join(CSRC, f) for f in
                                                                        ("route.cpp", "route.h", "tuning.h", "report.h",
                                                                         "worklist.h", "common.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-fvisibility=hidden"] +
                              (["-DDQQ_TUNING"] if tuning else []) + ["-o", so + ".tmp", src])
        os.replace(so + ".tmp", so)
    lib = ctypes.CDLL(so)
    lib.route_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int,
                               ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.route_hint_flags.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong]
    lib.route_workspace_bytes.argtypes = [ctypes.c_longlong]
    lib.route_workspace_bytes.restype = ctypes.c_ulonglong
    assert lib.route_tuning() == (1 if tuning else 0)
    return lib


@pytest.fixture(scope="module")
def routes():
    return {False: _build(False), True: _build(True)}


def raw_plan(lib, pas, kind, N, B, p_layout, **knobs):
    k = dict(SHIPPED, **knobs)
    kn = (ctypes.c_int * 8)(*[k[n] for n in KNOBS])
    out = (ctypes.c_int * 14)()
    lib.route_plan(pas, kind, N, B, p_layout, kn, out)
    return list(out)


def render(o):
    """'E-3' for an error, else '<first> [+ <drain>] [ws] [scr] [keep] [#counter]'; a diagonal launch shows its lanes per
    problem and /fuse, a lane-per-problem backward its mode."""
    if o[0] != 0:
        return "E%d" % o[0]

    def launch(f, lpp, fuse, mode, _):
        s = FAMILY[f]
        if f == 1:
            s += "/%d" % lpp
        if fuse:
            s += "/fuse"
        if f == 8:
            s += "/m%d" % mode
        return s

    s = launch(*o[4:9])
    if o[9] != 0:
        s += " + " + launch(*o[9:14])
    for flag, word in ((o[2], "ws"), (o[3], "scr"), (o[1], "keep")):
        if flag:
            s += " " + word
    for c in (o[8], o[13]):
        if c:
            s += " " + COUNTER[c]
    return s


# (pass, kind, N, B, p_layout, knobs, expected).  Written from the routes as DESIGN.md section 3 states them.
F, Bw = 0, 1
TABLE = [
    # ---- forward, DQQ_P_AUTO: lanes per problem of the diagonal kernel on both sides of each batch-size rule
    (F, QP, 16, 40960, AUTO, {}, "fdiag/8 + fsmall ws keep"),
    (F, QP, 16, 40961, AUTO, {}, "fdiag/4 + fsmall ws keep"),
    (F, QP, 8, 57343, AUTO, {}, "fdiag/4/fuse ws keep"),
    (F, QP, 8, 57344, AUTO, {}, "fdiag/2/fuse ws keep"),
    (F, QP, 4, 131071, AUTO, {}, "fdiag/2/fuse ws keep"),
    (F, QP, 4, 131072, AUTO, {}, "fdiag/1/fuse ws keep"),      # the fuse limit ...
    (F, QP, 4, 131073, AUTO, {}, "fdiag/1 + flane ws keep"),   # ... and one past it: drain launch behind
    (F, QP, 2, 1, AUTO, {}, "fdiag/1/fuse ws keep"),
    (F, QP, 2, 1 << 20, AUTO, {}, "fdiag/1/fuse ws keep"),
    (F, QCQP, 8, 65536, AUTO, {}, "fdiag/2/fuse ws keep"),
    (F, BOX, 8, 65536, AUTO, {}, "fdiag/2/fuse ws keep"),
    (F, SBOX, 16, 300, AUTO, {}, "fdiag/8 + fsmall ws keep"),
    (F, QP, 32, 300, AUTO, {}, "fdiag/16 + fwave64 ws keep"),
    (F, QCQP, 64, 300, AUTO, {}, "fdiag/32 + fwave64 ws keep"),
    (F, QP, 32, 300, AUTO | REF, {}, "fdiag/16 + flds ws keep"),
    (F, QP, 64, 300, AUTO | REF, {}, "fdiag/32 + flds ws keep"),
    # hint flags: N = 8 on one lane per problem where two would run (QP / QCQP only), the long-list hint is the backward's
    (F, QP, 8, 65536, AUTO | XD, {}, "fdiag/1/fuse ws keep #feedback"),
    (F, QCQP, 8, 65536, AUTO | XD, {}, "fdiag/1/fuse ws keep #feedback"),
    (F, QP, 8, 57343, AUTO | XD, {}, "fdiag/4/fuse ws keep"),
    (F, BOX, 8, 65536, AUTO | XD, {}, "fdiag/2/fuse ws keep"),
    (F, SBOX, 8, 65536, AUTO | XD, {}, "fdiag/2/fuse ws keep"),
    (F, QP, 4, 131072, AUTO | XD, {}, "fdiag/1/fuse ws keep"),
    (F, QP, 8, 65536, AUTO | XL, {}, "fdiag/2/fuse ws keep"),
    (F, QP, 8, 65536, AUTO | XD | REF, {}, "fdiag/1/fuse ws keep #feedback"),
    # sizes without a fast path: as DQQ_P_DENSE
    (F, QP, 6, 100, AUTO, {}, "flane"),
    (F, QP, 5, 100, AUTO, {}, "flds"),
    (F, QP, 10, 100, AUTO, {}, "fsmall"),
    (F, QP, 17, 100, AUTO, {}, "fwave64"),
    (F, QP, 17, 100, AUTO | REF, {}, "flds"),
    (F, QP, 65, 10, AUTO, {}, "fany scr"),
    (F, QCQP, 66, 10, AUTO, {}, "fany scr"),
    # ---- forward, DQQ_P_DENSE
    (F, QP, 8, 32768, DENSE, {}, "fdiag/4/fuse"),               # group solve of the fused kernel ...
    (F, QP, 8, 32769, DENSE, {}, "flane"),                      # ... below 32 Ki problems only
    (F, QCQP, 8, 32768, DENSE, {}, "fdiag/4/fuse"),
    (F, BOX, 8, 32768, DENSE, {}, "flane"),
    (F, QP, 8, 32768, DENSE | XD, {}, "fdiag/4/fuse"),
    (F, QP, 4, 100, DENSE, {}, "flane"),
    (F, QP, 2, 100, DENSE, {}, "flane"),
    (F, QP, 3, 100, DENSE, {}, "flds"),
    (F, QP, 15, 100, DENSE, {}, "flds"),
    (F, QP, 16, 100, DENSE, {}, "fsmall"),
    (F, SBOX, 12, 100, DENSE, {}, "fsmall"),
    (F, QP, 32, 100, DENSE, {}, "fwave64"),
    (F, QP, 32, 100, DENSE | REF, {}, "flds"),
    (F, QCQP, 64, 100, DENSE, {}, "fwave64"),
    (F, QP, 64, 100, DENSE, {}, "fwave64"),
    (F, QP, 65, 100, DENSE, {}, "fany scr"),
    (F, BOX, 65, 100, DENSE | REF, {}, "fany scr"),
    # ---- forward, DQQ_P_DIAG
    (F, QP, 8, 65536, DIAG, {}, "fdiag/2"),
    (F, QP, 8, 65536, DIAG | XD, {}, "fdiag/2"),
    (F, QP, 16, 40961, DIAG, {}, "fdiag/4"),
    (F, SBOX, 64, 100, DIAG, {}, "fdiag/32"),
    (F, QP, 6, 100, DIAG, {}, "E-3"),
    (F, QP, 65, 100, DIAG, {}, "E-3"),
    # ---- forward: B = 0 and argument errors
    (F, QP, 8, 0, AUTO, {}, "- keep"),
    (F, QP, 6, 0, DIAG, {}, "-"),
    (F, QP, 6, 0, AUTO, {}, "-"),
    (F, QCQP, 5, 100, AUTO, {}, "E-2"),
    (F, QCQP, 5, 0, DENSE, {}, "E-2"),
    (F, QCQP, 65, 100, DENSE, {}, "E-2"),
    (F, QP, 8, -1, AUTO, {}, "E-2"),
    (F, QP, 8, 1 << 31, AUTO, {}, "E-2"),
    (F, QP, 0, 10, AUTO, {}, "E-2"),
    (F, QP, 8, 10, 3, {}, "E-4"),
    (F, QP, 8, 10, 0x800, {}, "E-4"),
    # ---- forward, developer-build knobs
    (F, QP, 8, 65536, AUTO, {"fuse_fallback": 0}, "fdiag/2 + flane ws keep"),
    (F, QP, 8, 65536, AUTO, {"fuse_fallback": 0, "lane_dense": 0}, "fdiag/2 + flds ws keep"),
    (F, QP, 8, 65536, AUTO | XD, {"fuse_fallback": 0}, "fdiag/2 + flane ws keep"),
    (F, QP, 4, 131073, AUTO, {"fuse_fallback": 1}, "fdiag/1/fuse ws keep"),
    (F, QP, 16, 40960, AUTO, {"fuse_fallback": 1}, "fdiag/8/fuse ws keep"),
    (F, QP, 32, 300, AUTO, {"fuse_fallback": 1}, "fdiag/16 + fwave64 ws keep"),
    (F, QP, 16, 300, AUTO, {"small_fwd": 0}, "fdiag/8 + flds ws keep"),
    (F, QP, 8, 65536, AUTO, {"fwd_lpp": 4}, "fdiag/4/fuse ws keep"),
    (F, QP, 8, 65536, AUTO | XD, {"fwd_lpp": 2}, "fdiag/2/fuse ws keep"),
    (F, QP, 8, 65536, AUTO, {"fwd_lpp": 3}, "fdiag/2/fuse ws keep"),      # not instantiated: the built-in layout
    (F, QP, 8, 65536, AUTO | XD, {"fwd_feedback": 0}, "fdiag/2/fuse ws keep"),
    (F, QP, 8, 100, DIAG, {"fwd_lpp": 1}, "fdiag/1"),
    (F, QP, 8, 32768, DENSE, {"fwd_lpp": 2}, "fdiag/2/fuse"),
    (F, QP, 8, 32768, DENSE, {"fwd_lpp": 3}, "fdiag/4/fuse"),
    (F, QP, 8, 32768, DENSE, {"fuse_fallback": 0}, "flane"),
    (F, QP, 8, 32768, DENSE, {"lane_dense": 0}, "flds"),
    (F, QP, 8, 100, DENSE, {"lane_dense": 0, "fuse_fallback": 0}, "flds"),
    # ---- backward, DQQ_P_AUTO: diagonal kernel + drain of the work-list
    (Bw, QP, 8, 1000, AUTO, {}, "bdiag + bsmall ws"),
    (Bw, QCQP, 2, 1000, AUTO, {}, "bdiag + bsmall ws"),
    (Bw, QP, 16, 1000, AUTO, {}, "bdiag + bsmall ws"),
    (Bw, QP, 32, 300, AUTO, {}, "bdiag + bchol ws"),
    (Bw, QP, 64, 300, AUTO, {}, "bdiag + bchol ws"),
    (Bw, QP, 32, 300, AUTO | REF, {}, "bdiag + bteam ws"),
    (Bw, QCQP, 32, 300, AUTO, {}, "bdiag + bqcqp ws"),
    (Bw, QCQP, 64, 300, AUTO, {}, "bdiag + bqcqpbig ws"),
    (Bw, QCQP, 32, 300, AUTO | REF, {}, "bdiag + bteam ws"),
    (Bw, QCQP, 64, 300, AUTO | REF, {}, "bdiag + bany ws scr"),
    (Bw, BOX, 2, 300, AUTO, {}, "bdiag + bsmall ws"),
    (Bw, BOX, 4, 300, AUTO, {}, "bdiag + bteam ws"),
    (Bw, BOX, 16, 300, AUTO, {}, "bdiag + bteam ws"),
    (Bw, BOX, 32, 300, AUTO, {}, "bdiag + bany ws scr"),
    # the long-list hint: the lane kernel drains a list that fills the chip (N = 8: 24576 problems, else 16384)
    (Bw, QP, 8, 24575, AUTO | XL, {}, "bdiag + bsmall ws"),
    (Bw, QP, 8, 24576, AUTO | XL, {}, "bdiag + blane/m1 ws #drains"),
    (Bw, QCQP, 4, 16383, AUTO | XL, {}, "bdiag + bsmall ws"),
    (Bw, QCQP, 4, 16384, AUTO | XL, {}, "bdiag + blane/m1 ws #drains"),
    (Bw, QP, 16, 65536, AUTO | XL, {}, "bdiag + bsmall ws"),
    (Bw, QP, 8, 65536, AUTO, {}, "bdiag + bsmall ws"),
    # the dense hint: the lane kernel takes the whole batch, no classifying launch
    (Bw, QP, 8, 24575, AUTO | XD, {}, "bdiag + bsmall ws"),
    (Bw, QP, 8, 24576, AUTO | XD, {}, "blane/m2 ws #whole"),
    (Bw, QCQP, 8, 65536, AUTO | XD | XL, {}, "blane/m2 ws #whole"),
    (Bw, QCQP, 2, 16384, AUTO | XD, {}, "blane/m2 ws #whole"),
    (Bw, QCQP, 2, 16383, AUTO | XD | XL, {}, "bdiag + bsmall ws"),
    # the box QP backward takes no hint flags
    (Bw, BOX, 8, 65536, AUTO | XD | XL, {}, "bdiag + bteam ws"),
    (Bw, BOX, 2, 65536, AUTO | XD | XL, {}, "bdiag + bsmall ws"),
    # sizes without a fast path: as DQQ_P_DENSE
    (Bw, QP, 6, 16383, AUTO, {}, "bsmall"),
    (Bw, QP, 6, 16384, AUTO, {}, "blane/m0"),
    (Bw, QP, 6, 16384, AUTO | XD, {}, "blane/m0"),
    (Bw, QP, 5, 100, AUTO, {}, "bteam"),
    (Bw, QP, 65, 100, AUTO, {}, "bany scr"),
    # ---- backward, DQQ_P_DENSE
    (Bw, QP, 8, 24575, DENSE, {}, "bsmall"),
    (Bw, QP, 8, 24576, DENSE, {}, "blane/m0"),
    (Bw, QCQP, 4, 16383, DENSE, {}, "bsmall"),
    (Bw, QCQP, 4, 16384, DENSE, {}, "blane/m0"),
    (Bw, BOX, 8, 65536, DENSE, {}, "bteam"),
    (Bw, QP, 16, 100, DENSE, {}, "bsmall"),
    (Bw, QCQP, 16, 100, DENSE, {}, "bsmall"),
    (Bw, QP, 17, 100, DENSE, {}, "bchol"),
    (Bw, QP, 17, 100, DENSE | REF, {}, "bteam"),
    (Bw, QP, 64, 100, DENSE, {}, "bchol"),
    (Bw, QP, 65, 100, DENSE, {}, "bany scr"),
    (Bw, QCQP, 18, 100, DENSE, {}, "bqcqp"),
    (Bw, QCQP, 32, 100, DENSE, {}, "bqcqp"),
    (Bw, QCQP, 34, 100, DENSE, {}, "bqcqpbig"),
    (Bw, QCQP, 64, 100, DENSE, {}, "bqcqpbig"),
    (Bw, QCQP, 66, 100, DENSE, {}, "bany scr"),
    (Bw, QCQP, 42, 100, DENSE | REF, {}, "bteam"),
    (Bw, QCQP, 44, 100, DENSE | REF, {}, "bany scr"),
    (Bw, BOX, 21, 100, DENSE, {}, "bteam"),
    (Bw, BOX, 22, 100, DENSE, {}, "bany scr"),
    (Bw, BOX, 2, 100, DENSE, {}, "bsmall"),
    # ---- backward, DQQ_P_DIAG, B = 0, errors
    (Bw, QP, 8, 65536, DIAG, {}, "bdiag"),
    (Bw, BOX, 64, 100, DIAG, {}, "bdiag"),
    (Bw, QCQP, 64, 100, DIAG | REF, {}, "bdiag"),
    (Bw, QP, 6, 100, DIAG, {}, "E-3"),
    (Bw, QP, 8, 0, AUTO, {}, "-"),
    (Bw, QP, 6, 0, DIAG, {}, "-"),
    (Bw, QCQP, 7, 100, AUTO, {}, "E-2"),
    (Bw, QCQP, 43, 100, DENSE | REF, {}, "E-2"),
    (Bw, QP, 8, 100, 0x1000, {}, "E-4"),
    # ---- backward, developer-build knobs
    (Bw, QP, 8, 1000, AUTO, {"fuse_fallback": 1}, "bdiag/fuse ws"),
    (Bw, QCQP, 2, 1000, AUTO, {"fuse_fallback": 1}, "bdiag/fuse ws"),
    (Bw, QP, 8, 65536, AUTO | XD, {"fuse_fallback": 1}, "bdiag/fuse ws"),
    (Bw, BOX, 8, 1000, AUTO, {"fuse_fallback": 1}, "bdiag + bteam ws"),
    (Bw, QP, 16, 1000, AUTO, {"fuse_fallback": 1}, "bdiag + bsmall ws"),
    (Bw, QP, 8, 1000, AUTO, {"fuse_fallback": 0}, "bdiag + bsmall ws"),
    (Bw, QP, 8, 65536, AUTO | XD, {"bwd_skip_classify": 0}, "bdiag + bsmall ws"),
    (Bw, QP, 8, 65536, AUTO | XD | XL, {"bwd_skip_classify": 0}, "bdiag + blane/m1 ws #drains"),
    (Bw, QP, 8, 65536, AUTO | XD | XL, {"lane_bwd": 0}, "bdiag + bsmall ws"),
    (Bw, QP, 8, 65536, DENSE, {"lane_bwd": 0}, "bsmall"),
    (Bw, QP, 8, 100, DENSE, {"small_bwd": 0}, "bteam"),
    (Bw, BOX, 2, 100, AUTO, {"small_bwd": 0}, "bdiag + bteam ws"),
    (Bw, QP, 8, 100, DIAG, {"fuse_fallback": 1}, "bdiag"),
]


@pytest.mark.parametrize("row", TABLE, ids=lambda r: "%s-k%d-N%d-B%d-L%#x%s" % (
    "fwd" if r[0] == 0 else "bwd", r[1], r[2], r[3], r[4], "".join("-%s%d" % kv for kv in sorted(r[5].items()))))
def test_route_table(routes, row):
    pas, kind, N, B, p_layout, knobs, want = row
    assert render(raw_plan(routes[False], pas, kind, N, B, p_layout, **knobs)) == want
    # the developer build routes the same (its knobs at these values; its extra lane layouts are below)
    assert render(raw_plan(routes[True], pas, kind, N, B, p_layout, **knobs)) == want


def test_extra_lane_layouts_are_the_developer_builds_only(routes):
    """fwd_lpp values the shipped build does not instantiate fall back to the built-in layout."""
    for N, B, lpp, built_in in ((16, 40960, 2, 8), (32, 300, 4, 16), (32, 300, 8, 16), (64, 300, 8, 32), (64, 300, 16, 32)):
        for layout in (AUTO, DIAG):
            shipped = raw_plan(routes[False], 0, QP, N, B, layout, fwd_lpp=lpp)
            dev = raw_plan(routes[True], 0, QP, N, B, layout, fwd_lpp=lpp)
            assert shipped[5] == built_in and dev[5] == lpp, (N, lpp, layout)


def test_an_empty_batch_launches_nothing(routes):
    """B = 0 is Family::None, with no drain, work-list or scratch: for every kind, pass, layout and flag combination and every
    N the tests of this file enumerate, and for every row of the table (its knobs included) with its B set to 0, in both
    builds.  The launchers rest on it: none of them looks for an empty batch."""
    for r in routes.values():
        for pas, kinds in ((0, (QP, QCQP, BOX, SBOX)), (1, (QP, QCQP, BOX))):
            for kind in kinds:
                for N in list(range(1, 80)) + [96, 128, 200]:
                    for layout in (AUTO, DENSE, DIAG):
                        for flags in (0, REF, XD, XL, XD | XL, REF | XD | XL):
                            o = raw_plan(r, pas, kind, N, 0, layout | flags)
                            assert o[0] == (-2 if kind == QCQP and N % 2 else 0), (pas, kind, N, layout | flags)
                            assert o[2:5] == [0, 0, 0] and o[9] == 0, (pas, kind, N, layout | flags)
        for pas, kind, N, _, p_layout, knobs, _ in TABLE:
            o = raw_plan(r, pas, kind, N, 0, p_layout, **knobs)
            assert o[2:5] == [0, 0, 0] and o[9] == 0, (pas, kind, N, p_layout, knobs)


def test_workspace_bytes(routes):
    """dqq_workspace_bytes, from route.cpp alone: the header (3104 ints) and 32 segments of B / 32 + 512
    entries, rounded up to 64 ints; B < 0 as B = 0."""
    for r in routes.values():
        for B in (-5, -1, 0, 1, 31, 32, 33, 63, 64, 65, 1000, 65536, 65537, (1 << 31) - 1):
            ints = 3104 + 32 * (max(B, 0) // 32 + 512)
            assert r.route_workspace_bytes(B) == 4 * ((ints + 63) // 64 * 64), B


@pytest.fixture(scope="module")
def lib():
    from diffqcqp_amd import build, _capi
    build.build()
    return _capi.ctypes_lib()


def test_queries_follow_the_plans(routes, lib):
    """dqq_scratch_bytes > 0 exactly when the plan of that size takes the global-memory kernels (the query does not look at
    the layout: it answers for the general path, which DQQ_P_DIAG never takes); dqq_max_n is where they start."""
    r = routes[False]
    for pas, kinds in ((0, (QP, QCQP, BOX, SBOX)), (1, (QP, QCQP, BOX))):
        for kind in kinds:
            for N in list(range(1, 80)) + [96, 128, 200]:
                for B in (0, 1, 300, 65536):
                    for flags in (0, REF, XD | XL):
                        scratch = lib.dqq_scratch_bytes(kind, pas, N, B, flags)
                        for layout in (AUTO, DENSE, DIAG):
                            o = raw_plan(r, pas, kind, N, B, layout | flags)
                            if o[0] != 0:
                                continue
                            if layout == DIAG:
                                assert not o[3]
                            else:
                                assert o[3] == (scratch > 0), (pas, kind, N, B, layout | flags)
                        which = (1 if kind == QCQP else 0) if pas == 0 else {QP: 0, QCQP: 2, BOX: 3}[kind]
                        if B > 0 and not (kind == QCQP and N % 2):
                            plan = raw_plan(r, pas, kind, N, B, DENSE | flags)
                            assert (FAMILY[plan[4]] in ("fany", "bany")) == (N > lib.dqq_max_n(which, flags))
    assert lib.dqq_scratch_bytes(SBOX, 1, 200, 10, 0) == 0
    for B in (-5, -1, 0, 1, 31, 32, 33, 63, 64, 65, 1000, 65536, 65537, (1 << 31) - 1):
        assert lib.dqq_workspace_bytes(B) == r.route_workspace_bytes(B)


def test_hint_flags_follow_the_plans(routes, lib):
    """The flags dqq_hint_flags derives from a report word are taken by the plan of that call: DQQ_F_EXPECT_DENSE moves a
    backward whole to the lane kernel (a forward of N = 8 to one lane per problem where two would run),
    DQQ_F_EXPECT_LONG_LIST drains with it."""
    r = routes[False]
    for kind in (QP, QCQP, BOX):
        for N in (2, 4, 6, 8, 16):
            for B in (1000, 16383, 16384, 24575, 24576, 57344, 65536):
                for count in (0, 100, B // 4, B // 2, (3 * B) // 4, B):
                    for streak in (0, 1, 3):
                        for single in (0, 1):
                            word = (streak << 62) | ((B & 0x3fffffff) << 32) | (single << 31) | count
                            for pas in (0, 1):
                                flags = lib.dqq_hint_flags(kind, pas, N, B, word)
                                assert r.route_hint_flags(kind, pas, N, B, word) == flags   # (the same function, host shim)
                                if flags == 0:
                                    continue
                                assert kind in (QP, QCQP) and N % 2 == 0 and N <= 8, (kind, pas, N, B, word)
                                got = render(raw_plan(r, pas, kind, N, B, AUTO | flags))
                                if N == 6:   # no fast path: DQQ_P_AUTO is DQQ_P_DENSE, where the hints change nothing
                                    assert got == render(raw_plan(r, pas, kind, N, B, AUTO))
                                elif pas == 0:
                                    assert flags == XD and N == 8
                                    assert got.startswith("fdiag/1/fuse") if B >= 57344 else got.startswith("fdiag/4/fuse")
                                elif flags & XD:
                                    assert got == "blane/m2 ws #whole"
                                else:
                                    assert flags == XL and N in (2, 4, 8) and got == "bdiag + blane/m1 ws #drains"
    word = (1 << 62) | (65536 << 32) | 65536   # arguments that describe no call: no flags, from either
    for args in ((QP, 1, 8, 0, word), (QP, 1, 8, -1, word), (QP, 2, 8, 65536, word), (QP, -1, 8, 65536, word),
                 (7, 1, 8, 65536, word), (-1, 0, 8, 65536, word), (SBOX, 0, 8, 65536, word), (QP, 1, 7, 65536, word)):
        assert lib.dqq_hint_flags(*args) == r.route_hint_flags(*args) == 0, args
