"""CPU check of the signed box QP backward's routes (diffqcqp_amd/csrc/route.cpp), on the harness of tests/test_routes.py:
plan_bwd(kind 3) is plan_bwd(kind 2) -- same families, same drain, same work-list and scratch, no hints, never fused --, the
rows of tests/test_gpu_sbox_bwd.py take the kernels they name, and dqq_scratch_bytes(3, 1, ...) still answers 0 (the entry
point is sized by the box QP's query, include/diffqcqp_hip.h)."""
import pytest

from test_routes import AUTO, BOX, DENSE, DIAG, REF, SBOX, XD, XL, raw_plan, render, routes  # noqa: F401 (routes: fixture)

NS = list(range(1, 80)) + [96, 128, 200]
BS = (0, 1, 300, 65536)
FLAGS = [a | b | c for a in (0, REF) for b in (0, XD) for c in (0, XL)]

# the rows of tests/test_gpu_sbox_bwd.py: (row, N, B, p_layout, route)
ROWS = [("a", 8, 97, DIAG, "bdiag"),
        ("b", 8, 97, AUTO, "bdiag + bteam ws"),
        ("c", 8, 193, AUTO, "bdiag + bteam ws"),
        ("d", 2, 97, DENSE, "bsmall"),
        ("e", 5, 97, DENSE, "bteam"),
        ("f", 16, 97, DENSE, "bteam"),
        ("g", 21, 33, DENSE, "bteam"),
        ("h", 22, 17, DENSE, "bany scr"),
        ("i", 32, 65, AUTO, "bdiag + bany ws scr")]


def test_signed_box_backward_is_routed_as_the_box_backward(routes):
    for tuning, r in routes.items():
        for N in NS:
            for B in BS:
                for layout in (AUTO, DENSE, DIAG):
                    for flags in FLAGS:
                        signed, box = raw_plan(r, 1, SBOX, N, B, layout | flags), raw_plan(r, 1, BOX, N, B, layout | flags)
                        assert signed == box, (tuning, N, B, layout | flags, signed, box)
    # ... with the developer build's knobs off their defaults too (the box QP never fuses, never runs a lane per problem)
    r = routes[True]
    for knobs in ({"fuse_fallback": 1}, {"small_bwd": 0}, {"lane_bwd": 0}, {"bwd_skip_classify": 0}):
        for N in (2, 4, 8, 16, 21, 22, 32):
            for layout in (AUTO, DENSE):
                assert raw_plan(r, 1, SBOX, N, 65536, layout, **knobs) == raw_plan(r, 1, BOX, N, 65536, layout, **knobs)
    # (not a comparison of two errors: the plans launch something)
    assert render(raw_plan(routes[False], 1, SBOX, 8, 65536, AUTO | XD | XL)) == "bdiag + bteam ws"


@pytest.mark.parametrize("row,N,B,p_layout,want", ROWS)
def test_rows_of_the_gpu_test_take_the_kernels_they_name(routes, row, N, B, p_layout, want):
    for r in routes.values():
        assert render(raw_plan(r, 1, SBOX, N, B, p_layout)) == want
        assert render(raw_plan(r, 1, SBOX, N, B - 1, p_layout)) == want     # (the sliced call of the contract test)


def test_argument_errors_are_the_box_backwards(routes):
    r = routes[False]
    for N, B, p_layout in ((0, 10, AUTO), (8, -1, AUTO), (8, 10, 3), (8, 10, AUTO | 0x800), (5, 10, DIAG), (22, 10, DIAG)):
        o = raw_plan(r, 1, SBOX, N, B, p_layout)
        assert o[0] != 0 and o == raw_plan(r, 1, BOX, N, B, p_layout)


@pytest.fixture(scope="module")
def lib():
    from diffqcqp_amd import build, _capi
    build.build()
    return _capi.ctypes_lib()


def test_scratch_query_of_kind_3_is_unchanged(lib):
    """dqq_scratch_bytes(3, 1, ...) == 0 as before the backward existed; the entry point's scratch is the kind-2 query's, which
    is not 0 exactly beyond dqq_max_n(3) = 21."""
    for N in NS:
        for B in BS:
            for flags in (0, REF):
                assert lib.dqq_scratch_bytes(SBOX, 1, N, B, flags) == 0
                assert (lib.dqq_scratch_bytes(BOX, 1, N, B, flags) > 0) == (N > 21 and B > 0)
    assert lib.dqq_max_n(3, 0) == 21
    assert hasattr(lib, "dqq_signedboxqp_bwd_f64")
