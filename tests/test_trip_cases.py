"""CPU check of tests/trip_cases.py, what tests/test_gpu_trips.py stands on: every row takes the route it names, its B (or the
work-list its batch produces) sends each worker of the persistent kernel through at least two trips and ends inside a third,
per_trip is the launch geometry -- for the global-memory kernels also the library's own count of scratch slices --, the base
batch alone takes the same kernels in at most one trip, and the base is heterogeneous in what a worker keeps between trips."""
import pytest

from param_cases import KIND, families
from test_routes import _build, raw_plan, render
from trip_cases import (CITED, ROWS, Bw, F, base_size, check_heterogeneous, covered, launches, list_len, listed_mask,
                        one_trip_size, per_trip, persistent_launch, row_id)


@pytest.fixture(scope="module")
def shipped():
    return _build(False)


@pytest.fixture(scope="module")
def lib():
    from diffqcqp_amd import build, _capi
    build.build()
    return _capi.ctypes_lib()


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_row_takes_its_route_and_so_does_its_base(shipped, row):
    pas, kind, N, B, layout, _, want = row[:7]
    assert render(raw_plan(shipped, pas, KIND[kind], N, B, layout)) == want
    n1 = one_trip_size(row)
    one_trip = render(raw_plan(shipped, pas, KIND[kind], N, n1, layout))
    assert families(one_trip) == families(want), (one_trip, want)
    assert base_size(N) <= n1 <= row[7]


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_batch_is_two_trips_and_a_ragged_third(row):
    pas, kind, N, B = row[:4]
    launch, listed = persistent_launch(row)
    assert row[7] == per_trip(launch, kind, N, listed), row_id(row)
    n = covered(row)
    assert n >= 2 * row[7] + 1 and n % row[7] != 0, (row_id(row), n, row[7])
    if listed:
        assert n == list_len(row) <= B
        if pas == F or N < 64:
            # every problem is the drain's, in the full batch and in the one-trip call: the rows compare bits of ONE kernel
            assert all(listed_mask(row, B)) and all(listed_mask(row, one_trip_size(row))[:base_size(N)]), row_id(row)


def test_list_len_counts_whole_tiles():
    # N = 8 backward: 16 problems per wave tile, every tile of a mixed batch holds a dense problem; N = 64: tiles of two
    assert list_len((Bw, "box", 8, 4099, 0, "mixed", "bdiag + bteam ws")) == 4099
    row = (Bw, "qcqp", 64, 10, 0x100, "mixed", "bdiag + bany ws scr")
    assert list_len(row) == 6   # dense: 1, 4, 7 -> the tiles (0,1), (4,5), (6,7)
    assert list_len(row[:3] + (2,) + row[4:]) == 2 and list_len(row[:3] + (1,) + row[4:]) == 0


@pytest.mark.parametrize("row", [r for r in ROWS if persistent_launch(r)[0] in ("fany", "bany")], ids=row_id)
def test_per_trip_is_the_librarys_count_of_scratch_slices(lib, row):
    pas, kind, N, B, layout = row[:5]
    k = 2 if (pas == Bw and kind == "sbox") else KIND[kind]   # the signed box backward takes the box QP's scratch
    piece = lib.dqq_scratch_bytes(k, pas, N, 1, layout)
    assert piece > 0 and lib.dqq_scratch_bytes(k, pas, N, B, layout) == row[7] * piece
    # the variant the row names: both O(n^3) matrices in LDS (the slice holds the vectors, in the backward K too) or in the slice
    rows = N if (pas == F or kind == "qp") else (N + N // 2 if kind == "qcqp" else 3 * N)
    mat = 8 * rows * (rows | 1)
    assert (piece > 2 * mat) == (2 * mat > 152 * 1024), row_id(row)


def test_rows_cover_what_the_issue_of_trips_asks_for():
    have = {(r[0], r[1], r[2], persistent_launch(r)) for r in ROWS}
    for k in ("qp", "qcqp", "box", "sbox"):
        assert (F, k, 70, ("fany", False)) in have
    for want in [(F, "qp", 100, ("fany", False)), (F, "qcqp", 100, ("fany", False)),
                 (Bw, "qp", 70, ("bany", False)), (Bw, "qcqp", 44, ("bany", False)), (Bw, "box", 22, ("bany", False)),
                 (Bw, "sbox", 22, ("bany", False)), (Bw, "qp", 100, ("bany", False)), (Bw, "qcqp", 66, ("bany", False)),
                 (Bw, "box", 34, ("bany", False)), (Bw, "box", 32, ("bany", True)), (Bw, "qcqp", 64, ("bany", True)),
                 (F, "qp", 5, ("flds", False)), (F, "box", 5, ("flds", False)), (F, "sbox", 5, ("flds", False)),
                 (F, "qcqp", 18, ("flds", False)), (Bw, "qp", 5, ("bteam", False)), (Bw, "qcqp", 18, ("bteam", False)),
                 (Bw, "box", 8, ("bteam", True)), (Bw, "qp", 10, ("bsmall", False))]:
        assert want in have, want
    assert any(r[0] == F and r[2] == 32 and persistent_launch(r) == ("flds", True) for r in ROWS)
    assert set(CITED) == {("fsmall", "both"), ("bsmall", "list"), ("fwave64", "list"), ("bchol", "list"), ("bqcqp", "list"),
                          ("bqcqpbig", "list")}
    assert len({r[:6] for r in ROWS}) == len(ROWS) and all(len(launches(r[6])) <= 2 for r in ROWS)


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_base_is_heterogeneous(oracle, row):
    check_heterogeneous(row)
