"""CPU account of which instantiations of the smoothed Newton Jacobians' kernels a device row launches, in the manner of
tests/test_instantiation_cases.py: the library compiles dispatch_diag_n's six N x four kinds on the compact diagonal
(newton_jac_diag_smooth.hip), team_width's four widths x four kinds on the LDS teams and the any-N form x four kinds
(newton_jac_dense_smooth.hip) -- 44 kernels, no REG doubling and no mode.  A row's cell is taken from plan_newton_jac_smooth compiled
for the host (tests/hostcore/jac_smooth_route_check.cpp), not from the row's label.  Builds nothing but a host library."""
import jac_smooth_cases as C

DIAG_N = (2, 4, 8, 16, 32, 64)
WIDTHS = (8, 16, 32, 64)


def compiled():
    return {(k, form, size) for k in C.KINDS for form, size in [("diag", N) for N in DIAG_N] + [("team", w) for w in WIDTHS] + [("any", 0)]}


def missing(rows):
    reached = {C.cell(*row) for row in rows}
    assert None not in reached and reached <= compiled()
    return sorted(compiled() - reached, key=str)


def test_the_list_is_what_the_library_compiles():
    assert len(compiled()) == 4 * 11
    for kind in C.KINDS:
        for N in range(2, 67, 2):
            assert (C.plan(kind, N, 37, C.DIAG)[0] == 0) == (N in DIAG_N)
    assert sorted({C.team_width(N) for N in range(1, 65)}) == list(WIDTHS) and C.team_width(65) == 256


def test_every_compiled_instantiation_is_launched_by_a_bit_equality_row():
    assert missing(C.device_rows()) == []


def test_the_rows_are_ragged():
    """B of 37 and 67: no tile of 128/N problems and no wave of 64/T teams divides them."""
    assert {B for _, _, B, _ in C.device_rows()} == {37, 67}


def test_the_account_fails_when_a_size_leaves_the_table():
    rows = [r for r in C.device_rows() if not (r[1] == 16 and r[3] == C.DIAG)]
    assert missing(rows) == sorted(((k, "diag", 16) for k in C.KINDS), key=str)
    rows = [r for r in C.device_rows() if r[3] == C.DIAG or C.team_width(r[1]) != 16]
    assert missing(rows) == sorted(((k, "team", 16) for k in C.KINDS), key=str)


def test_kappa_zero_rows_launch_no_smoothed_kernel():
    assert all(C.cell(k, N, B, layout, 0.0, 0.0) is None for k, N, B, layout in C.device_rows())
