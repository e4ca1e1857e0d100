"""The rows of tests/test_gpu_path_trips.py: the persistent dense kernels of dqq_polish_path_f64 (polish_dense_path.hip) past their
first trip through the batch, in tests/trip_cases.py's pattern.  Not a test file.  The path's kernels launch with the damped
polish's geometry -- polish_team.h's slice through team_dense.h's team_geometry (the LDS teams: a grid capped at 256 * 8 workgroups
of 1 .. 4 waves of 64 / T teams), any_grid's 512 workgroups for the any-N form --, so the problems a launch holds at a time are
tests/newton_trip_cases.py's per_trip of "polish_ls", and the batch is its batch_size: two full trips of every team and a ragged
third.  One row per team width, the kinds rotating; the schedule is the default one, which the problems of every row's base leave
after different numbers of steps."""
import newton_trip_cases as T
from trip_cases import base_size

# (kind, N): T = 8, 16, 32, 64 with four waves per workgroup, T = 64 with one, and the any-N form
ROWS = (("qp", 6), ("qcqp", 12), ("box", 20), ("sbox", 34), ("qp", 64), ("qcqp", 66))
POISON_NAN, POISON_INF = 1, 4       # problems of the first trip


def geometry(kind, N):
    """-> (problems per trip, the batch, the base's size)"""
    per = T.per_trip("polish_ls", kind, N)
    return per, T.batch_size(per), base_size(N)
