"""The cases of tests/test_gpu_parameters.py: one row per kernel route, as data, and the inputs those tests feed it.

A row is (pass, kind, N, B, p_layout, structure, expected route).  The route is written the way tests/test_routes.py renders
a plan ('<first launch> [+ <drain>] [ws] [scr] [keep] [#counter]'); tests/test_param_cases.py checks every row against
route.cpp on the CPU and that the rows together reach every kernel family the plans can reach for each kind.  Each row sits
on the near side of a threshold of tests/test_routes.py:TABLE.

Inputs: make_problem's data.  A batch larger than base_size(N, B) repeats a base batch of that many problems, so that the oracle solves
the base once and every problem of the kernel's batch is still checked (problem b is problem b mod base).

nudge() (tools/oracle_params.py): the backward's inputs -- the oracle's forward x with a share of the constraints made barely inactive, so that the
dual-recovery threshold `epsilon` decides the active set."""
import numpy as np

from tools.oracle_params import nudge  # noqa: F401  (shared with tools/fuzz_bwd.py)

AUTO, DENSE, DIAG = 0, 1, 2
REF, XD, XL = 0x100, 0x200, 0x400          # DQQ_F_REFERENCE_ORDER, DQQ_F_EXPECT_DENSE, DQQ_F_EXPECT_LONG_LIST
F, Bw = 0, 1
KIND = {"qp": 0, "qcqp": 1, "box": 2, "sbox": 3}
K4 = ("qp", "qcqp", "box", "sbox")

FWD = (
    [(F, k, 8, 2051, AUTO, "mixed", "fdiag/4/fuse ws keep") for k in K4] +           # group solve in the fused kernel
    [(F, k, 8, 57344, AUTO, "mixed", "fdiag/2/fuse ws keep") for k in K4] +
    [(F, k, 4, 131073, AUTO, "mixed", "fdiag/1 + flane ws keep") for k in K4] +      # one past the fuse limit: drain
    [(F, k, 8, 57344, AUTO | XD, "mixed", "fdiag/1/fuse ws keep #feedback") for k in ("qp", "qcqp")] +
    [(F, k, 8, 2051, DIAG, "diag", "fdiag/4") for k in K4] +
    [(F, k, 16, 300, AUTO, "mixed", "fdiag/8 + fsmall ws keep") for k in K4] +
    [(F, k, 32, 130, AUTO, "mixed", "fdiag/16 + fwave64 ws keep") for k in K4] +
    [(F, k, 64, 40, AUTO, "mixed", "fdiag/32 + fwave64 ws keep") for k in K4] +
    [(F, k, 32, 60, AUTO | REF, "mixed", "fdiag/16 + flds ws keep") for k in K4] +
    [(F, k, 8, 32769, DENSE, "dense", "flane") for k in ("qp", "qcqp")] +
    [(F, k, 8, 300, DENSE, "dense", "flane") for k in ("box", "sbox")] +
    [(F, k, 6, 300, AUTO, "dense", "flane") for k in K4] +
    [(F, k, 12, 200, AUTO, "dense", "fsmall") for k in K4] +
    [(F, k, 24, 130, AUTO, "dense", "fwave64") for k in K4] +
    [(F, k, 5, 200, AUTO, "dense", "flds") for k in ("qp", "box", "sbox")] +
    [(F, k, 18, 64, AUTO | REF, "dense", "flds") for k in K4] +
    [(F, k, 70, 6, AUTO, "dense", "fany scr") for k in K4]
)

BWD = (
    [(Bw, k, 8, 2051, AUTO, "mixed", "bdiag + bsmall ws") for k in ("qp", "qcqp")] +
    [(Bw, "box", 8, 2051, AUTO, "mixed", "bdiag + bteam ws")] +
    [(Bw, k, 8, 2051, DIAG, "diag", "bdiag") for k in ("qp", "qcqp", "box")] +
    [(Bw, k, 8, 24576, DENSE, "dense", "blane/m0") for k in ("qp", "qcqp")] +
    [(Bw, k, 8, 24576, AUTO | XL, "mixed", "bdiag + blane/m1 ws #drains") for k in ("qp", "qcqp")] +
    [(Bw, k, 8, 24576, AUTO | XD, "mixed", "blane/m2 ws #whole") for k in ("qp", "qcqp")] +
    [(Bw, k, 12, 200, DENSE, "dense", "bsmall") for k in ("qp", "qcqp")] +
    # box N = 2 (its only bsmall size): with two coordinates per problem at most 1 - (1 - 0.4/2)^2 = 36 % of the problems
    # get a nudge below 1e-6, short of the 40 % that rows of B >= 64 must move; a small row: at least one problem
    [(Bw, "box", 2, 60, AUTO, "mixed", "bdiag + bsmall ws")] +
    [(Bw, "qp", 24, 130, DENSE, "dense", "bchol"), (Bw, "qcqp", 24, 130, DENSE, "dense", "bqcqp"),
     (Bw, "qp", 48, 60, DENSE, "dense", "bchol"), (Bw, "qcqp", 48, 60, DENSE, "dense", "bqcqpbig")] +
    [(Bw, "qp", 5, 200, DENSE, "dense", "bteam"), (Bw, "qcqp", 18, 64, DENSE | REF, "dense", "bteam"),
     (Bw, "box", 16, 300, AUTO, "mixed", "bdiag + bteam ws"), (Bw, "box", 4, 300, AUTO, "mixed", "bdiag + bteam ws")] +
    [(Bw, k, 70, 6, DENSE, "dense", "bany scr") for k in ("qp", "qcqp")] +
    [(Bw, "box", 32, 48, AUTO, "mixed", "bdiag + bany ws scr")]
)

# the families a row's launches belong to (what tests/test_param_cases.py counts as covered)
FWD_FAMILIES = ("fdiag/1", "fdiag/2", "fdiag/4", "fdiag/8", "fdiag/16", "fdiag/32", "fdiag alone", "fdiag + drain",
                "flane", "fsmall", "fwave64", "flds", "fany")
BWD_FAMILIES = ("bdiag", "blane/m0", "blane/m1", "blane/m2", "bsmall", "bchol", "bqcqp", "bqcqpbig", "bteam", "bany")


def families(route):
    """The families a rendered route launches: 'fdiag/2/fuse ws keep' -> {'fdiag/2', 'fdiag alone'}."""
    launches = [w for w in route.split(" + ")]
    launches = [launches[0].split(" ")[0]] + [w.split(" ")[0] for w in launches[1:]]
    out = set()
    for i, l in enumerate(launches):
        parts = l.split("/")
        if parts[0] == "fdiag":
            out.add("fdiag/" + parts[1])
            out.add("fdiag + drain" if len(launches) > 1 else "fdiag alone")
        elif parts[0] == "blane":
            out.add("blane/" + parts[1])
        elif parts[0] not in ("-",) and not parts[0].startswith("E"):
            out.add(parts[0])
    return out


def row_id(row):
    pas, kind, N, B, layout, structure, _ = row
    return "%s-%s-N%d-B%d-L%#x-%s" % ("fwd" if pas == F else "bwd", kind, N, B, layout, structure)


def base_size(N, B):
    return min(B, 4096 if N <= 8 else 1024 if N <= 16 else 256 if N <= 32 else 64)


# rows whose first seed missed a condition of tests/test_gpu_parameters.py (a share of problems that mu_prox moves)
SEED = {"fwd-sbox-N4-B131073-L0x0-mixed": 23001}


def row_seed(row):
    pas, kind, N, B, layout, structure, _ = row
    if row_id(row) in SEED:
        return SEED[row_id(row)]
    return 20000 + 1000 * KIND[kind] + 100 * pas + N + (layout >> 8) * 7 + {"diag": 0, "dense": 1, "mixed": 2}[structure] * 3


def row_problem(row, make_problem):
    """(base batch, tiled batch) as dicts of CPU tensors; the tiled batch has the row's B problems."""
    pas, kind, N, B, layout, structure, _ = row
    base = make_problem(kind, base_size(N, B), N, row_seed(row), structure)
    reps = -(-B // base["q"].shape[0])
    full = {k: v.repeat((reps,) + (1,) * (v.dim() - 1))[:B].contiguous() for k, v in base.items()}
    return base, full


def tile(a, B):
    """A base-batch array repeated to B problems (the layout of row_problem's tiled batch)."""
    reps = -(-B // a.shape[0])
    return np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:B]
