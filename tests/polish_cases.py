"""Inputs and host-side yardsticks of the polish tests -- tests/test_polish_*.py on the CPU, tests/test_gpu_polish.py on the
device.  Not a test file.  Problems: make_problem's families with every P re-conditioned by warm_cases.well_conditioned
(spectrum on [0.5, 2]); starts: the oracle's forward stopped early.  The yardstick of the kernels is the host core
(tests/hostcore/polish_core_check.cpp: csrc/polish_core.h on one CPU thread, a stand-alone program), itself held bit-equal to
the numpy restatement tests/polish_reference.py.  Two builds of that program: a plain one, the yardstick of the device tests,
and one with the address and undefined-behaviour sanitizers that only the CPU test tests/test_polish_hostcore.py runs."""
import functools
import os
import subprocess
import tempfile

import numpy as np

import polish_reference as R
from conftest import make_problem
from warm_cases import well_conditioned

HERE = os.path.dirname(os.path.abspath(__file__))
EXTRAS = {"qp": (), "qcqp": ("l_n", "mu"), "box": ("l_min", "l_max"), "sbox": ("l_min", "l_max", "v")}
KINDS = tuple(EXTRAS)
MAX_STEPS = 8
EPS_START, MAX_ITER = 1e-3, 100000     # the oracle's forward the polish starts from
B_CPU = 32
BATCHES = [(k, N, s) for k in KINDS for N in (8, 20) for s in ("diag", "dense")]

GOLDEN = os.path.join(HERE, "golden", "polish")

# The sizes of the device tables (tests/test_instantiation_cases.py holds them against what the library compiles).  The compact
# diagonal: every N of diag_tile.h's dispatch_diag_n.  N = 4, 16, 32 run at ragged_b(N) = 9 (128/N) + 1 problems: two whole
# workgroups of four tiles, one more tile and one problem -- the last wave holds a single valid problem.  The LDS teams: one N per
# width of team_dense.h's team_width -- 8 (N = 3 or 4, and 8), 16 (N = 12), 32 (N = 20), 64.
AUTO, DENSE, DIAG = 0, 1, 2               # p_layout, for every *_cases.py module and the device tests that read their tables
DIAG_N_FIRST, DIAG_N_MORE = (2, 8, 64), (4, 16, 32)
TEAM_N16 = 12
# what tests/test_gpu_polish.py runs over its tables, read by the test and by the account alike: the entry, and the layouts of
# the team rows (the diagonal rows run DQQ_P_DIAG, the any-N rows DQQ_P_DENSE)
ENTRIES = ("polish",)
TEAM_LAYOUTS = (AUTO, DENSE)


def ragged_b(N):
    return 9 * (128 // N) + 1


# (kind, N, B) of tests/test_gpu_polish.py
DIAG_ROWS = [(k, N, 67) for k in KINDS for N in DIAG_N_FIRST] + [(k, N, ragged_b(N)) for k in KINDS for N in DIAG_N_MORE]
TEAM_ROWS = [("qp", 3, 37), ("box", 3, 37)] + [(k, N, 37) for k in KINDS for N in (8, TEAM_N16, 20, 64)]
ANY_ROWS = [("qp", 65, 5), ("qcqp", 66, 5)]

# The largest r_after / resid[3] the numpy restatement leaves on BATCHES and on the figure workload (B_CPU problems each,
# MAX_STEPS steps), as measured, to two digits: tests/test_polish_reference.py measures it again and holds the record to those
# digits.  The measurement is made on the FROZEN batches of tests/golden/polish (frozen() below; golden/make_polish_golden.py
# wrote them from problem() and figure_workload()): those builders' last bits differ between hosts (eigh, BLAS, the oracle's
# compiled forward), and a maximum of few-ulp residuals over several hundred problems moves in its first digit with them -- 2.8e-16
# on one host, 4.6e-16 on another --, while the restatement on given inputs is elementwise IEEE arithmetic, the same everywhere.
# The bar of every "reaches machine precision" assertion is 64 x this record: an r of a few ulps of the scale is one rounding
# of a row sum of up to 20 terms (N 2^-53 of the scale) times a small factor.
RESIDUAL_CPU = 2.8e-16
BAR = 64 * RESIDUAL_CPU


def seed_of(kind, N, structure):
    return 71000 + 1000 * R.KIND[kind] + 10 * N + (structure == "diag")


def flat(d, kind):
    """make_problem's dict -> (P (B,N,N), q (B,N), extras each (B,.)) as numpy arrays."""
    B = d["q"].shape[0]
    return d["P"], d["q"].reshape(B, -1), tuple(d[n].reshape(B, -1) for n in EXTRAS[kind])


def oracle_forward(kind, d, eps, max_iter):
    from oracle import oracle as O
    O.build()
    if kind == "qp":
        return O.qp_fwd_batch(d["P"], d["q"], eps, max_iter)[0]
    if kind == "qcqp":
        return O.qcqp_fwd_batch(d["P"], d["q"], d["l_n"], d["mu"], eps, max_iter)[0]
    return O.boxqp_fwd_batch(d["P"], d["q"], d["l_min"], d["l_max"], eps, max_iter, v=d.get("v"))[0]


def _freeze(d, x):
    for a in list(d.values()) + [x]:
        a.setflags(write=False)
    return d, x


@functools.lru_cache(maxsize=None)
def problem(kind, N, B, structure="dense"):
    """-> (d: make_problem's dict as read-only numpy arrays, P with its spectrum on [0.5, 2]; x: the oracle's forward at
    eps = 1e-3, (B,N,1))."""
    t = make_problem(kind, B, N, seed_of(kind, N, structure), structure)
    t["P"] = well_conditioned(t["P"])
    d = {k: np.ascontiguousarray(v.numpy()) for k, v in t.items() if k != "grad_x"}
    return _freeze(d, np.ascontiguousarray(oracle_forward(kind, d, EPS_START, MAX_ITER)))


@functools.lru_cache(maxsize=None)
def ill_conditioned(kind, N, B):
    """Condition number about 60 (make_problem's dense family as it is: eigenvalues from 0.1 to about N / 4 + 0.1 ... scaled
    below), rough start: 10 oracle iterations."""
    import torch
    t = make_problem(kind, B, N, 5 + seed_of(kind, N, "dense"), "dense")
    lam, V = torch.linalg.eigh(t["P"])
    lo, hi = lam[:, :1], lam[:, -1:]
    t["P"] = (V @ torch.diag_embed(1.0 + 59.0 * (lam - lo) / (hi - lo)) @ V.transpose(1, 2))
    t["P"] = (0.5 * (t["P"] + t["P"].transpose(1, 2))).contiguous()
    d = {k: np.ascontiguousarray(v.numpy()) for k, v in t.items() if k != "grad_x"}
    return _freeze(d, np.ascontiguousarray(oracle_forward(kind, d, 1e-12, 10)))


@functools.lru_cache(maxsize=None)
def figure_workload(B=B_CPU, N=8, max_iter=20):
    """The reference's figure workload -- QP, P = diag(exp(U(-10, 10))), q ~ N(0, 1) -- from the oracle stopped at max_iter."""
    r = np.random.default_rng(20240)
    p = np.exp(r.uniform(-10.0, 10.0, (B, N)))
    d = {"P": np.ascontiguousarray(np.stack([np.diag(v) for v in p])), "q": r.standard_normal((B, N, 1))}
    return _freeze(d, np.ascontiguousarray(oracle_forward("qp", d, 1e-12, max_iter)))


def golden_path(kind, N, structure):
    return os.path.join(GOLDEN, "%s_%s_n%d.npz" % (kind, structure, N))


@functools.lru_cache(maxsize=None)
def frozen(kind, N, structure):
    """problem(kind, N, B_CPU, structure), or with structure "figure" figure_workload(), as tests/golden/polish holds it:
    the same arrays on every host.  -> (d, x) in problem()'s form."""
    with np.load(golden_path(kind, N, structure)) as z:
        d = {k: np.ascontiguousarray(z[k]) for k in z.files if k != "x"}
        x = np.ascontiguousarray(z["x"])
    if d["P"].ndim == 2:
        d["P"] = np.ascontiguousarray(np.stack([np.diag(v) for v in d["P"]]))
    return _freeze(d, x)


def compact(P):
    """(B,N,N) -> the diagonals (B,N)."""
    return np.ascontiguousarray(np.diagonal(P, axis1=1, axis2=2))


@functools.lru_cache(maxsize=None)
def hostcore(sanitized=False):
    """The host program's path, built on demand.  sanitized: the build with -fsanitize=address,undefined -- for CPU tests only;
    a test marked gpu uses the plain build."""
    src = os.path.join(HERE, "hostcore", "polish_core_check.cpp")
    exe = os.path.join(HERE, "hostcore", "polish_core_check_san" if sanitized else "polish_core_check")
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else ["-O2"]
    deps = [src] + [os.path.join(HERE, "..", "diffqcqp_amd", "csrc", f)
                    for f in ("polish_core.h", "check_core.h", "sbox_bounds.h", "common.h", "route.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(p) > os.path.getmtime(exe) for p in deps):
        subprocess.check_call(["g++"] + extra + ["-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", exe + ".tmp", src])
        os.replace(exe + ".tmp", exe)
    return exe


def host_polish(kind, P, q, ex, x, max_steps=MAX_STEPS, diag=False, in_place=False, sanitized=False):
    """The host core over a batch.  P (B,N,N), or (B,N) with diag; q, x (B,N); ex each (B,.) -> x_out, resid, steps, status.
    sanitized: run the sanitizer build (hostcore)."""
    B, N = x.shape
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in (P, q) + tuple(ex) + (x,)]
    assert arrays[0].shape == ((B, N) if diag else (B, N, N))
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        with open(fin, "wb") as f:
            f.write(np.array([R.KIND[kind], B, N, int(diag), max_steps, int(in_place)], dtype=np.int32).tobytes())
            for a in arrays:
                f.write(a.tobytes())
        subprocess.check_call([hostcore(sanitized), fin, fout])
        raw = open(fout, "rb").read()
    nd = B * N + 2 * B
    dbl = np.frombuffer(raw[: 8 * nd], dtype=np.float64)
    ints = np.frombuffer(raw[8 * nd:], dtype=np.int32)
    assert ints.size == 2 * B
    return dbl[: B * N].reshape(B, N).copy(), dbl[B * N:].reshape(B, 2).copy(), ints[:B].copy(), ints[B:].copy()


def same_bits(a, b):
    """Equal as bit patterns but for the payload of a NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=True)) and bool(
        np.array_equal(np.signbit(a[~np.isnan(a)]), np.signbit(b[~np.isnan(b)])))
