"""The cases of tests/test_gpu_newton_trips.py, as data: one row per persistent dense kernel of the Newton family (polish, damped
polish, Newton backward / JVP, Jacobians, active set; the REG = true units beside their parents), at a batch that sends every
team of its fixed grid through the batch at least twice and leaves the last trip ragged.  The model is tests/trip_cases.py, which
does the same for the ADMM solve kernels; tests/test_newton_trip_cases.py holds this table against route.cpp, the launch geometry
and the host cores on the CPU.

A row is (entry, kind, N, B, flags, reg, route, per_trip, where per_trip is set).  entry: the C function (ENTRY_FN); flags: ORed
into DQQ_P_DENSE, 0 or DQQ_F_INFINITE_BOUNDS; reg: the proximal weight, 0.0 for the entries that take none.  per_trip: the problems
ONE launch holds at a time -- its grid times the teams per workgroup --, restated in per_trip() from the launcher cited in `where`
(files of diffqcqp_amd/csrc).  The rule for B is trip_cases': B >= 2 * per_trip + 1 and B is no multiple of per_trip; every row
takes 2 * per_trip + 3.

Rows: every entry at every persistent width -- T = 8 (N = 6), 16 (N = 12), 32 (N = 20), 64 twice (N = 34: four waves per workgroup,
N = 64: one) and Any (N = 66, a 256-thread workgroup per problem on any_grid's 512 workgroups) -- with the kinds rotating over the
widths and the rotation starting one kind later per entry (START; the Jacobians' is set so that N = 34 runs more than one wave
per workgroup), so that every entry meets every kind and every width.  The first box
and the first signed-box row of every entry carry DQQ_F_INFINITE_BOUNDS on inf_bounds_cases' one-sided problems.  One T = 32 row
has N = 19, where ld = n | 1 = n.  Beside them: the damped polish with a weight, the Jacobians with a weight, and the Jacobians of
the box QP at N = 8, whose slice gives three waves per workgroup -- the only team count per workgroup that is no power of two.

Inputs: a base of trip_cases.base_size(N) problems (61 or 37, both prime: a team meets other problems on its second trip than on
its first) from the entry's own case builder, tiled to B on the device.  Problems 0 and 3 of the base are shaped so that what a
team keeps between problems differs as much as the entry allows:
  * polish entries: problem 0 is q = 0 from x = 0 -- r = 0 at once, no step, no elimination (status 1: "x kept");
  * the others: problem 0 sits strictly inside every bound (nothing active), problem 3 on a bound with z far outside wherever a
    bound is finite (at least three quarters of the elements active).
check_heterogeneous() asserts from the host core's outputs: polish entries -- step counts of 0 and of >= 2, status 0 exactly where
a step was accepted and 1 where none was (include/diffqcqp_hip.h: a start that is already a solution accepts nothing, so "every
clean problem has status 0" cannot hold beside "step counts include 0"; no clean problem has status 2), the damped polish also
halvings of 0 and of > 0; the others -- status 0 everywhere and active sets (active_cases.host_active: state != 0) of 0 and of
>= N / 2 elements (QCQP: problems with and without an active contact).

Poison (poisoned()): problem 1 gets a NaN in x, problem 4 P[0,0] = inf, problem 7 a singular system -- reg_cases' P with an
exactly duplicated row and column, every coordinate free, so that M = P and the elimination meets a zero pivot (the polish: on
its first solve).  All three lie below every row's per_trip.  The rows with a weight solve problem 7 and the active-set entry
eliminates nothing: they take the NaN and the inf problem only."""
import functools

import numpy as np

import polish_reference as R
from trip_cases import base_size

K4 = ("qp", "qcqp", "box", "sbox")
DENSE, F_INF = 1, 0x800
REG = 1e-7                      # reg_cases.REG: the weight of every row that takes one
MAX_HALVINGS = 8
MAX_STEPS = {"polish": 8, "polish_ls": 12}   # polish_cases.MAX_STEPS, polish_ls_cases.MAX_STEPS
POISON_NAN, POISON_INF, POISON_SINGULAR = 1, 4, 7
INSIDE, ACTIVE = 0, 3           # the shaped problems of the base

# entry -> (C function without / with a weight, the family of kernels, the route's stem in route.h's Family)
ENTRY = {
    "polish": ("dqq_polish_f64", "polish", "Polish"),
    "polish_reg": ("dqq_polish_reg_f64", "polish", "Polish"),
    "polish_ls": ("dqq_polish_ls_f64", "polish_ls", "PolishLs"),
    "bwd": ("dqq_newton_bwd_f64", "newton", "Newton"),
    "jvp": ("dqq_newton_jvp_f64", "newton", "Newton"),
    "bwd_reg": ("dqq_newton_bwd_reg_f64", "newton", "Newton"),
    "jvp_reg": ("dqq_newton_jvp_reg_f64", "newton", "Newton"),
    "jac": ("dqq_newton_jac_f64", "jac", "NewtonJac"),
    "jac_reg": ("dqq_newton_jac_reg_f64", "jac", "NewtonJac"),
    "active": ("dqq_newton_active_f64", "active", "Active"),
}
ENTRIES = ("polish", "polish_reg", "polish_ls", "bwd", "jvp", "bwd_reg", "jvp_reg", "jac", "active")   # the nine of the matrix
WIDTHS = ((8, 6), (16, 12), (32, 20), (64, 34), (64, 64), (256, 66))                                    # (T, N); 256: Any
# where per_trip is set: the slice, the loop's stride and the launcher per family; then the geometry they share
WHERE = {
    "polish": "polish_team.h:12, polish_dense.hip:123-129,146, team_dense.h:199-218 (launch_team)",
    "polish_ls": "polish_team.h:12, polish_dense_ls.hip:133-139,146, team_dense.h:199-218 (launch_team)",
    "newton": "newton_dense.hip:23,192-198,212, team_dense.h:199-218 (launch_team)",
    "jac": "newton_jac_dense.hip:30,161-167,190-192, newton_core.h:263, team_dense.h:199-218 (launch_team)",
    "active": "active_dense.hip:21-25,180-186,193-195, team_dense.h:199-218 (launch_team)",
}
GEOMETRY = "team_dense.h:165-174"
ANY_GRID = "general_any.hip:70-76"


def family(entry):
    return ENTRY[entry][1]


def is_polish(entry):
    return family(entry) in ("polish", "polish_ls")


def team_width(N):
    """team_dense.h:178-190 (team_width, dispatch_team); 256: the Any team of N > 64 (team_dense.h:21)."""
    return 8 if N <= 8 else 16 if N <= 16 else 32 if N <= 32 else 64 if N <= 64 else 256


def extra_cols(kind, N):
    """newton_core.h:263 (newton_jac_extra_cols)"""
    return 0 if kind == "qp" else (N // 2 if kind == "qcqp" else N)


def slice_doubles(entry, kind, N):
    """A team's slice in doubles, per family: polish_slice_doubles (polish_team.h:12; polish_vec_doubles: polish_core.h:60),
    newton_slice_doubles (newton_dense.hip:23; newton_vec_doubles: newton_core.h:130), jac_slice_doubles with every column
    requested (newton_jac_dense.hip:30,190), active_slice_doubles (active_dense.hip:21-25)."""
    mat, vec, fam = N * (N | 1), 7 * N, family(entry)
    if fam in ("polish", "polish_ls", "newton"):
        return (mat + vec + 1) & ~1
    if fam == "jac":
        return (mat + N * (N + 2 * extra_cols(kind, N)) + vec + 1) & ~1
    need, want = mat + N, (team_width(N) * (N | 1)) % 32
    return need + (want - need) % 32


def team_wpb(entry, kind, N):
    """Waves per workgroup of the LDS teams: as many as fit 64 KiB, 1 .. 4 (team_dense.h:167-170)."""
    per_wave = 8 * slice_doubles(entry, kind, N) * (64 // team_width(N))
    return min(4, max(1, 65536 // per_wave))


def per_trip(entry, kind, N):
    """Problems one launch holds at a time: the grid cap of 256 * 8 workgroups (team_dense.h:173) times wpb waves of 64 / T
    teams; the Any kernels: any_grid's 512 workgroups, a problem each (general_any.hip:72; the 4 GiB budget does not bind)."""
    if N > 64:
        return 512
    return 256 * 8 * team_wpb(entry, kind, N) * (64 // team_width(N))


def batch_size(per):
    B = 2 * per + 3
    while B % per == 0:
        B += 1
    return B


def _row(entry, kind, N, flags=0, reg=None):
    reg = (REG if entry.endswith("_reg") else 0.0) if reg is None else reg
    per = per_trip(entry, kind, N)
    route = ENTRY[entry][2] + ("Any" if N > 64 else "Team")
    where = "%s, %s" % (WHERE[family(entry)], ANY_GRID if N > 64 else GEOMETRY)
    return (entry, kind, N, batch_size(per), flags, reg, route, per, where)


# where an entry's rotation over the kinds starts: one kind later per entry -- but the Jacobians start at the QCQP, which puts
# the QP at N = 34: the box kinds' 3N columns leave room for one wave per workgroup there, the QP's slice for three
START = {entry: e for e, entry in enumerate(ENTRIES)}
START["jac"] = 1


def _matrix():
    rows = []
    for entry in ENTRIES:
        flagged = set()
        for w, (T, N) in enumerate(WIDTHS):
            kind = K4[(w + START[entry]) % 4]
            if entry == "polish" and T == 32:
                assert kind != "qcqp"
                N = 19                                   # ld = n | 1 = n
            flags = 0
            if kind in ("box", "sbox") and kind not in flagged:
                flagged.add(kind)
                flags = F_INF
            rows.append(_row(entry, kind, N, flags))
    return rows


ROWS = tuple(_matrix() + [
    _row("polish_ls", "qcqp", 12, reg=REG),              # the damped polish's run-time weight
    _row("jac_reg", "sbox", 20),
    _row("jac", "box", 8),                               # wpb = 3
])

# rows whose first seed missed a condition of check_heterogeneous: row_id -> the builders' `seed`
SEED = {}


def row_id(row):
    entry, kind, N, B, flags, reg = row[:6]
    return "%s-%s-N%d-B%d%s%s" % (entry, kind, N, B, "-inf" if flags & F_INF else "", "-reg" if reg else "")


def row_seed(row):
    return SEED.get(row_id(row), 0)


def _writable(*arrays):
    return [np.array(a, dtype=np.float64, order="C") for a in arrays]


def _inside_point(kind, ex, N):
    """A point at least 0.05 inside every effective bound of one problem (contacts: 0.3 of the radius along the first axis)."""
    if kind == "qcqp":
        x = np.zeros(N)
        x[0::2] = 0.3 * ex[0] * ex[1]
        return x
    lo, hi = R.effective_bounds(kind, ex, N)
    assert (hi - lo >= 0.1).all()
    flo, fhi = np.isfinite(lo), np.isfinite(hi)
    return np.where(flo & fhi, 0.5 * (np.where(flo, lo, 0.0) + np.where(fhi, hi, 0.0)),
                    np.where(flo, np.where(flo, lo, 0.0) + 0.5, np.where(fhi, np.where(fhi, hi, 0.0) - 0.5, 0.0)))


def _open_bounds(kind, ex, b):
    """Problem b's bounds made to hold 0 strictly (finite sides moved outwards by 0.1, a zero v made 1), its radii 1."""
    if kind == "qcqp":
        ex[0][b] = 1.0
        ex[1][b] = 1.0
    elif kind in ("box", "sbox"):
        ex[0][b] = -np.abs(ex[0][b]) - 0.1
        ex[1][b] = np.abs(ex[1][b]) + 0.1
        if kind == "sbox":
            ex[2][b] = np.where(ex[2][b] == 0.0, 1.0, ex[2][b])


@functools.lru_cache(maxsize=None)
def make_base(row):
    """The clean base of a row -> dict of read-only numpy arrays: P (nb,N,N), q, x (nb,N), ex (tuple of (nb,.)), g (nb,N) (the
    backward's cotangent), tan ((dP, dq[, da, db]): the JVP's tangents).  x: the polish's start, or the point the derivatives,
    Jacobians and active set are taken at."""
    entry, kind, N, _, flags, reg = row[:6]
    nb, seed, fam = base_size(N), row_seed(row), family(entry)
    tan = g = None
    if flags & F_INF:               # inf_bounds_cases: one-sided boxes, x not a solution
        import inf_bounds_cases as IB
        P, q, ex, x, g, tan = IB.problem(kind, nb, N, "dense", seed)
    elif fam == "polish_ls":        # cold starts x = PI(0)
        import polish_ls_cases as PLS
        P, q, ex, x = PLS.problem(kind, N, nb, "dense", seed)
    elif reg:                       # a singular free block; the polish starts beside the solution (tests/test_gpu_reg.py: problem)
        import reg_cases as RC
        d = RC.batch(kind, N, "lowrank", nb)
        P, q, ex, x = d["P"], d["q"], d["ex"], d["x"]
        if fam == "polish":
            x = np.stack([R.project(kind, x[b] + 1e-3 * np.sin(np.arange(N) + b), tuple(e[b] for e in ex), N) for b in range(nb)])
        tan, g = RC.inputs(kind, N, nb, seed)
    elif fam == "active":           # feasible, not a solution: z on either side of every bound
        import active_cases as AC
        P, q, ex, x = AC.random_problem(kind, nb, N, "dense", seed)
    else:                           # well-conditioned P, the oracle's forward at eps = 1e-3; the derivatives at its polished x
        import newton_cases as NC
        import polish_cases as PC
        d, x0 = PC.problem(kind, N, nb, "dense")
        P, q, ex = PC.flat(d, kind)
        x = x0[:, :, 0]
        if fam != "polish":
            x = PC.host_polish(kind, P, q, ex, x)[0]
            tan, g = NC.inputs(kind, N, nb, "dense", seed)
    P, q, x = _writable(P, q, x)
    ex = tuple(_writable(*ex))
    _open_bounds(kind, ex, INSIDE)
    if is_polish(entry):
        q[INSIDE] = 0.0             # r = 0 at x = 0: no step
        x[INSIDE] = 0.0
    else:
        ex0 = tuple(e[INSIDE] for e in ex)
        x[INSIDE] = _inside_point(kind, ex0, N)
        q[INSIDE] = -(P[INSIDE] @ x[INSIDE])          # z = x - (P x + q) is x to rounding
        ex3 = tuple(e[ACTIVE] for e in ex)
        if kind == "qcqp":
            x[ACTIVE] = 0.0
            x[ACTIVE, 0::2] = ex3[0] * ex3[1]         # on the rim, z far outside
            q[ACTIVE] = 0.0
            q[ACTIVE, 0::2] = -100.0
        else:
            lo, hi = R.effective_bounds(kind, ex3, N)
            down = np.isfinite(lo)
            up = ~down & np.isfinite(hi)
            x[ACTIVE] = np.where(down, np.where(down, lo, 0.0), np.where(up, np.where(up, hi, 0.0), 0.0))
            q[ACTIVE] = np.where(down, 100.0, np.where(up, -100.0, 0.0))
    out = {"P": P, "q": q, "ex": ex, "x": x}
    if entry.startswith("bwd"):
        out["g"] = _writable(g)[0]
    if entry.startswith("jvp"):
        out["tan"] = tuple(_writable(*tan[:2 if kind == "qp" else 4]))
    for a in [P, q, x] + list(ex) + [out.get("g")] + list(out.get("tan", ())):
        if a is not None:
            a.setflags(write=False)
    return out


def poison_plan(row):
    """problem -> the status the header documents for it on the poisoned base (include/diffqcqp_hip.h: 2 not finite; 1 a zero
    pivot -- the polish: no step accepted)."""
    plan = {POISON_NAN: 2, POISON_INF: 2}
    if not row[5] and family(row[0]) != "active":
        plan[POISON_SINGULAR] = 1
    return plan


def poisoned(row):
    """make_base(row) with the poisoned problems in place (module docstring) -> dict as make_base's, fresh arrays."""
    import reg_cases as RC
    entry, kind, N = row[:3]
    base = make_base(row)
    out = {k: (tuple(np.array(a) for a in v) if isinstance(v, tuple) else np.array(v)) for k, v in base.items()}
    out["x"][POISON_NAN, N // 2] = float("nan")
    out["P"][POISON_INF, 0, 0] = float("inf")
    if POISON_SINGULAR in poison_plan(row):
        b, ex = POISON_SINGULAR, out["ex"]
        out["P"][b] = RC.batch(kind, N, "duprow")["P"][b]         # an exactly duplicated row and column
        if kind == "qcqp":
            ex[0][b] = 1.0
            ex[1][b] = 1.0
        elif kind in ("box", "sbox"):
            ex[0][b] = -1.0
            ex[1][b] = 1.0
            if kind == "sbox":
                ex[2][b] = 1.0
        xin = _inside_point(kind, tuple(e[b] for e in ex), N)
        out["x"][b] = xin
        out["q"][b] = -(out["P"][b] @ xin) + 0.01                   # z = x - 0.01: every coordinate free, r = 0.01
    return out


def host(row, base, max_steps=None):
    """The entry's one-thread host core on a base (make_base's or poisoned()'s dict) -> dict name -> array, named and shaped
    as tests/test_gpu_newton_trips.py names the device's outputs."""
    entry, kind, N, _, flags, reg = row[:6]
    inf, fam = bool(flags & F_INF), family(entry)
    P, q, ex, x = base["P"], base["q"], base["ex"], base["x"]
    plain = not inf and not reg
    if fam == "polish":
        steps = MAX_STEPS["polish"] if max_steps is None else max_steps
        if plain:
            import polish_cases as PC
            r = PC.host_polish(kind, P, q, ex, x, steps)
        else:
            import reg_cases as RC
            r = RC.host_polish(kind, P, q, ex, x, steps, reg, False, inf)
        return dict(zip(("x_out", "resid", "steps", "status"), r))
    if fam == "polish_ls":
        import polish_ls_cases as PLS
        steps = MAX_STEPS["polish_ls"] if max_steps is None else max_steps
        r = PLS.host_polish_ls(kind, P, q, ex, x, steps, MAX_HALVINGS, reg, inf_ok=inf)
        return dict(zip(("x_out", "resid", "steps", "status", "halvings"), r))
    if fam == "active":
        import active_cases as AC
        return dict(zip(("state", "mult", "margin", "where", "status"), AC.host_active(kind, P, q, ex, x, flag=inf)))
    import jac_cases as JC
    import newton_cases as NC
    import reg_cases as RC
    if fam == "jac":
        r = JC.host_jac(kind, P, q, ex, x) if plain else RC.host_jacobian(kind, P, q, ex, x, reg, False, inf)
        names = ("Jq", "Ja", "Jb", "status")
    elif entry.startswith("jvp"):
        r = NC.host_jvp(kind, P, q, ex, x, base["tan"]) if plain else RC.host_jvp(kind, P, q, ex, x, base["tan"], reg, False, inf)
        names = ("dx", "status")
    else:
        r = NC.host_backward(kind, P, q, ex, x, base["g"]) if plain else RC.host_backward(kind, P, q, ex, x, base["g"], reg, False, inf)
        names = ("grad_P", "grad_q", "grad_a", "grad_b", "status")
    return {n: v for n, v in zip(names, r) if v is not None}


@functools.lru_cache(maxsize=None)
def reference(row):
    """The host core on the row's clean base, once per session."""
    return host(row, make_base(row))


def active_sizes(row):
    """Per problem of the clean base: the elements the Newton kernels treat as active (active_cases.host_active: state != 0)."""
    import active_cases as AC
    base = make_base(row)
    st = AC.host_active(row[1], base["P"], base["q"], base["ex"], base["x"], flag=bool(row[4] & F_INF))
    assert not st[4].any(), row_id(row)
    return (st[0] != 0).sum(1)


def check_heterogeneous(row):
    entry, kind, N = row[:3]
    ref = reference(row)
    st = ref["status"]
    if is_polish(entry):
        steps = ref["steps"]
        assert not (st == 2).any() and ((steps > 0) == (st == 0)).all(), (row_id(row), st, steps)
        assert steps[INSIDE] == 0 and (steps >= 2).any(), (row_id(row), steps)
        assert (ref["resid"][:, 1] <= ref["resid"][:, 0]).all()
        if family(entry) == "polish_ls":
            h = ref["halvings"]
            assert (h == 0).any() and (h > 0).any(), (row_id(row), h)
    else:
        assert not st.any(), (row_id(row), st)
        na = active_sizes(row)
        if kind == "qcqp":
            assert (na == 0).any() and (na > 0).any(), (row_id(row), na)
        else:
            assert (na == 0).any() and (na >= (N + 1) // 2).any(), (row_id(row), na)
    return ref
