"""CPU check of tests/footprint_cases.py and tests/footprint_arena.py, what tests/test_gpu_footprint.py stands on: every
case's plan from the shipped route.cpp is the route the table names; the tile sizes in the table are the launch geometry
(launch_g); the cases reach every kernel family with a batch that ends inside a tile and one below a tile -- or no such batch
exists, which is proved here by scanning the plans; and the arena's checks fail when a "kernel" (plain torch on a CPU arena)
writes past or before a payload, leaves the last problem unwritten or changes an input."""
import pytest
import torch

from footprint_arena import Arena, F64, I32, U8, call_specs, ws_guard
from footprint_cases import CASES, EXTRA_GROUPS, GROUPS, NO_B_BELOW_G, ZERO, case_g, case_id, launch_g, launches
from param_cases import BWD, BWD_FAMILIES, FWD, FWD_FAMILIES, KIND, families
from test_routes import AUTO, DENSE, DIAG, REF, XD, XL, _build, raw_plan, render


@pytest.fixture(scope="module")
def shipped():
    return _build(False)


@pytest.fixture(scope="module")
def lib():
    from diffqcqp_amd import build, _capi
    build.build()
    return _capi.ctypes_lib()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_case_takes_its_route(shipped, case):
    pas, kind, N, B, layout, _, want = case
    assert render(raw_plan(shipped, pas, KIND[kind], N, B, layout)) == want


def test_tile_sizes_are_the_launch_geometry():
    for pas, kinds, N, Bs, layout, structure, route, g, src, gd, srcd, below in GROUPS + EXTRA_GROUPS:
        ls = launches(route)
        for kind in kinds:
            assert launch_g(ls[0], kind, N) == (g, src), (route, kind, N)
            assert (launch_g(ls[1], kind, N) if len(ls) > 1 else (None, None)) == (gd, srcd), (route, kind, N)
    # what the launchers say, spelled out once per family
    assert [launch_g("fdiag/%d" % l, "qp", 8)[0] for l in (1, 2, 4, 8, 16, 32)] == [256, 128, 64, 32, 16, 8]
    assert [launch_g("bdiag", "qp", n)[0] for n in (2, 4, 8, 16, 32, 64)] == [256, 128, 64, 32, 16, 8]
    assert launch_g("flane", "qp", 8)[0] == 64 and launch_g("blane/m1", "qcqp", 8)[0] == 64 and launch_g("fsmall", "qp", 12)[0] == 16
    assert launch_g("bsmall", "qp", 8)[0] == 32 and launch_g("bsmall", "qcqp", 8)[0] == 20 and launch_g("bsmall", "box", 2)[0] == 40
    assert launch_g("flds", "qp", 5)[0] == 4 and launch_g("flds", "qp", 32)[0] == 3 and launch_g("flds", "qp", 64)[0] == 1
    assert launch_g("bteam", "qp", 5)[0] == 32 and launch_g("bteam", "box", 8)[0] == 4 and launch_g("bteam", "box", 16)[0] == 1


def test_every_row_of_param_cases_has_a_group():
    have = {(g[0], k, g[2], g[4], g[5], g[6]) for g in GROUPS for k in g[1]}
    for pas, kind, N, B, layout, structure, route in FWD + BWD:
        assert (pas, kind, N, layout, structure, route) in have, (pas, kind, N, layout, route)
    kinds = {(c[0], c[1]) for c in ZERO}
    assert kinds == {(0, k) for k in ("qp", "qcqp", "box", "sbox")} | {(1, k) for k in ("qp", "qcqp", "box")}


def _drain_len(case):
    """The problems a case's first launch leaves on the work-list, which is what its drain launch covers.  A wave of the fast
    kernels pushes its whole tile, one entry per problem, when any problem of the tile has a non-diagonal P (fwd_diag.hip:187,
    bwd_diag.hip:162; a wave's tile: a quarter of the workgroup's g); problem b of a 'mixed' batch is non-diagonal when
    b % 3 == 1 (conftest.make_problem), no problem of a 'diag' batch is."""
    B, structure = case[3], case[5]
    if structure != "mixed":
        return B if structure == "dense" else 0
    T = case_g(case)[0] // 4
    return sum(min(T, B - f) for f in range(0, B, T) if any(b % 3 == 1 for b in range(f, min(f + T, B))))


def _launch_gs(case):
    """[(family tags of a launch, its g, the problems it covers)] of a case: B for the first launch, the work-list's for a
    drain."""
    pas, kind, N, B, layout, _, route = case
    g, gd = case_g(case)
    ls = launches(route)
    out = []
    for i, l in enumerate(ls):
        parts = l.split("/")
        if parts[0] == "fdiag":
            tags = {"fdiag/" + parts[1], "fdiag + drain" if len(ls) > 1 else "fdiag alone"}
        elif parts[0] == "blane":
            tags = {"blane/" + parts[1]}
        else:
            tags = {parts[0]}
        out.append((tags, g if i == 0 else gd, B if i == 0 else _drain_len(case)))
    assert set().union(*(t for t, _, _ in out)) == families(route)
    return out


def test_cases_cover_every_family_at_the_tile_edges(shipped):
    ragged, below, whole = set(), set(), set()
    for case in CASES:
        if case[3] == 0:
            continue
        for tags, g, n in _launch_gs(case):
            whole |= tags
            if n == 0:               # a drain of an empty list covers nothing
                continue
            if g == 1:               # one problem per workgroup: no partial tile, no B below it
                ragged |= tags
                below |= tags
                continue
            if n % g:
                ragged |= tags
            if n < g:
                below |= tags
    every = set(FWD_FAMILIES) | set(BWD_FAMILIES)
    assert whole == every, every - whole
    assert ragged == every, "families without a batch that ends inside a tile: %s" % sorted(every - ragged)
    assert every - below == set(NO_B_BELOW_G), "families without a B < g: %s" % sorted(every - below)
    # the claim of NO_B_BELOW_G (and of the groups marked "none: ..."): no plan of a B < g launches them
    for pas, kinds in ((0, ("qp", "qcqp", "box", "sbox")), (1, ("qp", "qcqp", "box"))):
        for kind in kinds:
            for N in list(range(1, 73)) + [96, 128]:
                for layout in (AUTO, DENSE, DIAG):
                    for flags in (0, REF, XD, XL, XD | XL, XD | REF):
                        for B in range(1, 64):
                            got = families(render(raw_plan(shipped, pas, KIND[kind], N, B, layout | flags)))
                            assert not (got & set(NO_B_BELOW_G)), (pas, kind, N, B, layout | flags)
    for pas, kinds, N, Bs, layout, structure, route, g, src, gd, srcd, note in GROUPS + EXTRA_GROUPS:
        if note != "yes":
            assert note == "none: the route starts at B = %d" % Bs[0]
            for kind in kinds:
                for B in range(1, max(g, gd or 0)):
                    assert render(raw_plan(shipped, pas, KIND[kind], N, B, layout)) != route
                assert render(raw_plan(shipped, pas, KIND[kind], N, Bs[0] - 1, layout)) != route


# ---------------------------------------------------------------- the arena's checks can fail
def _cpu_arena(B=5, N=3, g=4, sliced=True):
    q = torch.arange(B * N, dtype=F64).reshape(B, N, 1)
    specs = [("q", "in", F64, (B, N, 1), q), ("x", "out", F64, (B, N, 1), None), ("iters", "out", I32, (B,), None),
             ("flags", "out", U8, (B,), None), ("ws", "ws", U8, (1024, 256), None)]
    return Arena(specs, g, "cpu", sliced=sliced)


def _good_kernel(a, B=5):
    a.view("x").copy_(2 * a.view("q"))
    a.view("iters").fill_(7)
    a.view("flags").fill_(1)
    a.view("ws")[:64].fill_(3)


def _all_checks(a):
    a.check_guards()
    a.check_inputs()
    for name in ("x", "iters", "flags"):
        a.check_written(name)


@pytest.mark.parametrize("sliced", [True, False])
def test_arena_layout_and_a_correct_kernel_passes(sliced):
    a = _cpu_arena(sliced=sliced)
    for name, per in (("q", 24), ("x", 24), ("iters", 4), ("flags", 1)):
        b = a.bufs[name]
        assert b["off"] % 512 == (per if sliced else 0) and b["guard"] >= 4096 and b["guard"] >= 2 * 4 * per
    assert a.bufs["ws"]["off"] % 512 == 0 and a.bufs["ws"]["nbytes"] == 1024
    assert not a.view("ws")[:256].any() and bool((a.view("ws")[256:].view(torch.int64) == 0x7FF8DEADBEEFCAFE).all())
    assert torch.isnan(a.view("x")).all()
    _good_kernel(a)
    _all_checks(a)
    with pytest.raises(AssertionError, match="arena modified"):
        a.check_untouched()
    _cpu_arena().check_untouched()


def test_guard_sizes_follow_g_and_the_bytes_per_problem():
    d = {"P": torch.zeros(3, 8, 8, dtype=F64), "q": torch.zeros(3, 8, 1, dtype=F64)}
    a = Arena(call_specs(0, "qp", 8, 3, 0, d, 2048, 1024), 256, "cpu")
    assert a.bufs["P"]["guard"] == 2 * 256 * 512 and a.bufs["iters"]["guard"] == 4096
    names = a.order
    for prev, name in zip(names, names[1:]):   # the gap holds the larger of the two guards that meet in it
        gap = a.bufs[name]["off"] - a.bufs[prev]["hi"]
        assert gap >= max(a.bufs[prev]["guard"], a.bufs[name]["guard"]), (prev, name)
    assert a.total - a.bufs["ws"]["hi"] >= 4096 + 2 * 256 * 4 and a.bufs[names[0]]["off"] >= a.bufs[names[0]]["guard"]
    # a workspace with scratch: the whole scratch, or two slices if that is more, and a tile of entries -- on both sides
    for scratch, piece in ((90000, 30000), (30000, 30000)):
        a = Arena(call_specs(0, "qp", 8, 3, 0, d, 1024 + scratch, 1024, piece), 256, "cpu")
        ws = a.bufs["ws"]
        assert ws["guard"] >= max(scratch, 2 * piece) + 2 * 256 * 4 and ws["nbytes"] == 1024 + scratch
        assert a.total - ws["hi"] >= ws["guard"] and ws["off"] - a.bufs[a.order[-2]]["hi"] >= ws["guard"]


def test_the_workspace_guards_of_the_scratch_cases_hold_the_scratch(lib):
    """The cases on the global-memory kernels: the scratch is whole slices, one per workgroup (general_any.hip any_grid: B
    workgroups up to 512), and the guards around the workspace hold all of it, twice one slice, and a tile of entries."""
    seen = 0
    for case in CASES:
        pas, kind, N, B, layout, _, route = case
        scratch = lib.dqq_scratch_bytes(KIND[kind], pas, N, B, layout)
        assert (scratch > 0) == (" scr" in route), case_id(case)
        if not scratch:
            continue
        seen += 1
        piece = lib.dqq_scratch_bytes(KIND[kind], pas, N, 1, layout)
        assert piece > 0 and scratch == piece * min(B, 512), case_id(case)
        g = max(g for g in case_g(case) if g)
        worklist = lib.dqq_workspace_bytes(B)
        guard = ws_guard(worklist + scratch, worklist, piece, g)
        assert guard >= scratch + 2 * g * 4 and guard >= 2 * piece + 2 * g * 4
    assert seen >= 3


def test_a_write_one_element_past_a_payload_is_found():
    a = _cpu_arena()
    _good_kernel(a)
    a.window("x", after=1)[-1] = 1.0
    with pytest.raises(AssertionError, match=r"guard behind 'x' overwritten: byte [0-7] past the end"):
        a.check_guards()
    a = _cpu_arena()
    _good_kernel(a)
    a.window("flags", after=1)[-1] = 2
    with pytest.raises(AssertionError, match=r"guard behind 'flags' overwritten: byte 0 past"):
        a.check_guards()
    a = _cpu_arena()
    _good_kernel(a)
    a.window("ws", after=1)[-1] = 0          # the exactly-sized workspace
    with pytest.raises(AssertionError, match=r"guard behind 'ws' overwritten: byte 0 past"):
        a.check_guards()


def test_a_write_one_element_before_a_payload_is_found():
    a = _cpu_arena()
    _good_kernel(a)
    a.window("iters", before=1)[0] = 12
    with pytest.raises(AssertionError, match=r"guard in front of 'iters' overwritten: byte [1-4] before"):
        a.check_guards()
    a = _cpu_arena()
    _good_kernel(a)
    a.window("q", before=1)[0] = 0.5         # the first buffer of the arena
    with pytest.raises(AssertionError, match=r"guard in front of 'q' overwritten: byte [1-8] before"):
        a.check_guards()


def test_an_unwritten_last_problem_is_found():
    a = _cpu_arena()
    _good_kernel(a)
    a.view("x")[:4].copy_(torch.full((4, 3, 1), float("nan")))   # an ordinary NaN is a written value ...
    _all_checks(a)
    a = _cpu_arena()
    a.view("x")[:4].copy_(2 * a.view("q")[:4])                   # ... what the arena was filled with is not
    a.view("iters").fill_(7)
    a.view("flags").fill_(1)
    with pytest.raises(AssertionError, match=r"output 'x' not written: problem 4 of 5, element 0 \(offset 12\)"):
        a.check_written("x")
    a.check_written("x", rows=torch.tensor([True, True, True, True, False]))
    a.view("x").copy_(2 * a.view("q"))
    a.view("iters")[4] = 0x7F5A5A5A
    with pytest.raises(AssertionError, match=r"output 'iters' not written: problem 4 of 5, element 0 \(offset 4\)"):
        a.check_written("iters")
    a.view("iters")[4] = 3
    a.view("flags")[4] = 0xA5
    with pytest.raises(AssertionError, match=r"output 'flags' not written: problem 4 of 5"):
        a.check_written("flags")


def test_a_modified_input_is_found():
    a = _cpu_arena()
    _good_kernel(a)
    a.view("q")[2, 1, 0] += 1.0
    a.check_guards()
    with pytest.raises(AssertionError, match=r"input 'q' modified at byte offset (5[6-9]|6[0-3]) \(element 7\)"):
        a.check_inputs()


# ---------------------------------------------------------------- the JVP's arena (tests/test_gpu_jvp_footprint.py)
def _jvp_arena(kind="box", N=22, B=5, worklist=1024, scratch=5 * 4000, piece=4000, g=1):
    from footprint_arena import jvp_call_specs
    gen = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=F64)   # noqa: E731
    e = (B, N // 2, 1) if kind == "qcqp" else (B, N, 1)
    d = {"P": r(B, N, N), "q": r(B, N, 1), "x": r(B, N, 1), "dP": r(B, N, N), "dq": r(B, N, 1), "da": r(*e), "db": r(*e)}
    d.update({n: r(*e) for n in ("l_n", "mu", "l_min", "l_max", "v")})
    return Arena(jvp_call_specs(kind, N, B, 1, d, worklist + scratch if scratch else 0, worklist, piece), g, "cpu")


def _jvp_good_kernel(a, steps=True):
    a.view("dx").copy_(a.view("q") + a.view("dq"))
    if steps:
        a.view("ir_steps").fill_(1)
    if "ws" in a.bufs:
        head = a.bufs["ws"]["shape"][1]
        a.view("ws")[head:].fill_(3)       # the scratch is the kernel's to write, the work-list in front is not


def test_the_jvp_arena_every_tangent_an_input_and_its_own_checks_can_fail():
    a = _jvp_arena()
    assert [n for n in a.order if a.bufs[n]["role"] == "in"] == ["P", "q", "l_min", "l_max", "x", "dP", "dq", "da", "db"]
    assert a.bufs["ir_steps"]["shape"] == (5, 2) and a.bufs["ws"]["guard"] >= 5 * 4000 + 8
    assert "ws" not in _jvp_arena(scratch=0).bufs and _jvp_arena("qp", 3, 37, scratch=0).bufs["dx"]["off"] % 512 == 24
    assert "da" not in _jvp_arena("qp", 3, 37, scratch=0).bufs
    _jvp_good_kernel(a)
    a.check_guards(); a.check_inputs(); a.check_written("dx"); a.check_written("ir_steps")   # noqa: E702
    a.check_pristine("ws", 1024)
    # a tangent that the kernel scribbles on is a modified input
    a.view("da")[4, 21, 0] = 0.0
    with pytest.raises(AssertionError, match="input 'da' modified"):
        a.check_inputs()
    # the work-list in front of the scratch is documented as not touched: one entry, even rewritten to zero's neighbour, shows
    a = _jvp_arena()
    _jvp_good_kernel(a)
    a.view("ws")[1020] = 1
    with pytest.raises(AssertionError, match="'ws' modified at byte offset 1020"):
        a.check_pristine("ws", 1024)
    # ir_steps = NULL: the buffer that was not handed over must stay as it was
    a = _jvp_arena()
    _jvp_good_kernel(a, steps=False)
    a.check_pristine("ir_steps")
    a.view("ir_steps")[4, 1] = 1
    with pytest.raises(AssertionError, match="'ir_steps' modified at byte offset 36"):
        a.check_pristine("ir_steps")
    # a scratch stride one slice short: the last workgroup's slice ends one slice past the workspace, inside the guard
    a = _jvp_arena()
    _jvp_good_kernel(a)
    a.window("ws", after=4000)[-4000:] = 3
    with pytest.raises(AssertionError, match="guard behind 'ws' overwritten: byte 0 past"):
        a.check_guards()
    # a dropped `valid` predicate: the ragged tile's idle lanes store past problem B - 1
    a = _jvp_arena("qcqp", 8, 67, scratch=0, g=64)
    _jvp_good_kernel(a)
    a.window("dx", after=8 * 61)[-8 * 61:] = 0.0     # problems 67 .. 127 of the second tile
    with pytest.raises(AssertionError, match="guard behind 'dx' overwritten: byte 0 past"):
        a.check_guards()


def test_the_jvp_footprint_rows_state_their_launchers_geometry():
    """g of tests/test_gpu_jvp_footprint.py's rows: JvpDiag is the diagonal backward's tile (4 waves of 128 / N problems),
    JvpTeam the backward's team geometry, JvpAny a problem per workgroup."""
    import test_gpu_jvp_footprint as T
    for family, kind, N, B, layout, structure, g in T.CASES:
        launch = {"diag": "bdiag", "team": "bteam", "any": "bany"}[family]
        assert g == launch_g(launch, "box" if kind == "sbox" else kind, N)[0], (family, kind, N)
        assert B % g != 0 or g == 1
