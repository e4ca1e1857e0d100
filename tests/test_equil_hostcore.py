"""The power-of-two equilibration on the CPU: diffqcqp_amd/csrc/equil_core.h compiled for the host
(tests/hostcore/equil_core_check.cpp) against the numpy restatement tests/equil_ref.py, bit for bit in the exponents and in
every scaled array; the rule itself against properties that do not go through either (the scaled diagonal's interval, the
even neighbour at a tie, hand-computed rows); the round trip; the QCQP's shared exponents; infinite bounds."""
import numpy as np
import pytest

import equil_ref as R

B = 5
NS = (1, 2, 3, 8, 17, 64, 65) + R.CHUNKED_N
CASES = [(k, N, d) for k in R.KINDS for N in NS for d in (False, True)
         if not (k == "qcqp" and N % 2) and not (d and N not in R.FAST_N)]


@pytest.fixture(scope="module")
def core():
    return R.hostcore()


@pytest.mark.parametrize("kind,N,diag", CASES)
def test_host_core_equals_the_restatement(core, kind, N, diag):
    P, q, extras, x0 = R.make_batch(kind, B, N, 11 * N + R.KIND_ID[kind], diag)
    want = R.equilibrate(kind, P, q, extras, x0, diag)
    got = R.host_equilibrate(core, kind, P, q, extras, x0, diag)
    assert R.same_problem(got, want) is None
    assert R.same_problem(R.host_equilibrate(core, kind, P, q, extras, None, diag)[:3], want[:3]) is None   # without x0
    e = want[4]
    assert N < 8 or e.min() < 0 < e.max(), "the batch must need scaling both ways"
    if kind == "qcqp":
        assert np.array_equal(e[:, 0::2], e[:, 1::2])
    for lo, lo_t in zip(extras[:2], want[2][:2]):     # an infinite bound passes through
        inf = np.isinf(lo)
        assert np.array_equal(lo[inf], lo_t[inf])
    if kind in ("box", "sbox"):
        assert N < 8 or (np.isinf(extras[0]).any() and np.isinf(extras[1]).any())
    if kind == "sbox":
        assert R.same_bits(want[2][2], extras[2])
    if kind == "qcqp":
        assert R.same_bits(want[2][1], extras[1])


def test_the_batches_hold_every_special_entry():
    """make_batch cycles SPECIAL over the diagonals: together the batches above must have held every entry."""
    seen = set()
    for kind, N, diag in CASES:
        P = R.make_batch(kind, B, N, 11 * N + R.KIND_ID[kind], diag)[0]
        d = P if diag else np.diagonal(P, axis1=1, axis2=2)
        seen |= set(d.ravel().view(np.uint64).tolist())
    missing = [v for v in R.SPECIAL if not np.isnan(v) and np.float64(v).view(np.uint64) not in seen]
    assert not missing, missing
    assert any(np.isnan(np.array(list(seen), dtype=np.uint64).view(np.float64)))


def test_the_rule_on_every_special_entry(core):
    p = R.SPECIAL
    e = R.host_exponents(core, p)
    assert np.array_equal(e, R.exponents("qp", p[None, :])[0])
    # hand-computed rows of equil_core.h's table
    table = {1.0: 0, 2.0: 0, 0.5: 0, 4.0: -1, 8.0: -2, 0.125: 2, 3.0: -1, 2.0 ** 40: -20, 2.0 ** -40: 20, 2.0 ** 600: -255,
             2.0 ** -600: 255, 5e-324: 255, 0.0: 0, -1.0: 0, 2.0 ** 510: -255, 2.0 ** 511: -255, 2.0 ** -510: 255, 2.0 ** -511: 255,
             32.0: -2, 1.0 / 32: 2, 2.0 ** 7: -4, 2.0 ** -7: 4}
    for v, want in table.items():
        assert e[np.flatnonzero(p == v)[0]] == want, v
    assert (e[~(p > 0) | np.isinf(p)] == 0).all()                # <= 0, NaN, infinite
    assert np.abs(e).max() == R.MAX_EXP
    # the definition, without frexp: where nothing is clamped the scaled entry lies in [1/2, 2], strictly inside unless the
    # entry is an odd power of two -- there the exponent chosen is the even one of the two nearest
    ok = (p > 0) & np.isfinite(p) & (np.abs(e) < R.MAX_EXP)
    pt = p[ok] * 4.0 ** e[ok]
    assert ((pt >= 0.5) & (pt <= 2.0)).all()
    edge = (pt == 0.5) | (pt == 2.0)
    assert edge.sum() >= 8 and (e[ok][edge] % 2 == 0).all()
    # a mantissa of sqrt(1/2) is no boundary: its neighbours and it share an exponent
    s = np.sqrt(0.5)
    for k in range(-7, 8):
        v = s * 2.0 ** k
        tri = R.host_exponents(core, np.array([np.nextafter(v, 0.0), v, np.nextafter(v, np.inf)]))
        assert tri[0] == tri[1] == tri[2] == -(k // 2), (k, tri)
    # ... and a power of two is one exactly when it is odd: below it the smaller exponent's neighbour, above it the larger's
    for k in range(-7, 8):
        v = 2.0 ** k
        lo, at, hi = R.host_exponents(core, np.array([np.nextafter(v, 0.0), v, np.nextafter(v, np.inf)]))
        if k % 2 == 0:
            assert lo == at == hi == -(k // 2)
        else:
            assert lo == -((k - 1) // 2) and hi == -((k + 1) // 2) and at in (lo, hi) and at % 2 == 0, (k, lo, at, hi)


def test_round_trip(core):
    r = np.random.default_rng(5)
    n = 4096
    x = np.ldexp(r.uniform(0.5, 1.0, n), r.integers(-299, 301, n)) * r.choice([-1.0, 1.0], n)
    x[:4] = [2.0 ** -300, -2.0 ** -300, 2.0 ** 300, -2.0 ** 300]
    e = r.integers(-R.MAX_EXP, R.MAX_EXP + 1, n).astype(np.int32)
    e[:4] = [R.MAX_EXP, -R.MAX_EXP, R.MAX_EXP, -R.MAX_EXP]
    y = np.ldexp(x, -e)
    assert R.same_bits(R.host_unscale(core, y, e), x) and R.same_bits(R.unscale(y, e), x)


@pytest.mark.parametrize("kind", R.KINDS)
def test_scaled_problem_is_the_problem_in_other_units(kind):
    """On a batch without special entries nothing rounds: D^-1 P~ D^-1, D^-1 q~ and D l~ give the inputs back bit for bit, and the
    scaled diagonal lies in [1/2, 2]."""
    P, q, extras, x0 = R.make_batch(kind, B, 8, 77, special=False)
    Pt, qt, ext, x0t, e = R.equilibrate(kind, P, q, extras, x0)
    d = np.diagonal(Pt, axis1=1, axis2=2)
    if kind == "qcqp":   # a contact's exponent is its larger entry's: that one lies in the interval, the other below it
        d = np.maximum(d[:, 0::2], d[:, 1::2])
    assert ((d >= 0.5) & (d <= 2.0)).all()
    assert R.same_bits(np.ldexp(Pt, -(e[:, :, None] + e[:, None, :])), P) and R.same_bits(np.ldexp(qt, -e), q)
    assert R.same_bits(R.unscale(x0t, e), x0)
    eb = e[:, 0::2] if kind == "qcqp" else e
    for a, at in zip(extras[:2 if kind != "qcqp" else 1], ext):
        assert R.same_bits(np.ldexp(at, eb), a)


def test_entry_argument_checks():
    """dqq_equilibrate_f64 / dqq_unscale_f64 refuse what the header says, in its order, before anything touches a GPU."""
    from diffqcqp_amd import build, _capi
    build.build()
    lib = _capi.ctypes_lib()
    f, u = lib.dqq_equilibrate_f64, lib.dqq_unscale_f64
    B, N = 4, 8
    P, q, a, b, c, x0 = (0x10000 * (i + 1) for i in range(6))          # never dereferenced: the checks fail first
    Po, qo, ao, bo, co, xo, eo = (0x100000 * (i + 1) for i in range(7))
    assert f(7, P, q, None, None, None, None, B, N, 1, Po, qo, None, None, None, None, eo, None) == -7
    assert f(0, P, q, None, None, None, None, -1, N, 1, Po, qo, None, None, None, None, eo, None) == -2
    assert f(1, P, q, a, b, None, None, B, 7, 1, Po, qo, ao, None, None, None, eo, None) == -2      # a QCQP of odd N
    assert f(0, P, q, None, None, None, None, B, N, 7, Po, qo, None, None, None, None, eo, None) == -4
    assert f(0, None, None, None, None, None, None, 0, N, 1, None, None, None, None, None, None, None, None) == 0   # B = 0
    assert f(0, P, q, None, None, None, None, B, N, 1, Po, qo, None, None, None, None, None, None) == -1   # e_out
    assert f(0, P, q, None, None, None, None, B, N, 1, Po, qo, ao, None, None, None, eo, None) == -1       # the QP has no extras
    assert f(2, P, q, None, b, None, None, B, N, 1, Po, qo, ao, bo, None, None, eo, None) == -1            # a_out without a
    assert f(0, P, q, None, None, None, None, B, N, 1, Po, qo, None, None, None, xo, eo, None) == -1       # x0_out without x0
    assert f(0, P, q, None, None, None, None, B, 6, 2, Po, qo, None, None, None, None, eo, None) == -3     # DQQ_P_DIAG, N = 6
    assert f(0, P, q, None, None, None, None, B, N, 1, P, qo, None, None, None, None, eo, None) == -4      # P_out is P
    assert f(0, P, q, None, None, None, None, B, N, 1, Po, P + 8 * (B * N * N - 1), None, None, None, None, eo, None) == -4
    assert f(2, P, q, a, b, None, x0, B, N, 1, Po, qo, ao, bo, None, a, eo, None) == -4                    # x0_out is l_min
    assert u(P, eo, -1, N, Po, None) == -2 and u(P, eo, 0, N, Po, None) == 0 and u(None, eo, B, N, Po, None) == -1
    assert u(P, None, B, N, Po, None) == -1 and u(P, eo, B, N, None, None) == -1
