"""CPU proof that csrc/common.h: ExactDivisor -- division with the denominator's share of the work done once -- and the
QcqpContact built on it (csrc/kkt_core.h) change no bit.  tests/hostcore/exact_divisor_check.cpp, a program of its own built
with the host compiler, runs the DEVICE's text with models of the hardware's reciprocal estimate (the correctly rounded
reciprocal moved by -1, 0, +1 ulp; a float-precision one moved likewise) and compares
  * div(n, d) with n / d, bit for bit: 10^7 pairs log-uniform over every exponent, 10^7 more around the range the fast form
    certifies, every pair of a list of edge values, and 10^6 (numerator, denominator) pairs as QcqpContact::setup meets them
    on the benchmark's distribution (p ~ U(0.1, 1.1), l_n, mu ~ U(0, 1));
  * QcqpContact against the struct as it was before (kept verbatim in the program): every member after setup and after each
    of three steps, on 10^5 contacts of the benchmark's distribution and 10^5 with zeros, NaN and extreme scales.
Zero mismatches, no tolerance.  The counts of cases that took the fast form are checked too: a test that only ever ran the
plain division would prove nothing."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "diffqcqp_amd", "csrc")


@pytest.fixture(scope="module")
def results():
    src = os.path.join(HERE, "hostcore", "exact_divisor_check.cpp")
    exe = os.path.join(HERE, "hostcore", "exact_divisor_check")
    deps = [src] + [os.path.join(CSRC, f) for f in ("common.h", "kkt_core.h", "bwd_systems.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", exe + ".tmp", src])
        os.replace(exe + ".tmp", exe)
    r = subprocess.run([exe, "all"], capture_output=True, text=True, timeout=600)
    rows = {}
    for line in r.stdout.splitlines():
        w = line.split()
        if not line.startswith("#") and len(w) >= 2:
            rows[w[0]] = [int(v) for v in w[1:]]
    return r.returncode, r.stdout, rows


MODELS = 6   # seed models per pair (and, with the host's own divider, 7 builds of the struct per contact)


@pytest.mark.parametrize("name, pairs, fast_share", [("random_full_range", 10 ** 7, 0.05), ("random_around_the_certified_range", 10 ** 7, 0.3),
                                                     ("edge_values", 200 ** 2, 0.05), ("bench_kkt_pairs", 10 ** 6, 0.999)])
def test_div_returns_the_bits_of_the_plain_division(results, name, pairs, fast_share):
    rc, out, rows = results
    cases, fast, bad = rows[name]
    assert bad == 0, out[-2000:]
    assert cases >= MODELS * pairs, (name, cases)
    assert fast >= fast_share * cases, "the fast form was hardly exercised: %d of %d" % (fast, cases)


@pytest.mark.parametrize("name", ["bench_contacts", "odd_contacts"])
def test_contact_matches_the_struct_it_replaces(results, name):
    rc, out, rows = results
    cases, _, bad = rows[name]
    assert bad == 0, out[-2000:]
    assert cases == (MODELS + 1) * 10 ** 5
    share = rows[{"bench_contacts": "contact_active_share", "odd_contacts": "odd_contact_active_share"}[name]][0] / cases
    assert 0.25 < share < 0.75, "active and inactive contacts must both occur: %.2f active" % share


def test_the_program_reports_success(results):
    assert results[0] == 0, results[1][-2000:]
