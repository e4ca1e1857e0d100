#!/usr/bin/env python3
"""Is the device code of two source trees the same?  CPU only (hipcc -S cross-compiles).

    python tools/device_code_diff.py <tree A> <tree B> [-j N] [unit.hip ...]

Every .hip unit of each tree's diffqcqp_amd/build.py: UNITS is compiled to a gfx950 listing with that tree's flags (device
code only, as tests/test_isa_guard.py: listing does), once as shipped and once with -DDQQ_TUNING.  Each listing is split by
function symbol; the per-function number in local labels (.LBB<k>_<m>, .Lfunc_end<k>) is normalised away.  Reported:
symbols on one side only, symbols whose instruction lines differ, symbols whose resource lines differ (registers, scratch,
LDS, occupancy, the kernel descriptor).  One summary line per unit and build; exit status 1 on any difference.  Text is
compared, no instruction is looked for; a kernel whose LDS or occupancy line is not found ends the run.  Listings are
cached in /tmp by the tree's build.source_sha16(), the compiler's version and the command line."""
import argparse
import difflib
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor


def load_build(tree):
    path = os.path.join(os.path.abspath(tree), "diffqcqp_amd", "build.py")
    spec = importlib.util.spec_from_file_location("dqq_build_" + hashlib.sha256(path.encode()).hexdigest()[:8], path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def listing(build, unit, tuning):
    cmd = [build._hipcc()] + build.COMMON + build.UNITS[unit] + (["-DDQQ_TUNING"] if tuning else []) + [
        "-I", build.INCLUDE, "-S", "--cuda-device-only", os.path.join(build.CSRC, unit)]
    if not hasattr(build, "compiler"):
        build.compiler = subprocess.run([cmd[0], "--version"], capture_output=True, text=True).stdout
    tag = hashlib.sha256((build.source_sha16() + build.compiler + " ".join(cmd)).encode()).hexdigest()[:16]
    path = "/tmp/dqq_devdiff_%s_%s.s" % (unit.replace(".hip", ""), tag)
    if not os.path.exists(path):
        r = subprocess.run(cmd + ["-o", path + ".tmp"], capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("%s\n%s" % (" ".join(cmd), r.stderr[-4000:]))
        os.replace(path + ".tmp", path)
    with open(path) as fh:
        return fh.read()


def functions(text):
    """{symbol: (instruction and label lines, resource lines)} of a listing."""
    out = {}
    parts = re.split(r"^\t\.type\t(\S+),@function\n", text, flags=re.M)
    for name, body in zip(parts[1::2], parts[2::2]):
        end = re.search(r"^\.Lfunc_end\d+:", body, flags=re.M)
        if end is None:
            continue
        norm = lambda l: re.sub(r"\.LBB\d+_", ".LBB_", l)
        code = [norm(l) for l in body[:end.start()].split("\n")
                if re.match(r"\.LBB\d+_\d+:", l) or (l.startswith("\t") and not l.strip().startswith((".", ";")))]
        # the kernel descriptor (.amdhsa_*) stands BEFORE .Lfunc_end, the .set lines and the "; Name: n" comments after it
        res = [l.strip() for l in body[:end.start()].split("\n") if re.match(r"\s*\.amdhsa_", l)] + [
            l.strip() for l in body[end.end():].split("\n") if re.match(r"\t\.set |; [\w:]+ ?: \d+", l)]
        if res and res[0].startswith(".amdhsa_kernel") and not (
                any(l.startswith(".amdhsa_group_segment_fixed_size") for l in res)
                and any(l.startswith("; LDSByteSize:") for l in res) and any(l.startswith("; Occupancy:") for l in res)):
            sys.exit("kernel %s: no LDS or occupancy line found; this listing format is not understood" % name)
        out[name] = (code, res)
    return out


def compare(a, b, verbose):
    """-> (symbols, only in A, only in B, instruction differences, resource differences)"""
    fa, fb = functions(a), functions(b)
    both = sorted(set(fa) & set(fb))
    code = [s for s in both if fa[s][0] != fb[s][0]]
    res = [s for s in both if fa[s][1] != fb[s][1]]
    if verbose:
        for k, s in [(0, s) for s in code] + [(1, s) for s in res]:
            print("\n".join(list(difflib.unified_diff(fa[s][k], fb[s][k], "A:" + s, "B:" + s, lineterm="", n=2))[:60]))
    return both, sorted(set(fa) - set(fb)), sorted(set(fb) - set(fa)), code, res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("units", nargs="*", help="default: every .hip unit of either tree")
    ap.add_argument("-j", type=int, default=8, help="parallel compilations")
    ap.add_argument("-v", action="store_true", help="print the first lines of every difference")
    args = ap.parse_args()
    ba, bb = load_build(args.tree_a), load_build(args.tree_b)
    units = args.units or sorted(u for u in set(ba.UNITS) | set(bb.UNITS) if u.endswith(".hip"))
    jobs = [(u, t) for u in units for t in (False, True)]
    with ThreadPoolExecutor(max_workers=args.j) as ex:
        texts = list(ex.map(lambda j: [listing(b, j[0], j[1]) if j[0] in b.UNITS else "" for b in (ba, bb)], jobs))
    bad = 0
    for (unit, tuning), (a, b) in zip(jobs, texts):
        both, only_a, only_b, code, res = compare(a, b, args.v)
        n = len(only_a) + len(only_b) + len(code) + len(res)
        bad += n
        print("%-22s %-8s %3d symbols: %d only in A, %d only in B, %d instruction differences, %d resource differences%s"
              % (unit, "tuning" if tuning else "shipped", len(both), len(only_a), len(only_b), len(code), len(res),
                 "" if n == 0 else "   <-- " + ", ".join((only_a + only_b + code + res)[:4])))
    print("device code: %s" % ("IDENTICAL" if bad == 0 else "%d DIFFERENCES" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
