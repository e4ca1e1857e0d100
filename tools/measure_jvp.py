"""What the forward-mode derivative costs next to the backward of the same family: N = 8, B = 65536, every
kind, P diagonal (DQQ_P_DIAG: jvp_diag against bwd_diag) and dense (DQQ_P_DENSE | DQQ_F_REFERENCE_ORDER: jvp_dense against the
backward's reference-order kernel), us per launch, in one process.  The method of tools/measure_warm.py: rotating buffer sets
larger than the L3 (256 MiB), device events around a window of `--calls` launches, median of 5 windows, the two calls
alternating window by window.  x is the library's own forward at eps = 1e-10; every tangent and every gradient is asked for.
usage: python tools/measure_jvp.py [--calls 40]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
F64 = torch.float64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    a = ap.parse_args()
    from diffqcqp_amd import _capi, ops
    B, N = 65536, 8
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1000)
    r = lambda *s: torch.rand(*s, generator=g, dtype=F64, device=dev)      # noqa: E731
    n = lambda *s: torch.randn(*s, generator=g, dtype=F64, device=dev)     # noqa: E731
    for structure, layout in (("diag", _capi.P_DIAG), ("dense", _capi.P_DENSE | _capi.F_REFERENCE_ORDER)):
        pshape = (B, N) if structure == "diag" else (B, N, N)
        per = 2 * (N if structure == "diag" else N * N) * 8 + 10 * N * 8
        nsets = max(2, (256 << 20) // (B * per) + 1)
        for kind, name in enumerate(("qp", "qcqp", "box", "sbox")):
            eshape = (B, N // 2, 1) if kind == 1 else (B, N, 1)
            sets = []
            for _ in range(nsets):
                if structure == "diag":
                    P = (r(B, N) + 0.5).contiguous()
                else:
                    S = r(B, N, N)
                    P = (torch.bmm(S, S.transpose(1, 2)) / N + torch.eye(N, dtype=F64, device=dev)).contiguous()
                q = 2 * r(B, N, 1) - 1
                ex = [] if kind == 0 else [r(*eshape), r(*eshape)] if kind == 1 else [-0.6 * (r(*eshape) + 0.5), 0.6 * (r(*eshape) + 0.5)]
                if kind == 3:
                    ex.append(2 * r(B, N, 1) - 1)
                x = ops._forward(kind, P, q, ex, 1e-10, 10000, layout=layout)
                tans = [n(*pshape), n(B, N, 1)] + ([n(*eshape), n(*eshape)] if kind else [])
                outs = [torch.empty(pshape, dtype=F64, device=dev), torch.empty(B, N, 1, dtype=F64, device=dev)]
                outs += [torch.empty(eshape, dtype=F64, device=dev), torch.empty(eshape, dtype=F64, device=dev)] if kind else []
                sets.append(dict(P=P, q=q, ex=ex, x=x, tans=tans, g=n(B, N, 1), outs=outs, dx=torch.empty(B, N, 1, dtype=F64, device=dev)))
            runs = [("bwd", lambda d: ops._backward(kind, d["P"], d["q"], d["ex"], d["x"], d["g"], (True,) * 4, layout, False, d["outs"],
                                                    1e-10, None, None, None)),
                    ("jvp", lambda d: ops._jvp(kind, d["P"], d["q"], d["ex"], d["x"], d["tans"], layout, out=d["dx"]))]
            times = {k: [] for k, _ in runs}
            for window in range(6):   # (the first window warms up and is dropped)
                for k, fn in runs:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for c in range(a.calls):
                        fn(sets[c % nsets])
                    e1.record()
                    torch.cuda.synchronize()
                    if window:
                        times[k].append(e0.elapsed_time(e1) * 1000.0 / a.calls)
            print("%-5s %-5s %d buffer sets: " % (name, structure, nsets) +
                  "   ".join("%s %.1f us (%s)" % (k, sorted(v)[2], " ".join("%.1f" % t for t in v)) for k, v in times.items()), flush=True)
            del sets


if __name__ == "__main__":
    main()
