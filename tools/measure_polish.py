"""What a polish costs and what it buys: N = 8, B = 65536.
  1. us per dqq_polish_f64 launch, every kind, P diagonal (DQQ_P_DIAG: polish_diag) and dense (DQQ_P_DENSE: polish_dense's LDS
     teams), from the library's own forward at eps = 1e-4, max_steps = 8.
  2. the reference's figure workload (QP, P = diag(exp(U(-10, 10))), DQQ_P_DIAG): the forward at eps = 1e-10 alone against the
     forward at eps = 1e-4 followed by a polish -- ms per batch and the worst natural residual (dqq_check_f64, relative to its
     scale) each way.
The method of tools/measure_warm.py: rotating buffer sets larger than the L3 (256 MiB), device events around a window of
`--calls` launches, median of 5 windows, the alternatives alternating window by window.
usage: python tools/measure_polish.py [--calls 40]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
F64 = torch.float64


def windows(runs, sets, calls):
    """-> {name: [us per call of 5 windows]}; the first window warms up and is dropped."""
    times = {k: [] for k, _ in runs}
    for window in range(6):
        for k, fn in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for c in range(calls):
                fn(sets[c % len(sets)])
            e1.record()
            torch.cuda.synchronize()
            if window:
                times[k].append(e0.elapsed_time(e1) * 1000.0 / calls)
    return times


def show(times):
    return "   ".join("%s %.1f us (%s)" % (k, sorted(v)[2], " ".join("%.1f" % t for t in v)) for k, v in times.items())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    a = ap.parse_args()
    from diffqcqp_amd import _capi, ops
    B, N = 65536, 8
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1000)
    r = lambda *s: torch.rand(*s, generator=g, dtype=F64, device=dev)      # noqa: E731
    for structure, layout in (("diag", _capi.P_DIAG), ("dense", _capi.P_DENSE)):
        per = (N if structure == "diag" else N * N) * 8 + 6 * N * 8
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
                x = ops._forward(kind, P, q, ex, 1e-4, 10000, layout=layout)
                sets.append(dict(P=P, q=q, ex=ex, x=x, xo=torch.empty_like(x)))
            d = sets[0]
            _, resid, steps, status = ops._polish(kind, d["P"], d["q"], d["ex"], d["x"], 8, layout, return_info=True)
            runs = [("polish", lambda d: ops._polish(kind, d["P"], d["q"], d["ex"], d["x"], 8, layout, out=d["xo"]))]
            print("%-5s %-5s %d buffer sets: %s   [accepted %.1f %%, steps max %d, r %.1e -> %.1e]" % (
                name, structure, nsets, show(windows(runs, sets, a.calls)), 100.0 * (status == 0).double().mean().item(),
                steps.max().item(), resid[:, 0].max().item(), resid[:, 1].max().item()), flush=True)
            del sets
    # the figure workload
    layout = _capi.P_DIAG
    nsets = max(2, (256 << 20) // (B * 4 * N * 8) + 1)
    sets = []
    for _ in range(nsets):
        P = torch.exp(20 * r(B, N) - 10).contiguous()
        q = torch.randn(B, N, 1, generator=g, dtype=F64, device=dev)
        sets.append(dict(P=P, q=q, x=torch.empty(B, N, 1, dtype=F64, device=dev)))

    def tight(d):
        return ops._forward(0, d["P"], d["q"], (), 1e-10, 100000, layout=layout, out=d["x"])

    def loose(d):
        ops._forward(0, d["P"], d["q"], (), 1e-4, 100000, layout=layout, out=d["x"])
        return ops._polish(0, d["P"], d["q"], (), d["x"], 8, layout, out=d["x"])

    for name, fn in (("forward eps 1e-10", tight), ("forward eps 1e-4 + polish", loose)):
        worst = 0.0
        for d in sets[:2]:
            _, resid, _ = ops.solution_check(0, d["P"], d["q"], (), fn(d), layout=layout)
            worst = max(worst, (resid[:, 0] / resid[:, 3]).max().item())
        print("figure workload, %-26s worst natural residual / scale %.2e" % (name + ":", worst), flush=True)
    t = windows([("forward eps 1e-10", tight), ("forward eps 1e-4 + polish", loose)], sets, max(2, a.calls // 8))
    print("figure workload, %d buffer sets: %s" % (nsets, show(t)), flush=True)


if __name__ == "__main__":
    main()
