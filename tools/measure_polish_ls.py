"""What the damped polish costs and what it repairs: N = 8, B = 65536, tools/measure_polish.py's inputs.
  1. us per launch, every kind, P diagonal (DQQ_P_DIAG) and dense (DQQ_P_DENSE: LDS teams), from the library's own forward at
     eps = 1e-4, max_steps = 8: dqq_polish_f64 (the parent), and dqq_polish_ls_f64 at max_halvings = 0 and 8.
  2. the same from the cold start x = 0 (the QP's and the discs' PI(0); the boxes contain 0), max_steps = 60: how many problems
     of the batch end with status 0 / 1 under each setting, and the launch's time.
  3. the reference's figure workload (QP, P = diag(exp(U(-10, 10))), DQQ_P_DIAG) from the forward stopped at max_iter = 20 and
     from the cold start: the problems that end with status 1, and those above the bar 64 x 2.8e-16 x scale, counted on the
     device outputs, at max_halvings = 0, 8 and 20.
The method of tools/measure_polish.py: rotating buffer sets larger than the L3 (256 MiB), device events around a window of
`--calls` launches, median of 5 windows, the alternatives alternating window by window.
usage: python tools/measure_polish_ls.py [--calls 40] [--n 8] [--batch 65536]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.measure_polish import show, windows   # noqa: E402

F64 = torch.float64
BAR = 64 * 2.8e-16


def counts(ops, kind, d, x, steps, layout, h):
    """-> (status 0, status 1, problems with r after above the bar) of one batch, on the device outputs"""
    xo, resid, _, status = ops._polish(kind, d["P"], d["q"], d["ex"], x, steps, layout, return_info=True, max_halvings=h)
    _, chk, _ = ops.solution_check(kind, d["P"], d["q"], d["ex"], xo, layout=layout)
    return (status == 0).sum().item(), (status == 1).sum().item(), (resid[:, 1] > BAR * chk[:, 3]).sum().item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--n", type=int, default=8, help="N; the dense rows run at any N (LDS teams to 64, any-N beyond)")
    ap.add_argument("--batch", type=int, default=65536, help="B")
    a = ap.parse_args()
    from diffqcqp_amd import _capi, ops
    B, N = a.batch, a.n
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1000)
    r = lambda *s: torch.rand(*s, generator=g, dtype=F64, device=dev)      # noqa: E731
    lib = _capi.lib()
    stream = torch.cuda.current_stream().cuda_stream

    def scratch(query, kind):      # the any-N form's workspace (N > 64; nothing below): (the buffer, its pointer or None, bytes)
        nbytes = query(kind, N, B)
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        return buf, (buf.data_ptr() if nbytes else None), nbytes

    def ls0(kind, d, x, steps, layout):      # the damped kernels with no halving allowed (ops._polish sends 0 to the parent)
        ex = [e.data_ptr() for e in d["ex"]] + [None] * (3 - len(d["ex"]))
        assert lib.dqq_polish_ls_f64(kind, d["P"].data_ptr(), d["q"].data_ptr(), *ex, x.data_ptr(), d["xo"].data_ptr(), B, N, steps,
                                     layout, 0.0, 0, None, None, None, None, ws[1], ws[2], stream) == 0

    for structure, layout in (("diag", _capi.P_DIAG), ("dense", _capi.P_DENSE)):
        if structure == "diag" and N not in (2, 4, 8, 16, 32, 64):
            print("diag rows skipped: DQQ_P_DIAG serves N = 2, 4, .., 64 only", flush=True)
            continue
        per = (N if structure == "diag" else N * N) * 8 + 6 * N * 8
        nsets = max(2, (256 << 20) // (B * per) + 1)
        for kind, name in enumerate(("qp", "qcqp", "box", "sbox")):
            eshape = (B, N // 2, 1) if kind == 1 else (B, N, 1)
            ws = scratch(lib.dqq_polish_scratch_bytes, kind) if structure == "dense" else (None, None, 0)
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
                sets.append(dict(P=P, q=q, ex=ex, x=x, cold=torch.zeros_like(x), xo=torch.empty_like(x)))
            for start, steps in (("x", 8), ("cold", 60)):
                runs = [("parent", lambda d: ops._polish(kind, d["P"], d["q"], d["ex"], d[start], steps, layout, out=d["xo"])),
                        ("ls h=0", lambda d: ls0(kind, d, d[start], steps, layout)),
                        ("ls h=8", lambda d: ops._polish(kind, d["P"], d["q"], d["ex"], d[start], steps, layout, out=d["xo"], max_halvings=8))]
                c = {h: counts(ops, kind, sets[0], sets[0][start], steps, layout, h) for h in (0, 8)}
                print("%-5s %-5s from %-12s %s   [status 0 / 1 / above the bar of %d: h=0 %s, h=8 %s]" % (
                    name, structure, "the forward:" if start == "x" else "the cold x:", show(windows(runs, sets, a.calls)), B, c[0], c[8]),
                    flush=True)
            del sets
    # the figure workload
    if N not in (2, 4, 8, 16, 32, 64):
        return
    layout = _capi.P_DIAG
    P = torch.exp(20 * r(B, N) - 10).contiguous()
    d = dict(P=P, q=torch.randn(B, N, 1, generator=g, dtype=F64, device=dev), ex=[])
    starts = (("the forward at max_iter 20", ops._forward(0, d["P"], d["q"], (), 1e-12, 20, layout=layout)),
              ("the forward at eps 1e-4", ops._forward(0, d["P"], d["q"], (), 1e-4, 100000, layout=layout)),
              ("the cold start", torch.zeros(B, N, 1, dtype=F64, device=dev)))
    for name, x in starts:
        for steps in (8, 60):
            print("figure workload from %s, max_steps %d, status 0 / 1 / above the bar of %d: %s" % (
                name, steps, B, "   ".join("h=%d %s" % (h, counts(ops, 0, d, x, steps, layout, h)) for h in (0, 8, 20))), flush=True)


if __name__ == "__main__":
    main()
