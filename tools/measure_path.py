"""What the polish path costs: N = 8, B = 65536, tools/measure_polish.py's inputs and method -- rotating buffer
sets larger than the L3 (256 MiB), device events around a window of `--calls` launches, median of 5 windows, the alternatives
alternating window by window.  us per solve of the batch from the cold start x = PI(0), every kind, P diagonal (DQQ_P_DIAG) and
dense (DQQ_P_DENSE: LDS teams):
  path    the default schedule (kappa 1e-1, 1e-2, 1e-3, 1e-4, 0; budgets 4, 4, 4, 4, 60; max_halvings 8) as ONE dqq_polish_path_f64
  chain   the same schedule as five chained dqq_polish_smooth_f64 launches of the same library
  admm    the library's ADMM forward at eps = 1e-7, as context (another method: its x agrees to its eps, not to rounding)
and, once per row, what the path reached: the share of problems with r <= 1e-13 and the most accepted steps.
usage: python tools/measure_path.py [--calls 20] [--n 8] [--batch 65536]"""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.measure_polish import show, windows   # noqa: E402

F64 = torch.float64
KAPPAS, STEPS, H = (1e-1, 1e-2, 1e-3, 1e-4, 0.0), (4, 4, 4, 4, 60), 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
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
    p = lambda t: None if t is None else t.data_ptr()                      # noqa: E731

    def scratch(query, kind):      # the any-N form's workspace (N > 64; nothing below): (the buffer, its pointer or None, bytes)
        nbytes = query(kind, N, B)
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        return buf, (buf.data_ptr() if nbytes else None), nbytes
    S = len(KAPPAS)
    ks, ns = (ctypes.c_double * S)(*KAPPAS), (ctypes.c_int * S)(*STEPS)

    for structure, layout in (("diag", _capi.P_DIAG), ("dense", _capi.P_DENSE)):
        if structure == "diag" and N not in (2, 4, 8, 16, 32, 64):
            print("diag rows skipped: DQQ_P_DIAG serves N = 2, 4, .., 64 only", flush=True)
            continue
        per = (N if structure == "diag" else N * N) * 8 + 8 * N * 8
        nsets = max(2, (256 << 20) // (B * per) + 1)
        for kind, name in enumerate(("qp", "qcqp", "box", "sbox")):
            eshape = (B, N // 2, 1) if kind == 1 else (B, N, 1)
            ws = scratch(lib.dqq_polish_scratch_bytes, kind) if structure == "dense" else (None, None, 0)
            sets = []
            for _ in range(nsets):
                if structure == "diag":
                    P = (r(B, N) + 0.5).contiguous()
                else:
                    M = r(B, N, N)
                    P = (torch.bmm(M, M.transpose(1, 2)) / N + torch.eye(N, dtype=F64, device=dev)).contiguous()
                q = 2 * r(B, N, 1) - 1
                ex = [] if kind == 0 else [r(*eshape), r(*eshape)] if kind == 1 else [-0.6 * (r(*eshape) + 0.5), 0.6 * (r(*eshape) + 0.5)]
                if kind == 3:
                    ex.append(2 * r(B, N, 1) - 1)
                new = lambda: torch.empty((B, N, 1), dtype=F64, device=dev)      # noqa: E731
                sets.append(dict(P=P, q=q, ex=ex, e3=[e.data_ptr() for e in ex] + [None] * (3 - len(ex)), x=ops.cold_start(kind, q, ex),
                                 xo=new(), xa=new(), xb=new()))

            def path(d):
                rc = lib.dqq_polish_path_f64(kind, p(d["P"]), p(d["q"]), *d["e3"], p(d["x"]), p(d["xo"]), B, N, layout, 0.0,
                                             ctypes.addressof(ks), ctypes.addressof(ns), S, H, None, None, None, None, None, None, ws[1], ws[2],
                                             stream)
                assert rc == 0

            def chain(d):
                src, dst = d["x"], d["xa"]
                for kappa, n in zip(KAPPAS, STEPS):
                    rc = lib.dqq_polish_smooth_f64(kind, p(d["P"]), p(d["q"]), *d["e3"], p(src), p(dst), B, N, n, layout, 0.0, kappa, H,
                                                   None, None, None, None, ws[1], ws[2], stream)
                    assert rc == 0
                    src, dst = dst, (d["xb"] if dst is d["xa"] else d["xa"])

            def admm(d):
                ops._forward(kind, d["P"], d["q"], d["ex"], 1e-7, 10000, layout=layout, out=d["xb"])

            d = sets[0]
            _, resid, steps, status, _, _, _ = ops._polish_path(kind, d["P"], d["q"], d["ex"], d["x"], KAPPAS, STEPS, H, layout=layout,
                                                                return_info=True)
            path(d)
            chain(d)
            torch.cuda.synchronize()
            last = d["xa"] if S % 2 else d["xb"]
            same = bool(torch.equal(d["xo"], last))
            print("%-5s %-5s %s   | solved %.4f of %d, most steps %d, status 0/1/2: %d/%d/%d, path == chain: %s" % (
                name, structure, show(windows([("path", path), ("chain", chain), ("admm", admm)], sets, a.calls)),
                float((resid[:, 1] <= 1e-13).double().mean()), B, int(steps.max()), int((status == 0).sum()), int((status == 1).sum()),
                int((status == 2).sum()), same), flush=True)
            del sets


if __name__ == "__main__":
    main()
