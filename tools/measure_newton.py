"""What the Newton derivatives cost beside the reference derivatives: N = 8, B = 65536, us per launch of
dqq_newton_bwd_f64 against the kind's backward and of dqq_newton_jvp_f64 against dqq_jvp_f64, every kind, P diagonal
(DQQ_P_DIAG: newton_diag against bwd_diag / jvp_diag) and dense (DQQ_P_DENSE: newton_dense's LDS teams against the general
backward / jvp_dense), at the library's own forward (eps = 1e-7) polished with 8 steps, every gradient / tangent requested.
The method of tools/measure_polish.py: rotating buffer sets larger than the L3 (256 MiB), device events around a window of
`--calls` launches, median of 5 windows, the new call and the existing one alternating window by window in one process.
usage: python tools/measure_newton.py [--calls 40]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from measure_polish import show, windows   # noqa: E402

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
    for structure, layout in (("diag", _capi.P_DIAG), ("dense", _capi.P_DENSE)):
        pshape = (B, N) if structure == "diag" else (B, N, N)
        per = 3 * pshape[1] * (pshape[2] if len(pshape) == 3 else 1) * 8 + 12 * N * 8   # P, dP, grad_P and a dozen vectors
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
                x = ops._forward(kind, P, q, ex, 1e-7, 10000, layout=layout)
                ops._polish(kind, P, q, ex, x, 8, layout, out=x)
                tan = [2 * r(*pshape) - 1, 2 * r(B, N, 1) - 1] + ([2 * r(*eshape) - 1, 2 * r(*eshape) - 1] if kind else [])
                outs = [torch.empty(pshape, dtype=F64, device=dev), torch.empty(B, N, 1, dtype=F64, device=dev)]
                outs += [torch.empty(eshape, dtype=F64, device=dev), torch.empty(eshape, dtype=F64, device=dev)] if kind else []
                sets.append(dict(P=P, q=q, ex=ex, x=x, g=2 * r(B, N, 1) - 1, tan=tan, outs=outs, dx=torch.empty_like(x)))
            need = (True,) * 4
            d = sets[0]
            status = ops._newton_backward(kind, d["P"], d["q"], d["ex"], d["x"], d["g"], need, layout, return_status=True)[-1]
            runs = [
                ("newton bwd", lambda d: ops._newton_backward(kind, d["P"], d["q"], d["ex"], d["x"], d["g"], need, layout, out=d["outs"])),
                ("bwd", lambda d: ops._backward(kind, d["P"], d["q"], d["ex"], d["x"], d["g"], need, layout, False, d["outs"], 1e-10,
                                                None, None, None)),
                ("newton jvp", lambda d: ops._newton_jvp(kind, d["P"], d["q"], d["ex"], d["x"], d["tan"], layout, out=d["dx"])),
                ("jvp", lambda d: ops._jvp(kind, d["P"], d["q"], d["ex"], d["x"], d["tan"], layout, out=d["dx"])),
            ]
            print("%-5s %-5s %d buffer sets: %s   [status 0 on %.2f %%]" % (
                name, structure, nsets, show(windows(runs, sets, a.calls)), 100.0 * (status == 0).double().mean().item()), flush=True)
            del sets


if __name__ == "__main__":
    main()
