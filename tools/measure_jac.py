"""What the Newton Jacobians cost beside the column loop they replace: N = 8, B = 65536, us per launch of
dqq_newton_jac_f64 (every output requested) against the N (QP), 2N (QCQP) or 3N (box kinds) dqq_newton_jvp_f64 launches with
unit tangents that give the same columns, and against a single dqq_newton_jvp_f64 with every tangent given; every kind, P
diagonal (DQQ_P_DIAG) and dense (DQQ_P_DENSE), at the library's own forward (eps = 1e-7) polished with 8 steps.
The method of tools/measure_newton.py: rotating buffer sets larger than the L3 (256 MiB), device events around a window of
`--calls` calls, median of 5 windows, the three alternating window by window in one process.  "loop" is one call = all its
launches; the unit tangents (one (B,.,1) buffer per column) are shared by the buffer sets.
usage: python tools/measure_jac.py [--calls 20]"""
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
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    from diffqcqp_amd import _capi, ops
    B, N = 65536, 8
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1000)
    r = lambda *s: torch.rand(*s, generator=g, dtype=F64, device=dev)      # noqa: E731
    for structure, layout in (("diag", _capi.P_DIAG), ("dense", _capi.P_DENSE)):
        pshape = (B, N) if structure == "diag" else (B, N, N)
        for kind, name in enumerate(("qp", "qcqp", "box", "sbox")):
            eshape = (B, N // 2, 1) if kind == 1 else (B, N, 1)
            shapes = ops._jac_shapes(kind, B, N, layout)[:3 if kind else 1]
            per = 8 * (sum(torch.Size(s[1:]).numel() for s in shapes) + torch.Size(pshape[1:]).numel() + 6 * N)
            nsets = max(2, (256 << 20) // (B * per) + 1)
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
                sets.append(dict(P=P, q=q, ex=ex, x=x, tan=tan, J=[torch.empty(s, dtype=F64, device=dev) for s in shapes],
                                 dx=torch.empty_like(x)))
            units = []   # (dP, dq, da, db) of every column: one unit tangent, the rest NULL
            for which in range(3 if kind else 1):
                w = N if which == 0 else eshape[1]
                for j in range(w):
                    e = torch.zeros((B, w, 1), dtype=F64, device=dev)
                    e[:, j] = 1.0
                    t = [None, None, None, None]
                    t[1 + which] = e
                    units.append(t[:4 if kind else 2])

            def loop(d):
                for t in units:
                    ops._newton_jvp(kind, d["P"], d["q"], d["ex"], d["x"], t, layout, out=d["dx"])

            d = sets[0]
            status = ops._newton_jacobian(kind, d["P"], d["q"], d["ex"], d["x"], layout=layout, return_status=True)[-1]
            runs = [
                ("jacobian", lambda d: ops._newton_jacobian(kind, d["P"], d["q"], d["ex"], d["x"], layout=layout, out=d["J"])),
                ("loop of %d jvp" % len(units), loop),
                ("one jvp", lambda d: ops._newton_jvp(kind, d["P"], d["q"], d["ex"], d["x"], d["tan"], layout, out=d["dx"])),
            ]
            print("%-5s %-5s %d buffer sets: %s   [status 0 on %.2f %%]" % (
                name, structure, nsets, show(windows(runs, sets, a.calls)), 100.0 * (status == 0).double().mean().item()), flush=True)
            del sets, units


if __name__ == "__main__":
    main()
