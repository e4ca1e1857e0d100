"""What the active-set report costs beside the comparable launches: N = 8, B = 65536, us per launch of
dqq_newton_active_f64 (all five outputs) against dqq_check_f64 -- the comparable streaming launch: the same inputs, small
outputs -- and against dqq_newton_jvp_f64 (every tangent given), every kind, P diagonal (DQQ_P_DIAG: active_diag against
check_diag / newton_diag) and dense (DQQ_P_DENSE: active_dense's LDS teams against check / newton_dense's), at the library's own
forward (eps = 1e-7) polished with 8 steps.  The method of tools/measure_polish.py: rotating buffer sets larger than the L3
(256 MiB), device events around a window of `--calls` launches, median of 5 windows, the calls alternating window by window in
one process.
usage: python tools/measure_active.py [--calls 40]"""
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
        per = 2 * pshape[1] * (pshape[2] if len(pshape) == 3 else 1) * 8 + 12 * N * 8   # P, dP and a dozen vectors
        nsets = max(2, (256 << 20) // (B * per) + 1)
        for kind, name in enumerate(("qp", "qcqp", "box", "sbox")):
            eshape = (B, N // 2, 1) if kind == 1 else (B, N, 1)
            ne = eshape[1]
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
                act = (torch.empty(B, ne, dtype=torch.int32, device=dev), torch.empty(B, ne, dtype=F64, device=dev),
                       torch.empty(B, dtype=F64, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
                       torch.empty(B, dtype=torch.int32, device=dev))
                chk = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, 4, dtype=F64, device=dev),
                       torch.zeros(3, dtype=torch.int64, device=dev))
                sets.append(dict(P=P, q=q, ex=ex, x=x, tan=tan, act=act, chk=chk, dx=torch.empty_like(x)))
            d = sets[0]
            first = ops._newton_active(kind, d["P"], d["q"], d["ex"], d["x"], layout)
            runs = [
                ("active", lambda d: ops._newton_active(kind, d["P"], d["q"], d["ex"], d["x"], layout, out=d["act"])),
                # (the C entry itself, without counts: ops.solution_check would put a fill launch for them into the window)
                ("check", lambda d: _capi.lib().dqq_check_f64(
                    kind, d["P"].data_ptr(), d["q"].data_ptr(), *([e.data_ptr() for e in d["ex"]] + [0] * (3 - len(d["ex"]))),
                    d["x"].data_ptr(), 0, 0, B, N, layout, d["chk"][1].data_ptr(), d["chk"][0].data_ptr(), 0,
                    torch.cuda.current_stream().cuda_stream)),
                ("newton jvp", lambda d: ops._newton_jvp(kind, d["P"], d["q"], d["ex"], d["x"], d["tan"], layout, out=d["dx"])),
            ]
            print("%-5s %-5s %d buffer sets: %s   [status 0 on %.2f %%, active elements %.1f %%, median margin %.2e]" % (
                name, structure, nsets, show(windows(runs, sets, a.calls)), 100.0 * (first.status == 0).double().mean().item(),
                100.0 * (first.state > 0).double().mean().item(), first.margin.median().item()), flush=True)
            del sets


if __name__ == "__main__":
    main()
