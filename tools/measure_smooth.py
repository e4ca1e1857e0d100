"""What the smoothed Newton family costs: N = 8, B = 65536, tools/measure_polish.py's inputs and method --
rotating buffer sets larger than the L3 (256 MiB), device events around a window of `--calls` launches, median of 5 windows, the
alternatives alternating window by window.  us per launch, every kind, P diagonal (DQQ_P_DIAG) and dense (DQQ_P_DENSE: LDS
teams), of the three new entries against their parents:
  polish    dqq_polish_ls_f64 | dqq_polish_smooth_f64 at kappa = 0 (the parent's kernels behind the new entry) | at kappa = 1e-2;
            from the library's own forward at eps = 1e-4, max_steps = 8, max_halvings = 8
  backward  dqq_newton_bwd_f64 | dqq_newton_bwd_smooth_f64 at kappa = 0 | at 1e-2, every gradient requested, at the polished x
  jvp       dqq_newton_jvp_f64 | dqq_newton_jvp_smooth_f64 at kappa = 0 | at 1e-2, every tangent given, at the polished x
On (B,N,N) the smoothed M has no unit rows: the kappa = 1e-2 column there is the dense elimination's cost.
usage: python tools/measure_smooth.py [--calls 40] [--n 8] [--batch 65536]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.measure_polish import show, windows   # noqa: E402

F64 = torch.float64
KAPPA, STEPS, H = 1e-2, 8, 8


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
    n = lambda *s: torch.randn(*s, generator=g, dtype=F64, device=dev)     # noqa: E731
    lib = _capi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()                      # noqa: E731

    def scratch(query, kind):      # the any-N form's workspace (N > 64; nothing below): (the buffer, its pointer or None, bytes)
        nbytes = query(kind, N, B)
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        return buf, (buf.data_ptr() if nbytes else None), nbytes

    for structure, layout in (("diag", _capi.P_DIAG), ("dense", _capi.P_DENSE)):
        if structure == "diag" and N not in (2, 4, 8, 16, 32, 64):
            print("diag rows skipped: DQQ_P_DIAG serves N = 2, 4, .., 64 only", flush=True)
            continue
        pshape = (B, N) if structure == "diag" else (B, N, N)
        per = 3 * (N if structure == "diag" else N * N) * 8 + 12 * N * 8
        nsets = max(2, (256 << 20) // (B * per) + 1)
        for kind, name in enumerate(("qp", "qcqp", "box", "sbox")):
            eshape = (B, N // 2, 1) if kind == 1 else (B, N, 1)
            dense = structure == "dense"
            ws = scratch(lib.dqq_polish_scratch_bytes, kind) if dense else (None, None, 0)
            wn = scratch(lib.dqq_newton_scratch_bytes, kind) if dense else (None, None, 0)
            sets = []
            for _ in range(nsets):
                if structure == "diag":
                    P = (r(B, N) + 0.5).contiguous()
                    dP = n(B, N)
                else:
                    S = r(B, N, N)
                    P = (torch.bmm(S, S.transpose(1, 2)) / N + torch.eye(N, dtype=F64, device=dev)).contiguous()
                    dP = n(B, N, N)
                    dP = (0.5 * (dP + dP.transpose(1, 2))).contiguous()
                q = 2 * r(B, N, 1) - 1
                ex = [] if kind == 0 else [r(*eshape), r(*eshape)] if kind == 1 else [-0.6 * (r(*eshape) + 0.5), 0.6 * (r(*eshape) + 0.5)]
                if kind == 3:
                    ex.append(2 * r(B, N, 1) - 1)
                x = ops._forward(kind, P, q, ex, 1e-4, 10000, layout=layout)
                xs = ops._polish(kind, P, q, ex, x, 40, layout, max_halvings=H)
                e3 = [e.data_ptr() for e in ex] + [None] * (3 - len(ex))
                new = lambda shape: torch.empty(shape, dtype=F64, device=dev)      # noqa: E731
                d = dict(P=P, q=q, e3=e3, ex=ex, x=x, xs=xs, xo=new((B, N, 1)), gx=n(B, N, 1), dP=dP, dq=n(B, N, 1),
                         da=n(*eshape) if kind else None, db=n(*eshape) if kind else None, gP=new(pshape), gq=new((B, N, 1)),
                         ga=new(eshape) if kind else None, gb=new(eshape) if kind else None, dx=new((B, N, 1)))
                sets.append(d)

            def polish(d, kappa):
                head = (kind, p(d["P"]), p(d["q"]), *d["e3"], p(d["x"]), p(d["xo"]), B, N, STEPS, layout, 0.0)
                tail = (H, None, None, None, None, ws[1], ws[2], stream)
                rc = lib.dqq_polish_ls_f64(*head, *tail) if kappa is None else lib.dqq_polish_smooth_f64(*head, kappa, *tail)
                assert rc == 0

            def bwd(d, kappa):
                head = (kind, p(d["P"]), p(d["q"]), *d["e3"], p(d["xs"]), p(d["gx"]), p(d["gP"]), p(d["gq"]), p(d["ga"]), p(d["gb"]), B, N, layout)
                tail = (None, wn[1], wn[2], stream)
                rc = lib.dqq_newton_bwd_f64(*head, *tail) if kappa is None else lib.dqq_newton_bwd_smooth_f64(*head, 0.0, kappa, *tail)
                assert rc == 0

            def jvp(d, kappa):
                head = (kind, p(d["P"]), p(d["q"]), *d["e3"], p(d["xs"]), p(d["dP"]), p(d["dq"]), p(d["da"]), p(d["db"]), p(d["dx"]), B, N, layout)
                tail = (None, wn[1], wn[2], stream)
                rc = lib.dqq_newton_jvp_f64(*head, *tail) if kappa is None else lib.dqq_newton_jvp_smooth_f64(*head, 0.0, kappa, *tail)
                assert rc == 0

            for what, fn in (("polish", polish), ("backward", bwd), ("jvp", jvp)):
                runs = [("parent", lambda d, fn=fn: fn(d, None)), ("kappa=0", lambda d, fn=fn: fn(d, 0.0)),
                        ("kappa=1e-2", lambda d, fn=fn: fn(d, KAPPA))]
                print("%-5s %-5s %-8s %s" % (name, structure, what, show(windows(runs, sets, a.calls))), flush=True)
            del sets


if __name__ == "__main__":
    main()
