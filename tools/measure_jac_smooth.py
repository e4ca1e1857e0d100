"""What the smoothed Newton Jacobians cost: N = 8, B = 65536, tools/measure_polish.py's inputs and method --
rotating buffer sets larger than the L3 (256 MiB), device events around a window of `--calls` launches, median of 5 windows, the
alternatives alternating window by window.  us per launch, every kind, P diagonal (DQQ_P_DIAG) and dense (DQQ_P_DENSE: LDS
teams), every Jacobian requested, at the smoothed polish's x:
  jacobian  dqq_newton_jac_reg_f64 | dqq_newton_jac_smooth_f64 at kappa = 0 (the parent's kernels behind the new entry) | at 1e-2
  jvps      for context: the launches of dqq_newton_jvp_smooth_f64 at kappa = 1e-2 the Jacobian call replaces, one per column (N for
            the QP, 2N for the QCQP, 3N for the box kinds), each on a unit tangent
usage: python tools/measure_jac_smooth.py [--calls 40] [--n 8] [--batch 65536]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.measure_polish import show, windows   # noqa: E402

F64 = torch.float64
KAPPA, H = 1e-2, 8


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
    p = lambda t: None if t is None else t.data_ptr()                      # noqa: E731

    def scratch(query, *args):      # the any-N form's workspace (N > 64; nothing below): (the buffer, its pointer or None, bytes)
        nbytes = query(*args)
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        return buf, (buf.data_ptr() if nbytes else None), nbytes

    for structure, layout in (("diag", _capi.P_DIAG), ("dense", _capi.P_DENSE)):
        if structure == "diag" and N not in (2, 4, 8, 16, 32, 64):
            print("diag rows skipped: DQQ_P_DIAG serves N = 2, 4, .., 64 only", flush=True)
            continue
        diag = structure == "diag"
        for kind, name in enumerate(("qp", "qcqp", "box", "sbox")):
            eshape = (B, N // 2, 1) if kind == 1 else (B, N, 1)
            ne = 0 if kind == 0 else eshape[1]
            shapes = ((B, N, 2) if kind == 1 else (B, N), (B, N), (B, N)) if diag else ((B, N, N), (B, N, ne), (B, N, ne))
            cols = N + 2 * ne
            per = ((N if diag else N * N) + 5 * N + (2 * N if diag else N * cols)) * 8
            nsets = max(2, (256 << 20) // (B * per) + 1)
            wj = scratch(lib.dqq_newton_jac_scratch_bytes, kind, N, B) if not diag else (None, None, 0)
            wn = scratch(lib.dqq_newton_scratch_bytes, kind, N, B) if not diag else (None, None, 0)
            sets = []
            for _ in range(nsets):
                if diag:
                    P = (r(B, N) + 0.5).contiguous()
                else:
                    S = r(B, N, N)
                    P = (torch.bmm(S, S.transpose(1, 2)) / N + torch.eye(N, dtype=F64, device=dev)).contiguous()
                q = 2 * r(B, N, 1) - 1
                ex = [] if kind == 0 else [r(*eshape), r(*eshape)] if kind == 1 else [-0.6 * (r(*eshape) + 0.5), 0.6 * (r(*eshape) + 0.5)]
                if kind == 3:
                    ex.append(2 * r(B, N, 1) - 1)
                x = ops._forward(kind, P, q, ex, 1e-4, 10000, layout=layout)
                xs = ops._polish(kind, P, q, ex, x, 40, layout, max_halvings=H, kappa=KAPPA)
                new = lambda shape: torch.empty(shape, dtype=F64, device=dev)      # noqa: E731
                J = [new(shapes[0])] + ([new(shapes[1]), new(shapes[2])] if kind else [None, None])
                sets.append(dict(P=P, q=q, e3=[e.data_ptr() for e in ex] + [None] * (3 - len(ex)), ex=ex, xs=xs, J=J, dx=new((B, N, 1))))
            # the unit tangents: one (B, width, 1) tensor per column, shared by the sets (they are inputs)
            units = []
            for which in range(3 if kind else 1):
                w = N if which == 0 else ne
                for j in range(w):
                    t = torch.zeros((B, w, 1), dtype=F64, device=dev)
                    t[:, j] = 1.0
                    units.append((which, t))

            def jac(d, kappa):
                head = (kind, p(d["P"]), p(d["q"]), *d["e3"], p(d["xs"]), *[p(j) for j in d["J"]], B, N, layout, 0.0)
                tail = (None, wj[1], wj[2], stream)
                rc = lib.dqq_newton_jac_reg_f64(*head, *tail) if kappa is None else lib.dqq_newton_jac_smooth_f64(*head, kappa, *tail)
                assert rc == 0

            def jvps(d):
                for which, t in units:
                    tang = [None, None, None, None]
                    tang[1 + which] = p(t)
                    rc = lib.dqq_newton_jvp_smooth_f64(kind, p(d["P"]), p(d["q"]), *d["e3"], p(d["xs"]), *tang, p(d["dx"]), B, N, layout, 0.0,
                                                       KAPPA, None, wn[1], wn[2], stream)
                    assert rc == 0

            runs = [("parent", lambda d: jac(d, None)), ("kappa=0", lambda d: jac(d, 0.0)), ("kappa=1e-2", lambda d: jac(d, KAPPA))]
            print("%-5s %-5s jacobian %s" % (name, structure, show(windows(runs, sets, a.calls))), flush=True)
            runs = [("%d jvps at 1e-2" % len(units), jvps)]
            print("%-5s %-5s jvps     %s" % (name, structure, show(windows(runs, sets, max(2, a.calls // 8)))), flush=True)
            del sets


if __name__ == "__main__":
    main()
