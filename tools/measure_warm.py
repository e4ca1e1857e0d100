"""What a warm start buys on the device: N = 8, B = 65536, QP and QCQP, P diagonal (through DQQ_P_DIAG) and
dense (DQQ_P_DENSE), us per forward launch --
    cold, the library given as --parent (a build of the commit before dqq_fwd_warm_f64; optional),
    cold, this build,
    warm, this build, x0 = the cold solution of the batch with q perturbed by 1 %.
Rotating buffer sets larger than the L3 (256 MiB: each launch reads inputs no launch of the last 256 MiB touched), device
events around a window of `--calls` launches, median of 5 windows, the libraries alternating window by window.
usage: python tools/measure_warm.py [--parent libdiffqcqp_hip.so] [--calls 40]"""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
vp, i32, i64, dbl, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_size_t
F64 = torch.float64


def bind(path):
    L = ctypes.CDLL(path)
    L.dqq_workspace_bytes.argtypes, L.dqq_workspace_bytes.restype = [i64], sz
    L.dqq_qp_fwd_f64.argtypes = [vp, vp, vp, i64, i32, dbl, dbl, i32, i32, i32, vp, vp, vp, vp, sz, vp]
    L.dqq_qcqp_fwd_f64.argtypes = [vp, vp, vp, vp, vp, i64, i32, dbl, dbl, i32, i32, i32, vp, vp, vp, vp, sz, vp]
    if hasattr(L, "dqq_fwd_warm_f64"):
        L.dqq_fwd_warm_f64.argtypes = [i32] + [vp] * 7 + [i64, i32, dbl, dbl, i32, i32, i32, vp, vp, vp, vp, sz, vp]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--calls", type=int, default=40)
    a = ap.parse_args()
    from diffqcqp_amd import _capi, build
    build.build()
    libs = {"this": bind(_capi.LIB_PATH)}
    if a.parent:
        libs["parent"] = bind(os.path.abspath(a.parent))
    B, N = 65536, 8
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1000)
    r = lambda *s: torch.rand(*s, generator=g, dtype=F64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    for structure, layout in (("diag", 2), ("dense", 1)):
        per = (N if layout == 2 else N * N) * 8 + 4 * N * 8
        nsets = max(2, (256 << 20) // (B * per) + 1)
        sets = []
        for _ in range(nsets):
            if layout == 2:
                P = (r(B, N) + 0.5).contiguous()
            else:
                S = r(B, N, N)
                P = (torch.bmm(S, S.transpose(1, 2)) / N + torch.eye(N, dtype=F64, device=dev)).contiguous()
            sets.append(dict(P=P, q=2 * r(B, N, 1) - 1, l_n=r(B, N // 2, 1), mu=r(B, N // 2, 1),
                             x=torch.empty(B, N, 1, dtype=F64, device=dev), x0={}))
        wsb = libs["this"].dqq_workspace_bytes(B)
        ws = torch.zeros((wsb + 3) // 4, dtype=torch.int32, device=dev)
        for kind, name in ((0, "qp"), (1, "qcqp")):
            def cold(L, d, q=None, x=None):
                q, x = d["q"] if q is None else q, d["x"] if x is None else x
                if kind == 0:
                    return L.dqq_qp_fwd_f64(p(d["P"]), p(q), p(x), B, N, 1e-7, 1e-7, 1000, 1, layout, None, None, None, p(ws), wsb, s)
                return L.dqq_qcqp_fwd_f64(p(d["P"]), p(q), p(d["l_n"]), p(d["mu"]), p(x), B, N, 1e-7, 1e-7, 1000, 1, layout, None,
                                          None, None, p(ws), wsb, s)

            def warm(L, d):
                ex = (p(d["l_n"]), p(d["mu"])) if kind == 1 else (None, None)
                return L.dqq_fwd_warm_f64(kind, p(d["P"]), p(d["q"]), ex[0], ex[1], None, p(d["x0"][kind]), p(d["x"]), B, N, 1e-7,
                                          1e-7, 1000, 1, layout, None, None, None, p(ws), wsb, s)
            for d in sets:   # the start points: the solutions of the 1 % perturbed batch
                qn = d["q"] * (1 + 0.01 * torch.randn(B, N, 1, generator=g, dtype=F64, device=dev))
                d["x0"][kind] = torch.empty(B, N, 1, dtype=F64, device=dev)
                assert cold(libs["this"], d, qn, d["x0"][kind]) == 0
            runs = [("cold " + k, (lambda d, L=L: cold(L, d))) for k, L in libs.items()] + [("warm this", lambda d: warm(libs["this"], d))]
            times = {k: [] for k, _ in runs}
            for window in range(6):   # (the first window warms up and is dropped)
                for k, fn in runs:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for c in range(a.calls):
                        assert fn(sets[c % nsets]) == 0
                    e1.record()
                    torch.cuda.synchronize()
                    if window:
                        times[k].append(e0.elapsed_time(e1) * 1000.0 / a.calls)
            print("%-5s %-5s %d buffer sets: " % (name, structure, nsets) +
                  "   ".join("%s %.1f us (%s)" % (k, sorted(v)[2], " ".join("%.1f" % t for t in v)) for k, v in times.items()))


if __name__ == "__main__":
    main()
