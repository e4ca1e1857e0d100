"""What the proximal weight of the Newton family costs, at the workload of tools/measure_newton.py and
tools/measure_polish.py: N = 8, B = 65536, every kind, P diagonal (DQQ_P_DIAG) and dense (DQQ_P_DENSE), positive definite.
  * reg = 1e-7 against reg = 0 in this library: dqq_newton_bwd_reg_f64, dqq_newton_jvp_reg_f64, dqq_newton_jac_reg_f64 at the
    library's own forward (eps = 1e-7) polished with 8 steps, and dqq_polish_reg_f64 (8 steps) from a forward at eps = 1e-3 --
    with the mean number of accepted steps of each, which is what a polish's time follows;
  * --parent-lib PATH: the parent entries (dqq_newton_bwd_f64, dqq_newton_jvp_f64, dqq_newton_jac_f64, dqq_polish_f64) of this
    library -- calls with reg = 0 -- against the same entries of another build of the library, both bound with ctypes.
The method of tools/measure_polish.py: rotating buffer sets larger than the L3 (256 MiB), device events around a window of
`--calls` launches, median of 5 windows, the two sides alternating window by window in one process.
usage: python tools/measure_reg.py [--calls 40] [--reg 1e-7] [--parent-lib other/libdiffqcqp_hip.so]"""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from measure_polish import show, windows   # noqa: E402

F64 = torch.float64
PARENTS = ("dqq_newton_bwd_f64", "dqq_newton_jvp_f64", "dqq_newton_jac_f64", "dqq_polish_f64")


def bind(path, signatures):
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in PARENTS:
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = signatures[name]
    return lib


def raw_runs(lib, tag, kind, layout, B, N, stream):
    """The four parent entries of `lib` on a buffer set, by raw pointers (no scratch: N <= 64)."""
    p = lambda t: None if t is None else t.data_ptr()   # noqa: E731

    def ex3(d):
        return [p(e) for e in d["ex"]] + [None] * (3 - len(d["ex"]))

    def opt(d, i):
        return p(d["outs"][i]) if kind else None

    def tan(d, i):
        return p(d["tan"][i]) if i < len(d["tan"]) else None
    return [
        (tag + " bwd", lambda d: lib.dqq_newton_bwd_f64(kind, p(d["P"]), p(d["q"]), *ex3(d), p(d["x"]), p(d["g"]), p(d["outs"][0]),
                                                        p(d["outs"][1]), opt(d, 2), opt(d, 3), B, N, layout, None, None, 0, stream)),
        (tag + " jvp", lambda d: lib.dqq_newton_jvp_f64(kind, p(d["P"]), p(d["q"]), *ex3(d), p(d["x"]), tan(d, 0), tan(d, 1), tan(d, 2),
                                                        tan(d, 3), p(d["dx"]), B, N, layout, None, None, 0, stream)),
        (tag + " jac", lambda d: lib.dqq_newton_jac_f64(kind, p(d["P"]), p(d["q"]), *ex3(d), p(d["x"]), p(d["J"][0]),
                                                        p(d["J"][1]) if kind else None, p(d["J"][2]) if kind else None, B, N, layout,
                                                        None, None, 0, stream)),
        (tag + " polish", lambda d: lib.dqq_polish_f64(kind, p(d["P"]), p(d["q"]), *ex3(d), p(d["x0"]), p(d["dx"]), B, N, 8, layout,
                                                       None, None, None, None, 0, stream)),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--reg", type=float, default=1e-7)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    from diffqcqp_amd import _capi, ops
    B, N = 65536, 8
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1000)
    r = lambda *s: torch.rand(*s, generator=g, dtype=F64, device=dev)      # noqa: E731
    libs = None
    if a.parent_lib:
        libs = (bind(a.parent_lib, _capi.SIGNATURES), bind(_capi.LIB_PATH, _capi.SIGNATURES))
    stream = torch.cuda.current_stream().cuda_stream
    for structure, layout in (("diag", _capi.P_DIAG), ("dense", _capi.P_DENSE)):
        pshape = (B, N) if structure == "diag" else (B, N, N)
        per = 5 * pshape[1] * (pshape[2] if len(pshape) == 3 else 1) * 8 + 14 * N * 8   # P, dP, grad_P, Jacobians and the vectors
        nsets = max(2, (256 << 20) // (B * per) + 1)
        for kind, name in enumerate(("qp", "qcqp", "box", "sbox")):
            eshape = (B, N // 2, 1) if kind == 1 else (B, N, 1)
            jshapes = ((B, N, 2) if kind == 1 else (B, N), (B, N), (B, N)) if structure == "diag" else \
                ((B, N, N), (B, N, eshape[1]), (B, N, eshape[1]))
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
                x0 = ops._forward(kind, P, q, ex, 1e-3, 10000, layout=layout)
                x = ops._forward(kind, P, q, ex, 1e-7, 10000, layout=layout)
                ops._polish(kind, P, q, ex, x, 8, layout, out=x)
                tan = [2 * r(*pshape) - 1, 2 * r(B, N, 1) - 1] + ([2 * r(*eshape) - 1, 2 * r(*eshape) - 1] if kind else [])
                outs = [torch.empty(pshape, dtype=F64, device=dev), torch.empty(B, N, 1, dtype=F64, device=dev)]
                outs += [torch.empty(eshape, dtype=F64, device=dev), torch.empty(eshape, dtype=F64, device=dev)] if kind else []
                J = [torch.empty(s, dtype=F64, device=dev) for s in jshapes[:3 if kind else 1]]
                sets.append(dict(P=P, q=q, ex=ex, x=x, x0=x0, g=2 * r(B, N, 1) - 1, tan=tan, outs=outs, J=J, dx=torch.empty_like(x)))
            need = (True,) * 4
            d = sets[0]
            steps = [ops._polish(kind, d["P"], d["q"], d["ex"], d["x0"], 8, layout, return_info=True, reg=w)[2].double().mean().item()
                     for w in (0.0, a.reg)]
            runs = []
            for tag, w in (("reg=0", 0.0), ("reg=%g" % a.reg, a.reg)):
                runs += [
                    (tag + " bwd", lambda d, w=w: ops._newton_backward(kind, d["P"], d["q"], d["ex"], d["x"], d["g"], need, layout,
                                                                      out=d["outs"], reg=w)),
                    (tag + " jvp", lambda d, w=w: ops._newton_jvp(kind, d["P"], d["q"], d["ex"], d["x"], d["tan"], layout, out=d["dx"],
                                                                 reg=w)),
                    (tag + " jac", lambda d, w=w: ops._newton_jacobian(kind, d["P"], d["q"], d["ex"], d["x"], (True,) * 3, layout,
                                                                      out=d["J"], reg=w)),
                    (tag + " polish", lambda d, w=w: ops._polish(kind, d["P"], d["q"], d["ex"], d["x0"], 8, layout, out=d["dx"], reg=w)),
                ]
            print("%-5s %-5s %d buffer sets, accepted polish steps (mean) reg=0 %.3f / reg=%g %.3f: %s" % (
                name, structure, nsets, steps[0], a.reg, steps[1], show(windows(runs, sets, a.calls))), flush=True)
            if libs is not None:
                runs = raw_runs(libs[0], "parent", kind, layout, B, N, stream) + raw_runs(libs[1], "this", kind, layout, B, N, stream)
                print("%-5s %-5s against %s: %s" % (name, structure, a.parent_lib, show(windows(runs, sets, a.calls))), flush=True)
            del sets


if __name__ == "__main__":
    main()
