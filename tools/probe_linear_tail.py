#!/usr/bin/env python3
"""dev probe: a bf16 Linear whose reduction length is not a multiple of 64 -- forward (ops.linear, bias, no epilogue), dX
(meant_linear_bwd_dx) and dW (ops._bwd_dw, with the cut back to [N, K] where K was padded) at
  M = 393216, N = 768, K = 784 / 588   the patch embedding of 14 x 14 patches, 4 / 3 channels, at 128 samples x 12 days x 256 patches
  M = 36864,  N = K = 520              5 heads of 104
and, as the like-for-like rows, the same one-tile kernels at the next multiple of 64 (K = 832 with option nt_stream = 0, which
keeps the launch on the one-tile 256 x 256 kernel; K = 576 at N = 520) plus K = 832 on the streaming kernel for scale.

Per row: the median ms of ROUNDS rounds in which all rows take turns (so that drift of the box hits them alike), the algorithmic
TFLOP/s 2 M N K / time with the Linear's own K, and the routes the call took.  The script runs unchanged on a build without the
K-tail kernels (there the tail rows go to the exact-f32 engine, route "gemm_f32"): that is where the "before" figures of DESIGN
section 6 "Linear at any K" come from.
usage: python tools/probe_linear_tail.py [rounds, default 5]"""
import os, statistics, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from meant_amd import _lib, ops
from meant_amd._lib import lib, check, BF16

dev = torch.device("cuda")
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
BF = torch.bfloat16
ROUTES = ("nt128k", "nt256k", "nt128", "nt256", "nt256s", "gemm_f32", "tn128", "tn256", "tn_tail")
HAS_TAIL = hasattr(ops, "_k_pad")                     # a build with the K-tail kernels and the K padding of ops.linear
# (M, N, K, nt_stream)
CASES = [(393216, 768, 784, 1), (393216, 768, 588, 1), (393216, 768, 832, 0), (393216, 768, 832, 1), (36864, 520, 520, 1), (36864, 520, 576, 1)]


def routes():
    out = []
    for r in ROUTES:
        try:
            n = _lib.route_count(r)
        except KeyError:                              # a route this build does not have
            continue
        if n:
            out.append(f"{r}:{n}")
    return " ".join(out)


def timeit(f):
    f(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); f(); e1.record(); torch.cuda.synchronize()
    n = max(3, min(100, int(40.0 / max(e0.elapsed_time(e1), 1e-3))))      # ~40 ms of work per timed window
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


class Case:
    def __init__(self, M, N, K, nt_stream):
        self.M, self.N, self.K, self.nt_stream = M, N, K, nt_stream
        g = torch.Generator(device=dev).manual_seed(K)
        self.x = torch.randn(M, K, device=dev, generator=g).to(BF)
        self.dy = torch.randn(M, N, device=dev, generator=g).to(BF)
        self.w = torch.nn.Parameter(torch.randn(N, K, device=dev, generator=g) * K ** -0.5)
        self.b = torch.nn.Parameter(torch.zeros(N, device=dev))
        self.wT = ops.weights.get((self.w,), BF, True)
        self.dx = torch.empty(M, K, device=dev, dtype=BF)
        # what backward holds of x: the K-padded copy where ops.linear made one
        self.xs = ops._k_pad(self.x, self.w)[0] if HAS_TAIL else self.x
        self.dw = torch.zeros(N, self.xs.shape[1], device=dev)
        self.db = torch.zeros(N, device=dev)

    def fwd(self):
        with torch.no_grad():
            return ops.linear(self.x, self.w, self.b)

    def bwd_dx(self):
        check(lib.meant_linear_bwd_dx(self.dy.data_ptr(), self.N, self.wT.data_ptr(), self.dx.data_ptr(), self.K, self.M, self.N, self.K, BF16,
                                      torch.cuda.current_stream().cuda_stream), "linear_bwd_dx")

    def bwd_dw(self):
        ops._bwd_dw(self.dy, self.xs, self.dw, self.db)
        return ops._pad_cols(self.dw, self.K) if self.xs.shape[1] != self.K else self.dw


print(f"bf16 Linear, K-tail probe; median of {ROUNDS} rounds, rows interleaved; TFLOP/s = 2 M N K / time; tail kernels in this build: {HAS_TAIL}")
print("     M     N     K stream | op      ms   TFLOP/s | routes")
cases = [Case(*c) for c in CASES]
OPS = ("fwd", "bwd_dx", "bwd_dw")
names, times = {}, {}
for c in cases:                                        # warm-up and which kernels ran
    for op in OPS:
        _lib.set_option("nt_stream", c.nt_stream)
        _lib.route_reset(); getattr(c, op)(); torch.cuda.synchronize()
        names[(c, op)] = routes()
        times[(c, op)] = []
for _ in range(ROUNDS):
    for c in cases:
        _lib.set_option("nt_stream", c.nt_stream)
        for op in OPS:
            times[(c, op)].append(timeit(getattr(c, op)))
_lib.set_option("nt_stream", 1)
for c in cases:
    for op in OPS:
        ms = statistics.median(times[(c, op)])
        tf = 2.0 * c.M * c.N * c.K / ms / 1e9
        print(f"{c.M:6d} {c.N:5d} {c.K:5d} {c.nt_stream:6d} | {op:6s} {ms:7.3f} {tf:8.1f} | {names[(c, op)]}", flush=True)
