#!/usr/bin/env python3
"""dev probe for "Models at any width" (DESIGN section 6); writes profiles/any_width_probe.txt.

(a) bf16 Linear backward at an output width N that is no multiple of 8, both products (dX, dW + dbias) of one Linear:
      new route   ops._linear_bwd_npad: one meant_pad_copy2d pass dY -> [M, ceil8(N)], dX on the K-tail NT kernels with the cached
                  [K, ceil8(N)] transposed weight, dW / dbias on the TN kernels through padded accumulators (zeroed and cut back inside
                  the timed region)
      old route   meant_linear_bwd_dx / meant_linear_bwd_dw called with lddy = N: rows of dY are not 16-byte aligned, the C ABI takes
                  both on the exact-f32 engine -- what ops.linear's backward ran before, reproducible in the same build
    at N in {100, 588} with K = 768, M = 25088 (128 images of 196 patches) and N = 588 at M = 393216 (the 14 x 14 x 3 MIM decoder at
    128 samples x 12 days x 256 patches).  The two routes take turns inside each of ROUNDS rounds; per route the median and the
    run-to-run spread (max - min of the rounds); "wins" = the medians differ by more than the larger spread.
(b) one bf16 `meant` step (forward + backward, 8 samples, lag 12, 512 tokens, 224 x 224 images at patch 16, 8 heads, one encoder layer)
    at widths (772, 772) next to (768, 768).  Information only: the odd-width model is a correctness route.
usage: python tools/probe_any_width.py [rounds, default 5] [output file]"""
import os, statistics, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import meant_amd
from meant_amd import _lib, ops
from meant_amd._lib import lib, check, BF16

dev = torch.device("cuda")
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "any_width_probe.txt")
BF = torch.bfloat16
ROUTES = ("nt128k", "nt256k", "nt128", "nt256", "nt256s", "gemm_f32", "tn128", "tn256", "tn_tail")
CASES = [(25088, 100, 768), (25088, 588, 768), (393216, 588, 768)]
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def routes():
    return " ".join(f"{r}:{_lib.route_count(r)}" for r in ROUTES if _lib.route_count(r))


def timeit(f, budget_ms=40.0):
    f(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); f(); e1.record(); torch.cuda.synchronize()
    n = max(2, min(100, int(budget_ms / max(e0.elapsed_time(e1), 1e-3))))
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


class Case:
    def __init__(self, M, N, K):
        self.M, self.N, self.K = M, N, K
        g = torch.Generator(device=dev).manual_seed(N)
        self.x = torch.randn(M, K, device=dev, generator=g).to(BF)
        self.dy = torch.randn(M, N, device=dev, generator=g).to(BF)
        self.w = torch.nn.Parameter(torch.randn(N, K, device=dev, generator=g) * K ** -0.5)
        self.wT = ops.weights.get((self.w,), BF, True)

    def new(self):
        return ops._linear_bwd_npad(self.dy, self.x, (self.w,), True, True, 0, self.K)

    def old(self):
        M, N, K = self.M, self.N, self.K
        st = torch.cuda.current_stream().cuda_stream
        dx = torch.empty(M, K, device=dev, dtype=BF)
        check(lib.meant_linear_bwd_dx(self.dy.data_ptr(), N, self.wT.data_ptr(), dx.data_ptr(), K, M, N, K, BF16, st), "linear_bwd_dx")
        dw, db = torch.zeros(N, K, device=dev), torch.zeros(N, device=dev)
        check(lib.meant_linear_bwd_dw(self.dy.data_ptr(), N, self.x.data_ptr(), K, dw.data_ptr(), db.data_ptr(), M, N, K, BF16, None, 0, st), "linear_bwd_dw")
        return dx, dw, db


say(f"(a) bf16 Linear backward (dX + dW + dbias) at N % 8 != 0; median of {ROUNDS} rounds, routes interleaved; spread = max - min of the rounds")
say("     M     N     K | route     ms   spread | launches")
for M, N, K in CASES:
    c = Case(M, N, K)
    names, times = {}, {"new": [], "old": []}
    for r in ("new", "old"):
        _lib.route_reset(); out = getattr(c, r)(); torch.cuda.synchronize()
        names[r] = routes()
        if r == "new":
            keep = out
        else:                                             # the two routes compute the same thing
            for a, b, what in zip(keep, out, ("dx", "dw", "db")):
                e = (a.float() - b.float()).abs().max().item() / max(b.float().abs().max().item(), 1e-6)
                assert e < 2e-2, (what, e)
    del keep, out
    for _ in range(ROUNDS):
        for r in ("new", "old"):
            times[r].append(timeit(getattr(c, r)))
    med = {r: statistics.median(times[r]) for r in times}
    spr = {r: max(times[r]) - min(times[r]) for r in times}
    for r in ("new", "old"):
        say(f"{M:6d} {N:5d} {K:5d} | {r:5s} {med[r]:8.3f} {spr[r]:8.3f} | {names[r]}")
    wins = med["old"] - med["new"] > max(spr.values())
    say(f"{'':18s} | old / new = {med['old'] / med['new']:.2f}x; the new route {'wins' if wins else 'DOES NOT win'} by more than the spread")
    del c
    torch.cuda.empty_cache()

say()
say(f"(b) one bf16 meant step, forward + backward, 8 samples x lag 12, 512 tokens, 224 x 224 / 16, 8 heads; median of {ROUNDS} rounds, interleaved")
B, LAG, S, V = 8, 12, 512, 2000
g = torch.Generator().manual_seed(0)
ids = torch.randint(0, V, (B, LAG, S), generator=g).to(dev)
img = torch.randn(B, LAG, 4, 224, 224, generator=g).to(dev).to(BF)
mask = torch.ones(B, LAG, S, device=dev)
tgt = torch.randint(0, 2, (B,), generator=g).to(dev)
models = {}
for d in (768, 772):
    torch.manual_seed(d)
    m = meant_amd.meant(d, d, 4, 224, 224, 16, LAG, 2, torch.nn.Embedding(V, d), num_heads=8, num_encoders=1).to(dev).eval()
    m.compute_dtype = BF
    models[d] = m


def step(m):
    m.zero_grad(set_to_none=True)
    torch.nn.functional.cross_entropy(m(ids, img, mask), tgt).backward()


times = {d: [] for d in models}
for d, m in models.items():
    step(m); torch.cuda.synchronize()
for _ in range(ROUNDS):
    for d, m in models.items():
        times[d].append(timeit(lambda: step(m), budget_ms=400.0))
med = {d: statistics.median(times[d]) for d in times}
for d in times:
    say(f"widths ({d}, {d}): {med[d]:8.2f} ms  (spread {max(times[d]) - min(times[d]):.2f} ms)")
say(f"ratio 772 / 768 = {med[772] / med[768]:.2f}x (information only)")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
