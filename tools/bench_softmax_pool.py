#!/usr/bin/env python3
"""The learned softmax pooling (ops.softmax_pool; csrc/softpool.hip) on one MI355X against the same function in ATen ops on the
device, and its two pool kernels against the mean-pool kernels they stand beside.
    python tools/bench_softmax_pool.py [--out profiles/softmax_pool_probe.txt] [--windows 7]
Shapes: x bf16 [640, 128, 768] and [640, 512, 768] (128 samples x lag 5), and [640, 128, 772] for the element forms.
  (a) fused   ops.softmax_pool forward + backward through autograd (gradients of x and of the six parameters)
  (b) ATen    F.linear -> F.layer_norm -> F.gelu -> F.linear -> softmax over the sequence -> weighted sum, bf16 activations,
              fp32 parameters cast per call, forward + backward
A window is a host clock around `calls` back-to-back calls that ends in a device synchronise; the two sides take turns window by
window in one process; every figure is the median over the windows with the lowest and highest beside it.  The claim under test is
"every fused window below every ATen window": the line `claim` says whether it held, the ratio of the medians stands beside it.
Then the kernels alone (device events around back-to-back calls of the entry points), bytes/s over the algorithmic bytes and the
share of HBM's 8 TB/s: meant_softmax_pool_fwd (x read once) beside meant_meanpool_fwd (x read once); meant_softmax_pool_bwd (x read
once, dx written once) beside meant_meanpool_bwd (dx written once); meant_ln_gelu_dot_fwd (h read once) and _bwd (h read once, dh
written once)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

HBM_PEAK = 8.0e12


def spread(xs, fmt="%.3f"):
    return (fmt + " (" + fmt + " .. " + fmt + ")") % (statistics.median(xs), min(xs), max(xs))


def window_ms(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def device_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def alternate(fns, calls, windows, timer):
    res = {name: [] for name, _ in fns}
    for _ in range(windows):
        for name, fn in fns:
            res[name].append(timer(fn, calls))
    return res


def aten_pool(x, w1, b1, gamma, beta, w2, b2):
    dt = x.dtype
    h = F.linear(x, w1.to(dt), b1.to(dt))
    n = F.layer_norm(h, (x.shape[-1],), gamma.to(dt), beta.to(dt), 1e-5)
    s = F.linear(F.gelu(n), w2.to(dt), b2.to(dt))
    w = torch.softmax(s.float(), dim=1).to(dt)
    return (w * x).sum(dim=1, dtype=torch.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    import meant_amd
    from meant_amd import ops, _lib as L
    lib = L.lib
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/bench_softmax_pool.py  windows={args.windows} calls/window={args.calls}  device={torch.cuda.get_device_name(0)}")
    for (G, S, d) in [(640, 128, 768), (640, 512, 768), (640, 128, 772)]:
        g = torch.Generator(device="cpu").manual_seed(0)
        x = torch.randn(G, S, d, generator=g).to(dev, torch.bfloat16).requires_grad_(True)
        prm = [torch.randn(d, d, generator=g) / d ** 0.5, 0.1 * torch.randn(d, generator=g), 1 + 0.1 * torch.randn(d, generator=g),
               0.1 * torch.randn(d, generator=g), torch.randn(1, d, generator=g) / d ** 0.5, 0.1 * torch.randn(1, generator=g)]
        prm = [p.to(dev).requires_grad_(True) for p in prm]
        dout = torch.randn(G, d, generator=g).to(dev)

        def step(f):
            def run():
                x.grad = None
                for p in prm:
                    p.grad = None
                f(x, *prm).backward(dout)
            return run

        fused, aten = step(ops.softmax_pool), step(aten_pool)
        for f in (fused, aten):                           # warm-up: code objects, the weight cache, ATen's algorithm choices
            for _ in range(3):
                f()
        a, b = ops.softmax_pool(x, *prm).detach(), aten_pool(x, *prm).detach()
        say(f"\n## x bf16 [{G}, {S}, {d}]   forward + backward, ms per call: median (min .. max)")
        say(f"   max |fused - ATen| of the pooled output: {(a - b).abs().max().item():.3e}")
        res = alternate([("fused", fused), ("aten", aten)], args.calls, args.windows, window_ms)
        say(f"   fused  {spread(res['fused'])}")
        say(f"   ATen   {spread(res['aten'])}")
        held = max(res["fused"]) < min(res["aten"])
        say(f"   claim  every fused window below every ATen window: {'HELD' if held else 'NOT HELD'};  "
            f"ATen / fused (medians) = {statistics.median(res['aten']) / statistics.median(res['fused']):.2f}")

        # ---- the kernels alone ----
        st = torch.cuda.current_stream().cuda_stream
        T, e = G * S, 2
        xd = x.detach()
        h = torch.randn(T, d, generator=g).to(dev, torch.bfloat16)
        gam, bet, w2, b2 = (prm[2].detach(), prm[3].detach(), prm[4].detach().view(-1), prm[5].detach())
        score = torch.empty(T, device=dev)
        stats = torch.empty(T, 2, device=dev)
        w = torch.empty(G, S, device=dev)
        out = torch.empty(G, d, device=dev)
        dx, dh = torch.empty_like(xd), torch.empty_like(h)
        ds = torch.empty(G, S, device=dev)
        dg, db, dw2 = (torch.empty(d, device=dev) for _ in range(3))
        wsb = lib.meant_ln_gelu_dot_bwd_ws(T, d)
        ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
        P = lambda t: t.data_ptr()
        kern = [
            ("meant_softmax_pool_fwd", T * d * e, lambda: lib.meant_softmax_pool_fwd(P(xd), P(score), None, 0, P(w), P(out), d, 0, G, S, d, L.BF16, L.F32, st)),
            ("meant_meanpool_fwd    ", T * d * e, lambda: lib.meant_meanpool_fwd(P(xd), P(out), d, 0, G, S, d, L.BF16, L.F32, st)),
            ("meant_softmax_pool_bwd", 2 * T * d * e, lambda: lib.meant_softmax_pool_bwd(P(dout), d, 0, P(xd), P(w), P(dx), P(ds), G, S, d, L.BF16, L.F32, st)),
            ("meant_meanpool_bwd    ", T * d * e, lambda: lib.meant_meanpool_bwd(P(dout), d, 0, P(dx), G, S, d, L.BF16, L.F32, st)),
            ("meant_ln_gelu_dot_fwd ", T * d * e, lambda: lib.meant_ln_gelu_dot_fwd(P(h), P(gam), P(bet), P(w2), P(b2), P(score), P(stats), T, d, 1e-5, L.BF16, st)),
            ("meant_ln_gelu_dot_bwd ", 2 * T * d * e, lambda: lib.meant_ln_gelu_dot_bwd(P(ds), P(h), P(stats), P(gam), P(bet), P(w2), P(dh), P(dg), P(db), P(dw2), T, d,
                                                                                         L.BF16, P(ws), wsb, st)),
        ]
        for _, _, fn in kern[4:5] + kern[:4] + kern[5:]:  # warm-up, in an order that fills score / stats / w before their readers
            assert fn() == 0, lib.meant_last_error()
        res = alternate([(name, fn) for name, _, fn in kern], args.calls, args.windows, device_ms)
        say("   kernels alone, device events: ms median (min .. max) | algorithmic GB | TB/s at the median | share of 8 TB/s")
        for name, nbytes, _ in kern:
            med = statistics.median(res[name])
            say(f"   {name}  {spread(res[name])} | {nbytes / 1e9:.3f} | {nbytes / (med * 1e-3) / 1e12:.2f} | {100 * nbytes / (med * 1e-3) / HBM_PEAK:.0f} %")
        torch.cuda.empty_cache()

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
