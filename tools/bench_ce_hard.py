#!/usr/bin/env python3
"""Hard-label cross-entropy with class weights and label smoothing on one MI355X (meant_ce_probs_hard, meant_softmax_ce_hard_fwd /
_bwd) against ATen's F.cross_entropy with the same arguments and against this library's routes without them.
    python tools/bench_ce_hard.py [--out profiles/ce_hard_probe.txt] [--windows 7]
Shapes: the class head on float32 probabilities at [128, 2], [128, 3129] and [4096, 3129]; the vocabulary head on bfloat16 logits
[8192, 64001] in the 64256-wide buffer of the vocabulary GEMM.  Loss, forward + backward through autograd into the input's .grad
(ms per call), with weight = random positive class weights and label_smoothing = 0.1:
  (a) the new route        cross_entropy_on_probs(p, y, weight=, label_smoothing=)  /  ops.softmax_cross_entropy(x, y, weight=, label_smoothing=)
  (b) ATen                 F.cross_entropy(p, y, weight=, label_smoothing=) on the device
  (c) the plain route      the same wrappers without the arguments: meant_ce_probs / meant_softmax_ce_fwd + _bwd (another loss: context)
A window is a host clock around `calls` back-to-back calls that ends in a device synchronise; the sides of a comparison take
turns window by window in one process; every figure is the median over the windows with the lowest and highest beside it.
Then the kernels alone (device events around back-to-back calls of the entry points): time, bytes/s over the algorithmic bytes
(class head: probs read once, the gradient written once; vocabulary forward: the logits read once; backward: read once, written
once) and the share of HBM's 8 TB/s."""
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
EPS = 0.1


def spread(xs, fmt="%.3f"):
    return (fmt + " (" + fmt + " .. " + fmt + ")") % (statistics.median(xs), min(xs), max(xs))


def window_ms(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def alternate(fns, calls, windows):
    """one window of each side in turn, `windows` times: {name: [ms per call]}"""
    res = {name: [] for name, _, _ in fns}
    for _ in range(windows):
        for name, fn, div in fns:
            res[name].append(window_ms(fn, max(1, calls // div)))
    return res


def alternate_device(fns, calls, windows):
    """the same with device events around each window: {name: [ms per call]}"""
    res = {name: [] for name, _ in fns}
    for _ in range(windows):
        for name, fn in fns:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            res[name].append(a.elapsed_time(b) / calls)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ce_hard_probe.txt"))
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    from meant_amd import _lib, ops
    from meant_amd.train import cross_entropy_on_probs
    assert torch.cuda.is_available(), "this probe measures on an MI355X"
    dev = torch.device("cuda")
    W = args.windows
    lib, st = _lib.lib, ops._stream()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def rate(name, t, nbytes):
        r = nbytes / (statistics.median(t) * 1e-3)
        say("  %-46s %s ms, %.1f MB algorithmic, %.2f TB/s, %.1f %% of HBM's 8 TB/s" % (name, spread(t, "%.4f"), nbytes / 1e6, r / 1e12, 100 * r / HBM_PEAK))

    prop = torch.cuda.get_device_properties(0)
    say("Hard-label cross-entropy with class weights and label smoothing, tools/bench_ce_hard.py; %s, %d CUs, torch %s, %s; one process,"
        % (prop.name, prop.multi_processor_count, torch.__version__, time.strftime("%Y-%m-%d")))
    say("one visit to a machine shared with other work.  Every figure: median (lowest .. highest) over %d windows, the sides of a row" % W)
    say("alternating.  weight = 0.25 + 1.75 * rand per class, label_smoothing = %.1f." % EPS)
    gen = torch.Generator(device=dev).manual_seed(0)

    # ---- the class head ------------------------------------------------------------------------------------------------------
    for B, C, calls in ((128, 2, 400), (128, 3129, 400), (4096, 3129, 100)):
        probs = torch.rand(B, C, device=dev, generator=gen).requires_grad_(True)
        y = torch.randint(0, C, (B,), device=dev, generator=gen)
        w = 0.25 + 1.75 * torch.rand(C, device=dev, generator=gen)

        def step(loss_fn, **kw):
            def run():
                probs.grad = None
                loss_fn(probs, y, **kw).backward()
            return run

        ours, aten, plain = step(cross_entropy_on_probs, weight=w, label_smoothing=EPS), step(F.cross_entropy, weight=w, label_smoothing=EPS), \
            step(cross_entropy_on_probs)
        for fn in (ours, aten, plain):
            for _ in range(3):
                fn()
        _lib.route_reset()
        ours()
        plain()
        assert _lib.route_count("ce_hard_wave") + _lib.route_count("ce_hard_block") == 1 and _lib.route_count("ce_probs") == 1
        a = cross_entropy_on_probs(probs.detach(), y, weight=w, label_smoothing=EPS).item()
        b = F.cross_entropy(probs.detach().double(), y, weight=w.double(), label_smoothing=EPS).item()
        assert abs(a - b) <= 1e-6 * max(1.0, abs(b)), (a, b)
        say()
        say("class head [%d, %d] float32, %d calls per window, ms per call:" % (B, C, calls))
        r = alternate([("a", ours, 1), ("b", aten, 1), ("c", plain, 4 if C > 1000 else 1)], calls, W)
        say("  loss forward + backward  (a) new route %-28s (b) ATen %-28s (c) plain route %s" % (spread(r["a"]), spread(r["b"]), spread(r["c"])))
        say("                           (a) / (b) of the medians: %.2f   (a) / (c): %.2f"
            % (statistics.median(r["a"]) / statistics.median(r["b"]), statistics.median(r["a"]) / statistics.median(r["c"])))
        out = probs.detach()
        buf = torch.empty(ops.CE_STATS_FLOATS + 2 * B, device=dev)
        dp = torch.empty(B, C, device=dev)
        acc = torch.zeros(1, device=dev)
        base, n = buf.data_ptr(), ops.CE_STATS_FLOATS

        def hard(eps, wt):
            return lambda: _lib.check(lib.meant_ce_probs_hard(out.data_ptr(), C, y.data_ptr(), ops._p(wt), eps, -100, base + 4 * n, base + 4 * (n + B),
                                                              dp.data_ptr(), C, B, C, base, st))

        def old():
            _lib.check(lib.meant_ce_probs(out.data_ptr(), y.data_ptr(), acc.data_ptr(), dp.data_ptr(), B, C, st))
        r = alternate_device([("hs", hard(EPS, w)), ("h0", hard(0.0, w)), ("old", old)], calls, W)
        rate("meant_ce_probs_hard, weight + smoothing (2 launches)", r["hs"], 8 * B * C)
        rate("meant_ce_probs_hard, weight alone (2 launches)", r["h0"], 8 * B * C)
        rate("meant_ce_probs", r["old"], 8 * B * C)

    # ---- the vocabulary head -------------------------------------------------------------------------------------------------
    T, V, ld, calls = 8192, 64001, 64256, 4
    x = (torch.randn(T, ld, device=dev, generator=gen) * 3).bfloat16()
    xv = x[:, :V].detach().requires_grad_(True)                       # what a caller without the padded buffer holds: re-homed by the wrapper
    y = torch.randint(0, V, (T,), device=dev, generator=gen)
    y[torch.rand(T, device=dev, generator=gen) < 0.85] = -100         # the MLM collator labels 15 % of the positions
    w = 0.25 + 1.75 * torch.rand(V, device=dev, generator=gen)
    rows, roww, stat, lse = torch.empty(T, device=dev), torch.empty(T, device=dev), torch.empty(T, 4, device=dev), torch.empty(T, 2, device=dev)
    blk, g = torch.empty(ops.CE_STATS_FLOATS, device=dev), torch.full((1,), 1e-3, device=dev)
    dl = torch.empty_like(x)
    F32, BF16 = _lib.F32, _lib.BF16

    def fwd_hard(eps, wt):
        return lambda: _lib.check(lib.meant_softmax_ce_hard_fwd(x.data_ptr(), ld, y.data_ptr(), ops._p(wt), eps, T, V, -100, rows.data_ptr(),
                                                                roww.data_ptr(), stat.data_ptr(), blk.data_ptr(), BF16, st))

    def bwd_hard(eps, wt):
        return lambda: _lib.check(lib.meant_softmax_ce_hard_bwd(x.data_ptr(), ld, y.data_ptr(), ops._p(wt), eps, stat.data_ptr(), T, V, -100,
                                                                g.data_ptr(), dl.data_ptr(), BF16, st))

    def fwd_old():
        _lib.check(lib.meant_softmax_ce_fwd(x.data_ptr(), ld, y.data_ptr(), T, V, -100, rows.data_ptr(), lse.data_ptr(), BF16, st))

    def bwd_old():
        _lib.check(lib.meant_softmax_ce_bwd(x.data_ptr(), ld, y.data_ptr(), lse.data_ptr(), T, V, -100, g.data_ptr(), dl.data_ptr(), BF16, st))
    say()
    for frac, note in ((0.15, "15 % of the rows labelled (the MLM collator's share)"), (1.0, "every row labelled")):
        if frac == 1.0:
            y = torch.randint(0, V, (T,), device=dev, generator=gen)
        nlab = int(((y >= 0) & (y < V)).sum())
        say("vocabulary head [%d, %d] bfloat16 in a %d-wide buffer, %s (%d rows), %d calls per window, kernels alone:" % (T, V, ld, note, nlab, calls))
        for fn in (fwd_hard(EPS, w), fwd_hard(0.0, w), fwd_old, bwd_hard(EPS, w), bwd_hard(0.0, w), bwd_old):
            fn()
        r = alternate_device([("fs", fwd_hard(EPS, w)), ("f0", fwd_hard(0.0, w)), ("fo", fwd_old)], calls, W)
        # the new forward reads the rows that count alone; the plain one reads every row
        rate("meant_softmax_ce_hard_fwd, weight + smoothing", r["fs"], 2 * nlab * V)
        rate("meant_softmax_ce_hard_fwd, weight alone", r["f0"], 2 * nlab * V)
        rate("meant_softmax_ce_fwd", r["fo"], 2 * T * V)
        say("    forward, new / plain of the medians: weight + smoothing %.3f, weight alone %.3f"
            % (statistics.median(r["fs"]) / statistics.median(r["fo"]), statistics.median(r["f0"]) / statistics.median(r["fo"])))
        r = alternate_device([("bs", bwd_hard(EPS, w)), ("b0", bwd_hard(0.0, w)), ("bo", bwd_old)], calls, W)
        nb = 2 * nlab * V + 2 * T * ld
        rate("meant_softmax_ce_hard_bwd, weight + smoothing", r["bs"], nb)
        rate("meant_softmax_ce_hard_bwd, weight alone", r["b0"], nb)
        rate("meant_softmax_ce_bwd", r["bo"], nb)
        say("    backward, new / plain of the medians: weight + smoothing %.3f, weight alone %.3f"
            % (statistics.median(r["bs"]) / statistics.median(r["bo"]), statistics.median(r["b0"]) / statistics.median(r["bo"])))
    del dl

    def vstep(loss_fn, inp, **kw):
        def run():
            inp.grad = None
            loss_fn(inp, y, **kw).backward()
        return run
    xp = x.detach().requires_grad_(True)                              # the padded buffer itself, as vocab_linear_cross_entropy hands it over

    def padded(inp, tgt, **kw):
        return ops._softmax_ce(inp, tgt, V, -100, kw.get("weight"), kw.get("label_smoothing", 0.0), "bench")
    ours, aten, plain = vstep(padded, xp, weight=w, label_smoothing=EPS), vstep(F.cross_entropy, xv, weight=w.bfloat16(), label_smoothing=EPS), \
        vstep(padded, xp)
    for fn in (ours, aten, plain):
        fn()
    b = F.cross_entropy(xv.detach()[:256].double(), y[:256], weight=w.double(), label_smoothing=EPS).item()
    a256 = padded(xp.detach()[:256], y[:256], weight=w, label_smoothing=EPS).item()
    assert abs(a256 - b) <= 1e-6 * max(1.0, abs(b)), (a256, b)
    say("vocabulary head, every row labelled, loss forward + backward through autograd, %d calls per window, ms per call:" % calls)
    r = alternate([("a", ours, 1), ("b", aten, 1), ("c", plain, 1)], calls, W)
    say("  (a) new route %-28s (b) ATen %-28s (c) plain route %s" % (spread(r["a"]), spread(r["b"]), spread(r["c"])))
    say("  (a) / (b) of the medians: %.2f   (a) / (c): %.2f"
        % (statistics.median(r["a"]) / statistics.median(r["b"]), statistics.median(r["a"]) / statistics.median(r["c"])))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
