#!/usr/bin/env python3
"""Soft-target cross-entropy and the VQA score on one MI355X (meant_ce_probs_soft, meant_vqa_score_update) against what torch
offers for the same lines of the VQA loop (vqa.py:173,209,223).
    python tools/bench_ce_soft.py [--out profiles/ce_soft_probe.txt] [--windows 7]
Shapes: [128, 3129] (meant_vqa's batch), [4096, 3129] as a column view of a 3136-wide block, [8192, 64001] in a 64008-wide block.
Loss, forward + backward through autograd into probs.grad (ms per call):
  (a) cross_entropy_on_probs(probs, soft)           the new route
  (b) F.cross_entropy(probs, soft)                   ATen on the device
  (c) cross_entropy_on_probs(probs, soft.argmax(1))  the integer-target kernel at the same shape, for context only
Score (ms per call):
  (d) vqa_score.update(out, soft)        against  soft.gather(1, out.argmax(1, keepdim=True)).sum()  on the device
  (e) the same against out.cpu() first, then the same line on the host (the reference loop's hand-over)
A window is a host clock around `calls` back-to-back calls that ends in a device synchronise; the sides of a comparison take
turns window by window in one process; every figure is the median over the windows with the lowest and highest beside it.
Then the kernels alone (device events around back-to-back calls of the entry points): time, bytes/s over the algorithmic bytes
(loss: probs and target read once, the gradient written once; score: the scores read once) and the share of HBM's 8 TB/s."""
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


def alternate(fns, calls, windows):
    """one window of each side in turn, `windows` times: {name: [ms per call]}"""
    res = {name: [] for name, _, _ in fns}
    for _ in range(windows):
        for name, fn, div in fns:
            res[name].append(window_ms(fn, max(1, calls // div)))
    return res


def device_ms(fn, calls, windows):
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return out


def soft_targets(B, C, ld, dev, gen):
    """[B, C] view of a [B, ld] block: per row 0-4 answer columns with weights 0.3 / 0.6 / 0.9 / 1.0"""
    block = torch.zeros(B, ld, device=dev)
    cols = torch.randint(0, C, (B, 4), device=dev, generator=gen)
    w = torch.tensor([0.3, 0.6, 0.9, 1.0], device=dev)[torch.randint(0, 4, (B, 4), device=dev, generator=gen)]
    keep = torch.arange(4, device=dev)[None, :] < torch.randint(0, 5, (B, 1), device=dev, generator=gen)
    block.scatter_(1, cols, w * keep)
    return block[:, :C]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ce_soft_probe.txt"))
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    from meant_amd import _lib, ops, vqa_score
    from meant_amd.train import cross_entropy_on_probs
    assert torch.cuda.is_available(), "this probe measures on an MI355X"
    dev = torch.device("cuda")
    W = args.windows
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    prop = torch.cuda.get_device_properties(0)
    say("Soft-target cross-entropy and the VQA score, tools/bench_ce_soft.py; %s, %d CUs, torch %s, %s; one process, one visit to a"
        % (prop.name, prop.multi_processor_count, torch.__version__, time.strftime("%Y-%m-%d")))
    say("machine shared with other work.  Every figure: median (lowest .. highest) over %d windows, the sides of a row alternating." % W)
    gen = torch.Generator(device=dev).manual_seed(0)
    for B, C, ld, calls in ((128, 3129, 3129, 400), (4096, 3129, 3136, 100), (8192, 64001, 64008, 4)):
        probs = torch.rand(B, ld, device=dev, generator=gen)[:, :C].requires_grad_(True)       # a leaf that is a column view
        soft = soft_targets(B, C, ld, dev, gen)
        hard = soft.argmax(1)
        soft_cpu = soft.cpu()

        def step(loss_fn, target):
            def run():
                probs.grad = None
                loss_fn(probs, target).backward()
            return run

        ours, aten, ints = step(cross_entropy_on_probs, soft), step(F.cross_entropy, soft), step(cross_entropy_on_probs, hard)
        out = probs.detach()
        m = vqa_score("probe", device=dev)
        score = lambda: m.update(out, soft)
        score_aten = lambda: soft.gather(1, out.argmax(1, keepdim=True)).sum()
        score_host = lambda: soft_cpu.gather(1, out.cpu().argmax(1, keepdim=True)).sum()
        for fn in (ours, aten, ints, score, score_aten):
            for _ in range(3):
                fn()
        score_host()
        _lib.route_reset()
        ours()
        score()
        assert _lib.route_count("ce_soft_block") == 1 and _lib.route_count("vqa_score") == 1
        a, b = cross_entropy_on_probs(out, soft).item(), F.cross_entropy(out.double(), soft.double()).item()
        assert abs(a - b) <= 1e-6 * max(1.0, abs(b)), (a, b)

        say()
        say("[%d, %d]%s, %d calls per window, ms per call:" % (B, C, "" if ld == C else " in a %d-wide block" % ld, calls))
        r = alternate([("a", ours, 1), ("b", aten, 1), ("c", ints, 4)], calls, W)
        say("  loss forward + backward  (a) soft route %-28s (b) ATen %-28s (c) integer route %s" % (spread(r["a"]), spread(r["b"]), spread(r["c"])))
        say("                           (a) / (b) of the medians: %.2f" % (statistics.median(r["a"]) / statistics.median(r["b"])))
        r = alternate([("d", score, 1), ("g", score_aten, 1)], calls, W)
        say("  score                    (d) vqa_score  %-28s     ATen %-28s (d) / ATen: %.2f"
            % (spread(r["d"]), spread(r["g"]), statistics.median(r["d"]) / statistics.median(r["g"])))
        r = alternate([("d", score, 1), ("e", score_host, 8)], calls, max(3, W // 2))
        say("                           (d) vqa_score  %-28s (e) out.cpu() + host %-28s" % (spread(r["d"]), spread(r["e"])))

        # the kernels alone
        rows = torch.empty(B + 1, device=dev)
        dp = torch.empty(B, C, device=dev)
        td = soft

        def entry():
            _lib.check(_lib.lib.meant_ce_probs_soft(out.data_ptr(), ld, td.data_ptr(), ld, 0, rows.data_ptr(), rows.data_ptr() + 4 * B, dp.data_ptr(),
                                                    C, B, C, ops._stream()))
        for name, fn, nbytes in (("meant_ce_probs_soft (both launches)", entry, 12 * B * C), ("meant_vqa_score_update", score, 4 * B * C + 4 * B)):
            t = device_ms(fn, calls, W)
            rate = nbytes / (statistics.median(t) * 1e-3)
            say("  %-36s %s ms, %.1f MB algorithmic, %.2f TB/s, %.1f %% of HBM's 8 TB/s"
                % (name, spread(t, "%.4f"), nbytes / 1e6, rate / 1e12, 100 * rate / HBM_PEAK))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
