#!/usr/bin/env python3
"""AUROC on one MI355X (meant_score_capture, meant_auroc_rank, meant_amd.auroc): what keeping the scores costs per step against
f1_metrics.update and against the `out.cpu()` a host-side AUROC needs every step, and what the exact statistic costs at the end
against copying the scores to the host and ranking them there.
    python tools/bench_auroc.py [--out profiles/auroc_probe.txt] [--windows 5]
Sections:
  update     out [128, 2] f32 and target [128] on the device: device time per call (events around a window of back-to-back calls)
             and host time per call (the enqueue) of auroc.update and f1_metrics.update; host time of out.cpu() (a host sync).
  statistic  n = 10^4 and 10^6 captured rows: auroc.statistic() (sort + scans on the device, one copy of three integers back,
             host clock around the call, which ends in that copy) against scores.cpu() + sklearn.metrics.roc_auc_score; the two
             values side by side.
Every figure is the median over --windows windows, with the lowest and highest beside it."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch


def spread(xs, fmt="%.2f"):
    return (fmt + " (" + fmt + " .. " + fmt + ")") % (statistics.median(xs), min(xs), max(xs))


def device_us(fn, calls, windows):
    """device time per call, us: events around `calls` back-to-back calls"""
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)
    return out


def host_us(fn, calls, windows, sync_each=False):
    """host time per call, us; with the device drained at the end of the window (sync_each: the call itself reads the device)"""
    out = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        if not sync_each:
            t1 = time.perf_counter()
        torch.cuda.synchronize()
        if sync_each:
            t1 = time.perf_counter()
        out.append((t1 - t0) * 1e6 / calls)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "auroc_probe.txt"))
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    from sklearn.metrics import roc_auc_score
    from meant_amd import auroc, f1_metrics, _lib
    dev = torch.device("cuda")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    prop = torch.cuda.get_device_properties(0)
    say("AUROC on the device, tools/bench_auroc.py; %s, %d CUs, torch %s; one process, one visit to a machine shared with other work."
        % (prop.name, prop.multi_processor_count, torch.__version__))
    say("Every figure: median (lowest .. highest) over %d windows." % args.windows)
    W = args.windows

    # ---- one update ---------------------------------------------------------------------------------------------------------
    B, C, calls = 128, 2, 2000
    g = torch.Generator().manual_seed(0)
    out = torch.rand(B, C, generator=g).to(dev)
    tgt = torch.randint(0, C, (B,), generator=g).to(dev)
    a = auroc(C, "Train", capacity=B * calls, device=dev)                   # a window fills it once: no growth inside the timing
    m = f1_metrics(C, "Train", device=dev)

    def cap():
        a.update(out, tgt)

    def f1():
        m.update(out, tgt)

    def ref():
        return out.detach().cpu()

    for fn in (cap, f1, ref):
        for _ in range(20):
            fn()
    a.reset()
    _lib.route_reset()
    cap()
    assert _lib.route_count("score_capture") == 1

    def timed(measure, fn, **kw):                                           # the buffer is emptied before every window
        res = []
        for _ in range(W):
            a.reset()
            res += measure(fn, calls, 1, **kw)
        return res

    say()
    say("One update, out [128, 2] f32 and target [128] on the device, %d calls per window (us per call):" % calls)
    say("                                             device time              host time")
    say("  auroc.update (one launch)               %-24s %s" % (spread(timed(device_us, cap)), spread(timed(host_us, cap))))
    say("  f1_metrics.update (one launch)          %-24s %s" % (spread(device_us(f1, calls, W)), spread(host_us(f1, calls, W))))
    say("  out.cpu()                               %-24s %s   (a host sync per call, idle device)"
        % ("-", spread(host_us(ref, calls, W, sync_each=True))))

    # ---- the statistic --------------------------------------------------------------------------------------------------------
    say()
    say("The statistic over n captured rows, binary, float32 scores rounded to three decimals (ties), ms per call; the device side is")
    say("auroc.statistic(): class codes, a 4-pass radix sort, tile sums + scan + apply, one copy of (2U, P, N) to the host:")
    say("  n          auroc.statistic()          scores.cpu() + roc_auc_score   value (device)        value (scikit-learn)")
    for n, reps in ((10 ** 4, 20), (10 ** 6, 5)):
        g = torch.Generator().manual_seed(n)
        t = torch.randint(0, 2, (n,), generator=g)
        s = ((torch.randn(n, generator=g) + t) * 1000).round() / 1000
        sd, td = s.to(dev), t.to(dev)
        obj = auroc(2, "Val", capacity=n, device=dev)
        obj.update(sd, td)
        for _ in range(3):
            obj.statistic()
        _lib.route_reset()
        stat = obj.statistic()
        assert _lib.route_count("auroc_rank") == 1
        t_np = t.numpy()

        def host():
            return roc_auc_score(t_np, sd.cpu().numpy().astype("float64"))

        host()
        ours = [x / 1e3 for x in host_us(obj.statistic, reps, W, sync_each=True)]
        theirs = [x / 1e3 for x in host_us(host, reps, W, sync_each=True)]
        value = auroc.from_statistic(stat)[0].item()
        say("  %-9d  %-26s %-30s %-21.15f %.15f" % (n, spread(ours, "%.3f"), spread(theirs, "%.3f"), value, host()))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
