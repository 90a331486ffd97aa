#!/usr/bin/env python3
"""The optimizer tail on one MI355X at the benchmark model's parameter count, buckets as TrainStep makes them (64 MB).
    python tools/bench_optim_guard.py [--out profiles/optim_guard_probe.txt] [--windows 7] [--calls 20]
Three tails over their own copy of the parameters, with the same gradients, taking turns window by window in one process:
  (a) FusedAdamW.step()        meant_sumsq_f32 per bucket (float atomics), meant_adamw_f32 per bucket        the existing tail
  (b) GuardedAdam.step()       meant_grad_stats_f32 per bucket, meant_optim_step_f32 per bucket, meant_optim_finish
  (c) the reference's lines on torch: clip_grad_norm_ on the scaled gradients, GradScaler.step(AdamW(foreach=True)), GradScaler.update()
A window is a host clock around `calls` back-to-back steps that ends in a device synchronise; every figure is the median over the
windows with the lowest and highest beside it.  Bytes per step: 4 per parameter for the statistics, 28 for the update.
Then the norm pass alone (device events): meant_sumsq_f32 with `deterministic` 0 and 1 against meant_grad_stats_f32, over all buckets.
Launches per step: (a) and (b) from the calls they make, (c) counted by torch.profiler over one step."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch

HBM_PEAK = 8.0e12
V, D, H, L, IMG, P, C, NCLS = 64001, 768, 12, 12, 224, 16, 4, 2          # bench.py's headline model


def spread(xs, fmt="%.3f"):
    return (fmt + " (" + fmt + " .. " + fmt + ")") % (statistics.median(xs), min(xs), max(xs))


def window_ms(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_guard_probe.txt"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="a 2-layer toy instead of the benchmark model (a rehearsal of the script, not a measurement)")
    args = ap.parse_args()
    import meant_amd
    from meant_amd import _lib, ops
    from meant_amd.parallel import GradReducer
    from meant_amd.train import FusedAdamW, GuardedAdam
    assert torch.cuda.is_available(), "this probe measures on an MI355X"
    dev = torch.device("cuda")
    W, calls = args.windows, args.calls
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    if args.small:
        model = meant_amd.meant(128, 128, 4, 32, 32, 16, 3, 2, torch.nn.Embedding(100, 128), num_heads=2)
    else:
        model = meant_amd.meant(D, D, 4, IMG, IMG, P, L, NCLS, torch.nn.Embedding(V, D), num_heads=H, num_encoders=1, channels=C)
    shapes = [tuple(p.shape) for p in model.parameters() if p.requires_grad]
    del model
    gen = torch.Generator(device=dev).manual_seed(0)
    start = [torch.randn(s, device=dev, generator=gen) * 0.02 for s in shapes]
    hyper = dict(lr=5e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)

    def params():
        return [torch.nn.Parameter(t.clone()) for t in start]
    pa, pb, pc = params(), params(), params()
    ra, rb = GradReducer(pa, bucket_mb=64.0), GradReducer(pb, bucket_mb=64.0)
    fused = FusedAdamW(ra, max_grad_norm=1.0, **hyper)
    guarded = GuardedAdam(rb, kind="adamw", max_grad_norm=1.0, clip_scaled=True, loss_scale="dynamic", **hyper)
    for ba, bb in zip(ra.buckets, rb.buckets):
        ba.flat.normal_(0.0, 1e-3, generator=gen)
        bb.flat.copy_(ba.flat).mul_(guarded.get_scale())
    for p, q in zip(pc, pa):
        p.grad = (q.grad * 65536.0).clone()
    topt = torch.optim.AdamW(pc, foreach=True, **hyper)
    scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)
    scaler.scale(torch.ones(1, device=dev))

    def torch_step():
        torch.nn.utils.clip_grad_norm_(pc, 1.0)
        scaler.step(topt)
        scaler.update()
        # (the gradients stay clipped for the next call: every later call clips by 1, the same launches)

    n = sum(b.flat.numel() for b in ra.buckets)
    k = ra.num_buckets
    prop = torch.cuda.get_device_properties(0)
    say("The optimizer tail, tools/bench_optim_guard.py; %s, %d CUs, torch %s, %s; one process, one visit to a machine shared with"
        % (prop.name, prop.multi_processor_count, torch.__version__, time.strftime("%Y-%m-%d")))
    say("other work.  %d parameters%s (%.1f MB of gradients, bucket padding included) in %d buckets of at most 64 MB: %s elements."
        % (sum(t.numel() for t in start), " (--small: a rehearsal, not a measurement)" if args.small else "", 4 * n / 1e6, k,
           ", ".join(str(b.flat.numel()) for b in ra.buckets)))
    say("Every figure: median (lowest .. highest) over %d windows of %d steps, the variants alternating window by window." % (W, calls))

    for fn in (fused.step, guarded.step, torch_step):
        for _ in range(3):
            fn()
    assert guarded.steps_skipped() == 0 and guarded.steps_taken() == 3
    res = {"a": [], "b": [], "c": []}
    for _ in range(W):
        res["a"].append(window_ms(fused.step, calls))
        res["b"].append(window_ms(guarded.step, calls))
        res["c"].append(window_ms(torch_step, max(1, calls // 4)))
    say()
    say("ms per step, bytes/s over 32 B per parameter (4 read by the norm pass, 28 moved by the update), launches per step:")
    launches = {"a": "%d (1 fill, %d sumsq, %d adamw)" % (1 + 2 * k, k, k),
                "b": "%d (%d x 2 grad_stats, %d optim_step, 1 finish)" % (3 * k + 1, k, k), "c": "see below"}
    names = {"a": "(a) FusedAdamW.step()", "b": "(b) GuardedAdam.step()", "c": "(c) torch GradScaler + clip + foreach AdamW"}
    for key in "abc":
        rate = 32.0 * n / (statistics.median(res[key]) * 1e-3)
        say("  %-46s %-30s %.2f TB/s (%.0f %% of HBM's 8 TB/s)   launches: %s"
            % (names[key], spread(res[key]), rate / 1e12, 100 * rate / HBM_PEAK, launches[key]))
    say("  (b) / (a) of the medians: %.3f;  (c) / (b): %.2f" % (statistics.median(res["b"]) / statistics.median(res["a"]),
                                                                 statistics.median(res["c"]) / statistics.median(res["b"])))
    save()

    # the norm pass alone
    st = ops._stream()
    acc = torch.zeros(1, device=dev)

    def sumsq():
        for b in ra.buckets:
            _lib.check(_lib.lib.meant_sumsq_f32(b.flat.data_ptr(), b.flat.numel(), acc.data_ptr(), st))

    def stats():
        for i, b in enumerate(rb.buckets):
            _lib.check(_lib.lib.meant_grad_stats_f32(b.flat.data_ptr(), b.flat.numel(), guarded.state.data_ptr(), int(i == 0),
                                                     guarded._ws.data_ptr(), guarded._ws.numel(), st))
    say()
    say("the norm pass alone over the %d buckets (device events, %d calls per window), bytes/s over 4 B per parameter:" % (k, calls))
    old = _lib.get_option("deterministic")
    rows = []
    try:
        for name, fn, det, c in (("meant_sumsq_f32, deterministic = 0 (float atomics)", sumsq, 0, calls),
                                 ("meant_sumsq_f32, deterministic = 1 (one workgroup)", sumsq, 1, max(1, calls // 10)),
                                 ("meant_grad_stats_f32 (ordered, either value)", stats, 1, calls)):
            _lib.set_option("deterministic", det)
            fn()
            rows.append((name, device_ms(fn, c, W)))
    finally:
        _lib.set_option("deterministic", old)
    for name, t in rows:
        rate = 4.0 * n / (statistics.median(t) * 1e-3)
        say("  %-52s %s ms   %.3f TB/s (%.1f %% of HBM's 8 TB/s)" % (name, spread(t, "%.4f"), rate / 1e12, 100 * rate / HBM_PEAK))
    save()

    # launches of the torch variant
    say()
    try:
        from torch.profiler import profile, ProfilerActivity
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            torch_step()
            torch.cuda.synchronize()
        nk = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        say("launches of one step of (c), device activities counted by torch.profiler: %d" % nk)
    except Exception as e:                                                    # the figure is then missing, and the file says so
        say("launches of one step of (c): not measured (torch.profiler: %s)" % (str(e).splitlines()[0] if str(e) else type(e).__name__))
    save()


if __name__ == "__main__":
    main()
