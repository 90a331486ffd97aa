#!/usr/bin/env python3
"""Classification counts on one MI355X (meant_metrics_update, meant_amd.f1_metrics): what an update costs against the same counts
made with ATen on the device and against the reference loop's `.cpu()` + host counting, and what the wave-per-row kernel reads
per second on wide rows against a plain device copy of the same bytes.
    python tools/bench_metrics.py [--out profiles/metrics_probe.txt] [--windows 5] [--steps 12] [--batch 128] [--no-step-loop]
Sections:
  class head  [128, 2] f32: device time per update (events around a window of back-to-back calls) and host time per call (the
              enqueue), for f1_metrics.update, for argmax + bincount with ATen, and for .cpu() + numpy counting.
  step loop   the benchmark's train step (bench.py's model and batch) run as a loop that never reads the device, with
              TrainStep(metrics=m), and with the reference's per-step `out.cpu()` + `torch.isnan(out).any()` + host counting:
              ms per step of each, i.e. the stall the host reads put into the loop.
  wide rows   [4096, 3136] bf16 (meant_vqa's answers, padded) and [8192, 64008] bf16 (an MLM block, V = 64001): time per update, bytes
              of the class columns per second, the same for dst.copy_(src) (which reads AND writes those bytes).
  atomics     the wave-per-row kernel with every row ignored and with every row in one class: what its integer atomics cost.
Every figure is the median over --windows windows, with the lowest and highest beside it."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
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


def host_counts(out_cpu, target_cpu, C, state):
    """the counts the seven torchmetrics objects of the reference keep, made on the host"""
    pred = out_cpu.argmax(dim=1).numpy()
    t = target_cpu.numpy()
    state[:C] += np.bincount(pred[pred == t], minlength=C)
    state[C:2 * C] += np.bincount(pred, minlength=C)
    state[2 * C:3 * C] += np.bincount(t, minlength=C)
    state[3 * C] += len(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_probe.txt"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=12, help="train steps per window of the step loop")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--no-step-loop", action="store_true")
    ap.add_argument("--no-mlm", action="store_true", help="leave out the 1 GiB MLM block")
    args = ap.parse_args()
    import meant_amd
    from meant_amd import f1_metrics, _lib
    dev = torch.device("cuda")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    prop = torch.cuda.get_device_properties(0)
    say("Classification counts on the device, tools/bench_metrics.py; %s, %d CUs, torch %s; one process, one visit to a machine shared with"
        % (prop.name, prop.multi_processor_count, torch.__version__))
    say("other work.  Every figure: median (lowest .. highest) over %d windows." % args.windows)
    W = args.windows

    # ---- class head --------------------------------------------------------------------------------------------------------
    B, C = 128, 2
    g = torch.Generator().manual_seed(0)
    out = torch.rand(B, C, generator=g).to(dev)
    tgt = torch.randint(0, C, (B,), generator=g).to(dev)
    m = f1_metrics(C, "Train", device=dev)
    tgt_cpu = tgt.cpu()
    hstate = np.zeros(3 * C + 4, dtype=np.int64)

    def upd():
        m.update(out, tgt)

    def aten():
        pred = out.argmax(dim=1)
        return torch.bincount(tgt * C + pred, minlength=C * C)          # the confusion counts: tp, npred, ntarget are its sums

    def ref():
        o = out.detach().cpu()
        assert not torch.isnan(out).any()                                # in_loop_train.py:228
        host_counts(o, tgt_cpu, C, hstate)

    for fn in (upd, aten, ref):
        for _ in range(20):
            fn()
    _lib.route_reset()
    upd()
    assert _lib.route_count("metrics_rows") == 1
    say()
    say("Class head, out [128, 2] f32 and target [128] on the device, 2000 calls per window (us per call):")
    say("                                             device time              host time")
    say("  f1_metrics.update (one launch)          %-24s %s" % (spread(device_us(upd, 2000, W)), spread(host_us(upd, 2000, W))))
    say("  ATen argmax + bincount on the device    %-24s %s   (bincount reads its result size back: a host sync per call)"
        % (spread(device_us(aten, 2000, W)), spread(host_us(aten, 2000, W, sync_each=True))))
    say("  .cpu() + isnan().any() + host counting  %-24s %s   (two host syncs per call, idle device)"
        % ("-", spread(host_us(ref, 2000, W, sync_each=True))))

    # ---- the stall in a loop of train steps -----------------------------------------------------------------------------------
    if not args.no_step_loop:
        import bench
        from meant_amd.train import TrainStep
        model = bench.build_model(1, dev).train()
        inputs, target = bench.make_batch(args.batch, 0, dev)
        target_cpu = target.cpu()
        mm = f1_metrics(2, "Train", device=dev)
        plain = TrainStep(model)
        hs = np.zeros(3 * 2 + 4, dtype=np.int64)

        def loop(kind, n):
            ts = plain
            ts.metrics = mm if kind == "device" else None
            for _ in range(n):
                _, o = ts(*inputs, target=target)
                if kind == "reference":
                    oc = o.detach().cpu()
                    assert not torch.isnan(o).any()
                    host_counts(oc, target_cpu, 2, hs)

        res = {k: [] for k in ("none", "device", "reference")}
        loop("none", 3)
        for _ in range(W):
            for kind in res:                                              # the three alternate inside every window
                loop(kind, 1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loop(kind, args.steps)
                torch.cuda.synchronize()
                res[kind].append((time.perf_counter() - t0) * 1e3 / args.steps)
        say()
        say("Train step of bench.py (meant, 1 encoder, %d samples, bf16, TrainStep with clip + AdamW), %d steps per window, the three loops"
            % (args.batch, args.steps))
        say("alternating (ms per step):")
        say("  no metrics, nothing read                       %s" % spread(res["none"]))
        say("  TrainStep(metrics=m), nothing read             %s" % spread(res["device"]))
        say("  out.cpu() + isnan(out).any() + host counting   %s" % spread(res["reference"]))
        say("  difference of medians to the first line: device %+.3f ms, reference loop %+.3f ms"
            % (statistics.median(res["device"]) - statistics.median(res["none"]),
               statistics.median(res["reference"]) - statistics.median(res["none"])))
        del model, plain, inputs
        torch.cuda.empty_cache()

    # ---- wide rows ----------------------------------------------------------------------------------------------------------
    say()
    say("Wide rows, bf16, every row labelled (GB/s = bytes of the class columns per second; the copy reads and writes them):")
    say("  shape                     us per update            GB/s read     us per dst.copy_(src)    GB/s read (+ as much written)    update / copy")
    shapes = [(4096, 3129, 3136)] + ([] if args.no_mlm else [(8192, 64001, 64008)])
    for Bw, Cw, ld in shapes:
        src = torch.randn(Bw, ld, device=dev, dtype=torch.bfloat16)
        dst = torch.empty_like(src)
        t = torch.randint(0, Cw, (Bw,), device=dev)
        mw = f1_metrics(Cw, "MLM", device=dev)
        view = src[:, :Cw]
        calls = 200 if Bw * ld < (1 << 26) else 20
        for _ in range(3):
            mw.update(view, t)
            dst.copy_(src)
        _lib.route_reset()
        mw.update(view, t)
        assert _lib.route_count("metrics_wave") == 1
        u = device_us(lambda: mw.update(view, t), calls, W)
        c = device_us(lambda: dst.copy_(src), calls, W)
        nbytes = Bw * Cw * 2
        gbs = lambda us: nbytes / (us * 1e-6) / 1e9
        say("  [%5d, %5d] ld %5d   %-24s %-13.0f %-24s %-32.0f %.2f"
            % (Bw, Cw, ld, spread(u), gbs(statistics.median(u)), spread(c), gbs(statistics.median(c)), statistics.median(u) / statistics.median(c)))
        assert mw.state[3 * Cw].item() == Bw * (calls * W + 4)
        del src, dst
    # ---- what the atomics cost ------------------------------------------------------------------------------------------------
    say()
    say("Atomics of the wave-per-row kernel, [B, 3129] bf16 ld 3136 at the C ABI (us per call): random targets; every target the ignore")
    say("index (no row is read: the launch and one row-counter atomic per workgroup); every target class 0 (one address for every row's")
    say("ntarget atomic):")
    st = torch.cuda.current_stream().cuda_stream
    for Bw in (4096, 65536):
        Cw, ld = 3129, 3136
        src = torch.randn(Bw, ld, device=dev, dtype=torch.bfloat16)
        state = torch.zeros(3 * Cw + 4, dtype=torch.int64, device=dev)
        targets = (torch.randint(0, Cw, (Bw,), device=dev), torch.full((Bw,), -100, dtype=torch.int64, device=dev),
                   torch.zeros(Bw, dtype=torch.int64, device=dev))
        call = lambda t: (lambda: _lib.lib.meant_metrics_update(src.data_ptr(), ld, 1, t.data_ptr(), Bw, Cw, -100, state.data_ptr(), None, st))
        res = []
        for t in targets:
            for _ in range(3):
                call(t)()
            res.append(spread(device_us(call(t), 200, W)))
        say("  B = %5d   random %-26s ignored %-26s one class %s" % (Bw, res[0], res[1], res[2]))
        del src
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
