#!/usr/bin/env python3
"""The pretraining collators on one MI355X (meant_mlm_mask, meant_patchify_raw_masked, meant_mim_l1_fwd / _bwd) against the two ways
the same lines of the pretraining loops can run today.
    python tools/bench_collate.py [--out profiles/collate_probe.txt] [--windows 5]
MLM collate, ids [64, 512] and [256, 512] (ms per call):
  dev   MLMCollator on device tensors (one launch)
  host  mlm_dataset.mask_tokens restated with torch on the CPU (special-token mask, torch.bernoulli, the two fills; the per-sample
        Python loop of the reference is NOT included, so this side is flattered) + the H2D copies of ids and labels
MIM data path, raw images [128, 4, 224, 224] in f32 / f64 / u8, decoder output [128, 3, 224, 224] bf16 (ms per call):
  (a) mim_dataset.mask_image on the host (normalise, torch.bernoulli per element, where, fill) + the two image-sized H2D copies
  (b) the raw batch on the device, the mask applied with ATen: normalise, torch.bernoulli, two torch.where, ops.patchify, then
      F.l1_loss forward + backward on the materialised labels[:, :3]
  (c) the fused pair: ops.patchify_masked, then ops.mim_l1_loss forward + backward; with bytes/s over the bytes the algorithm needs
      (patchify: raw in, bf16 patches out; loss forward: out and the first three raw planes in; backward: the same in, dout out)
One MIM step (forward + backward of meant_vision_pretrainer, 768 wide, bf16, batch 128) under (b) and under (c).
Every window is one JSON line; the sides of a comparison take turns window by window in one process after a warm-up; device windows
are device events around back-to-back calls, host windows a host clock that ends in a device synchronise; the call counts make a
window last from a hundred to a few hundred ms.  After each MIM row the three pieces of (c) -- the masked patchify, the loss forward, the
loss forward + backward -- are timed on their own the same way, with their rates over their own algorithmic bytes.  The summary quotes
the median with the lowest and highest window beside it: that spread is the margin any comparison here has."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

HBM_PEAK = 8.0e12
MEAN, STD, P = 0.3, 1.7, 0.15


def spread(xs, fmt="%.3f"):
    return (fmt + " (" + fmt + " .. " + fmt + ")") % (statistics.median(xs), min(xs), max(xs))


def host_ms(fn, calls):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collate_probe.txt"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    args = ap.parse_args()
    import meant_amd as M
    from meant_amd import data, ops
    assert torch.cuda.is_available(), "this probe measures on an MI355X"
    dev = torch.device("cuda")
    W = args.windows
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def alternate(section, shape, sides):
        """sides: (name, fn, calls, clock); one window of each in turn, W times, after a warm-up of each: {name: [ms per call]}"""
        for _, fn, _, _ in sides:
            fn()
            fn()
        res = {name: [] for name, _, _, _ in sides}
        for w in range(W):
            for name, fn, calls, clock in sides:
                ms = (device_ms if clock == "device" else host_ms)(fn, calls)
                res[name].append(ms)
                say(json.dumps(dict(section=section, shape=shape, side=name, window=w, calls=calls, clock=clock, ms_per_call=round(ms, 5))))
        return res

    prop = torch.cuda.get_device_properties(0)
    say("# Pretraining collators on the device, tools/bench_collate.py; %s, %d CUs, torch %s, %s; one process, one visit to a machine"
        % (prop.name, prop.multi_processor_count, torch.__version__, time.strftime("%Y-%m-%d")))
    say("# shared with other work.  One JSON line per window; summaries: median (lowest .. highest) over %d windows." % W)

    # ---- MLM ----------------------------------------------------------------------------------------------------------------------
    special, mask_id, vocab = (0, 1, 2, 3, 64000), 64000, 64001
    coll = data.MLMCollator(mask_id=mask_id, special_ids=special, vocab_size=vocab, seed=1)
    for B, S in ((64, 512), (256, 512)):
        ids_cpu = torch.randint(4, 64000, (B, S))
        ids_cpu[:, 0], ids_cpu[:, -1] = 0, 2
        am_cpu = torch.ones(B, S)
        ids, am = ids_cpu.to(dev), am_cpu.to(dev)
        spec_cpu = torch.tensor(special)

        def on_device():
            coll(ids, am)

        def on_host():
            labels = ids_cpu.clone()
            inputs = ids_cpu.clone()
            prob = torch.full(labels.shape, P)
            prob.masked_fill_(torch.isin(labels, spec_cpu), 0.0)
            chosen = torch.bernoulli(prob).bool()
            labels[~chosen] = -100
            inputs[chosen] = mask_id
            return inputs.to(dev), labels.to(dev)

        r = alternate("mlm_collate", [B, S], [("dev", on_device, 10000, "device"), ("host", on_host, 100, "host")])
        say("# MLM collate [%d, %d], ms per call: device kernel %s; host collator + H2D %s" % (B, S, spread(r["dev"], "%.4f"), spread(r["host"])))

    # ---- MIM data path --------------------------------------------------------------------------------------------------------------
    B, C, Co, H = args.batch, 4, 3, 224
    N, E = B * Co * H * H, B * C * H * H
    out = (torch.randn(B, Co, H, H, device=dev) * 2).to(torch.bfloat16).requires_grad_(True)
    for kind, dtype, size in (("f32", torch.float32, 4), ("f64", torch.float64, 8), ("u8", torch.uint8, 1)):
        raw_cpu = (torch.rand(B, C, H, H) * 255).to(dtype)
        raw = raw_cpu.to(dev)

        def a_host():
            x = (raw_cpu.float() - MEAN) / STD
            mask = torch.bernoulli(torch.full(x.shape, P)).bool()
            inputs = torch.where(mask, 0.0, x)
            x[~mask] = -100
            return inputs.to(dev), x.to(dev)

        def b_aten():
            x = (raw.float() - MEAN) / STD
            mask = torch.bernoulli(torch.full(x.shape, P, device=dev)).bool()
            inputs = torch.where(mask, 0.0, x)
            labels = torch.where(mask, x, -100.0)
            ops.patchify(inputs, 16, torch.bfloat16)
            out.grad = None
            F.l1_loss(out.float(), labels[:, :Co]).backward()

        def c_fused():
            ops.patchify_masked(raw, 16, torch.bfloat16, MEAN, STD, prob=P, seed=1)
            out.grad = None
            ops.mim_l1_loss(out, raw, prob=P, seed=1, mean=MEAN, std=STD).backward()

        r = alternate("mim_data_path", [B, C, H, H, kind], [("a", a_host, 1, "host"), ("b", b_aten, 500, "device"), ("c", c_fused, 1000, "device")])
        need = E * size + E * 2 + 2 * (N * 2 + N * size) + N * 2
        rate = need / (statistics.median(r["c"]) * 1e-3)
        say("# MIM data path [%d, %d, %d, %d] %s, ms per call: (a) host + 2 H2D %s; (b) ATen on the device %s; (c) fused %s"
            % (B, C, H, H, kind, spread(r["a"], "%.1f"), spread(r["b"]), spread(r["c"])))
        say("#   (c): %.1f MB algorithmic, %.2f TB/s, %.1f %% of HBM's 8 TB/s; (c) / (b) of the medians %.2f; highest (c) window %s lowest (b) window"
            % (need / 1e6, rate / 1e12, 100 * rate / HBM_PEAK, statistics.median(r["c"]) / statistics.median(r["b"]),
               "below" if max(r["c"]) < min(r["b"]) else "NOT below"))
        # the three pieces of (c) on their own, so that a rate describes a kernel and not the enqueue of four
        out_d = out.detach()

        def k_patchify():
            ops.patchify_masked(raw, 16, torch.bfloat16, MEAN, STD, prob=P, seed=1)

        def k_l1_fwd():
            ops.mim_l1_loss(out_d, raw, prob=P, seed=1, mean=MEAN, std=STD)

        def k_l1_both():
            out.grad = None
            ops.mim_l1_loss(out, raw, prob=P, seed=1, mean=MEAN, std=STD).backward()

        k = alternate("mim_pieces", [B, C, H, H, kind], [("patchify_masked", k_patchify, 1000, "device"), ("l1_fwd", k_l1_fwd, 1000, "device"),
                                                          ("l1_fwd_bwd", k_l1_both, 1000, "device")])
        for name, nbytes in (("patchify_masked", E * size + E * 2), ("l1_fwd", N * 2 + N * size), ("l1_fwd_bwd", 2 * (N * 2 + N * size) + N * 2)):
            t = statistics.median(k[name])
            say("#   %-16s %s ms, %.1f MB algorithmic, %.2f TB/s, %.1f %% of HBM's 8 TB/s"
                % (name, spread(k[name], "%.4f"), nbytes / 1e6, nbytes / (t * 1e-3) / 1e12, 100 * nbytes / (t * 1e-3) / HBM_PEAK))
        del raw, raw_cpu

    # ---- one MIM step -----------------------------------------------------------------------------------------------------------------
    torch.manual_seed(0)
    dec = torch.nn.Sequential(torch.nn.Conv2d(768, 16 * 16 * 3, kernel_size=1), torch.nn.PixelShuffle(16))
    m = M.meant_vision_pretrainer(1, dec, 768, patch_res=16, channels=4, height=H, width=H, image_dim=768, num_heads=8).to(dev)
    m.compute_dtype = torch.bfloat16
    raw = (torch.rand(B, C, H, H) * 255).to(torch.float64).to(dev)
    mim = data.MIMCollator(p=P, seed=1)
    pat = m.patchEmbed[0]

    def step_b():
        pat.set_normalization(0.0, 1.0)
        x = (raw.float() - MEAN) / STD
        mask = torch.bernoulli(torch.full(x.shape, P, device=dev)).bool()
        inputs = torch.where(mask, 0.0, x)
        labels = torch.where(mask, x, -100.0)
        m.zero_grad(set_to_none=True)
        F.l1_loss(m(inputs).float(), labels[:, :Co]).backward()

    def step_c():
        pat.set_normalization(MEAN, STD)
        m.zero_grad(set_to_none=True)
        m.loss(raw, mim).backward()

    r = alternate("mim_step", [B, C, H, H, "f64"], [("b", step_b, 100, "device"), ("c", step_c, 100, "device")])
    say("# One MIM step (768 wide, bf16, raw f64 [%d, %d, %d, %d]), ms: (b) ATen mask + forward + F.l1_loss + backward %s; (c) m.loss(raw, collator) + backward %s"
        % (B, C, H, H, spread(r["b"]), spread(r["c"])))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
