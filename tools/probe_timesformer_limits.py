#!/usr/bin/env python3
"""dev probe: what lifting TimeSformer's width and length limits costs ("TimeSformer at any width and any video
length").  Takes no part in any test.

  1. the cls query's attention over key segments, meant_attn_cls_split_fwd / _bwd, at B = 4, H = 12, Dh = 64 for
     L in {18 817, 40 001, 100 001} with nseg = 0 (the library's count), both tiers; at L = 18 817, where the one-workgroup pair
     meant_attn_cls_fwd / _bwd still runs, that pair against nseg = 4 and nseg = 16 in alternating rounds.
     Bytes: the forward reads K and V once (B L 2 H Dh elements), the backward reads K and V and read-modify-writes dK and dV
     (three times that); q, out, stats and the workspace are left out (< 0.1 %).  Share = those bytes over the median time over
     the 6.3 TB/s a copy reaches on this part.
  2. one layer of TimeSformer forward + backward at dim = 772 against dim = 768 at the design shape (12 frames of 224 x 224,
     patch 16, 12 heads of 64, bf16 tier), alternating rounds.

usage: python tools/probe_timesformer_limits.py [--batch 32] [--skip-model]"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from meant_amd import _lib
from meant_amd._lib import lib, check

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--skip-model", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda")
st = torch.cuda.current_stream().cuda_stream
B, H, Dh, ROUNDS, COPY_BW = 4, 12, 64, 3, 6.3e12
D = H * Dh
scale = Dh ** -0.5


def timeit(f):
    f(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); f(); e1.record(); torch.cuda.synchronize()
    n = max(3, min(100, int(30.0 / max(e0.elapsed_time(e1), 1e-3))))      # ~30 ms of work per timed window
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


print(f"cls attention, B {B} H {H} Dh {Dh}; median of {ROUNDS} alternating rounds; share = bytes / time / 6.3 TB/s")
print("tier       L  kernel   segs f/b  kv MB |   fwd ms   GB/s  share |   bwd ms   GB/s  share | max |diff| vs one-workgroup: out, dqkv")
for dtype, name, code in ((torch.float32, "f32 ", 0), (torch.bfloat16, "bf16", 1)):
    for L in (18817, 40001, 100001):
        qkv = torch.randn(B, L, 3 * D, device=dev).to(dtype)
        dout = torch.randn(B, D, device=dev).to(dtype)
        both = L <= lib.meant_attn_cls_max_len(Dh, 1)
        variants = (["one-wg", "split4", "split16"] if both else []) + ["split0"]
        nseg = {"split0": 0, "split4": 4, "split16": 16}
        buf = {v: dict(out=torch.empty(B, D, device=dev, dtype=dtype), stats=torch.empty(B, H, 2, device=dev),
                       dqkv=torch.zeros_like(qkv)) for v in variants}
        wsb = max(lib.meant_attn_cls_split_ws(B, L, H, Dh, n) for n in (0, 4, 16))
        ws = torch.empty(wsb, device=dev, dtype=torch.uint8)

        def fwd(v):
            b = buf[v]
            if v == "one-wg":
                check(lib.meant_attn_cls_fwd(qkv.data_ptr(), b["out"].data_ptr(), D, b["stats"].data_ptr(), None, B, L, H, Dh, scale, code, st))
            else:
                check(lib.meant_attn_cls_split_fwd(qkv.data_ptr(), b["out"].data_ptr(), D, b["stats"].data_ptr(), None, B, L, H, Dh, scale,
                                                   nseg[v], code, ws.data_ptr(), wsb, st))

        def bwd(v):
            b = buf[v]
            if v == "one-wg":
                check(lib.meant_attn_cls_bwd(qkv.data_ptr(), b["out"].data_ptr(), D, dout.data_ptr(), D, b["stats"].data_ptr(), None,
                                             b["dqkv"].data_ptr(), B, L, H, Dh, scale, code, st))
            else:
                check(lib.meant_attn_cls_split_bwd(qkv.data_ptr(), b["out"].data_ptr(), D, dout.data_ptr(), D, b["stats"].data_ptr(), None,
                                                   b["dqkv"].data_ptr(), B, L, H, Dh, scale, nseg[v], code, ws.data_ptr(), wsb, st))

        diffs = {}
        for v in variants:                                                    # one clean pass each for the comparison, and warm-up
            buf[v]["dqkv"].zero_(); fwd(v); bwd(v); torch.cuda.synchronize()
            if v != "one-wg" and "one-wg" in buf:
                diffs[v] = [(buf[v][k].float() - buf["one-wg"][k].float()).abs().max().item() for k in ("out", "dqkv")]
        tf, tb = {v: [] for v in variants}, {v: [] for v in variants}
        for _ in range(ROUNDS):
            for v in variants:
                tf[v].append(timeit(lambda: fwd(v))); tb[v].append(timeit(lambda: bwd(v)))
        kvb = B * L * 2 * D * qkv.element_size()
        for v in variants:
            mf, mb = statistics.median(tf[v]), statistics.median(tb[v])
            gf, gb = kvb / mf / 1e6, 3 * kvb / mb / 1e6
            segs = "1/1" if v == "one-wg" else "/".join(str(nseg[v] or -(-L // lib.meant_attn_cls_max_len(Dh, a))) for a in (0, 1))
            line = (f"{name} {L:7d} {v:>8s} {segs:>8s} {kvb / 1e6:7.1f} | {mf:8.4f} {gf:6.0f} {gf * 1e9 / COPY_BW:6.1%} | "
                    f"{mb:8.4f} {gb:6.0f} {gb * 1e9 / COPY_BW:6.1%}")
            if v in diffs:
                line += f" | {diffs[v][0]:.1e} {diffs[v][1]:.1e}"
            print(line, flush=True)
        del qkv, dout, buf, ws
        torch.cuda.empty_cache()

if not args.skip_model:
    import meant_amd as M
    print(f"\none TimeSformer layer fwd+bwd, bf16, batch {args.batch}, 12 frames of 224 x 224, patch 16, 12 heads of 64; {ROUNDS} alternating rounds")
    models, video, grads = {}, torch.randn(args.batch, 12, 3, 224, 224, device=dev), {}
    for dim in (768, 772):
        m = M.TimeSformer(dim=dim, num_frames=12, num_classes=2, image_size=224, patch_size=16, channels=3, depth=1, heads=12, dim_head=64).to(dev)
        m.compute_dtype = torch.bfloat16
        models[dim] = m

    def step(dim):
        m = models[dim]
        for p in m.parameters():
            p.grad = None
        x = m.meant_forward(video)
        if dim not in grads:
            grads[dim] = torch.randn_like(x) / x.numel() ** 0.5
        x.backward(grads[dim])

    times = {768: [], 772: []}
    for dim in times:
        _lib.route_reset(); step(dim); step(dim); torch.cuda.synchronize()
        print(f"dim {dim}: rows_elem launches per step {_lib.route_count('rows_elem') // 2}")
    for _ in range(ROUNDS):
        for dim in times:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(3): step(dim)
            torch.cuda.synchronize(); times[dim].append((time.perf_counter() - t0) / 3 * 1e3)
    for dim in times:
        print(f"dim {dim}: ms per step {' '.join(f'{t:8.2f}' for t in times[dim])}   median {statistics.median(times[dim]):8.2f}")
    print(f"ratio 772 / 768: {statistics.median(times[772]) / statistics.median(times[768]):.2f}")
