#!/usr/bin/env python3
"""dev probe: the temporal (lag-axis) attention core, forward and backward, at B = 128, H = 12, Dh = 128 for
L in {12, 64, 65, 128, 512} in both tiers, through meant_temporal_attn_fwd / _bwd.  L <= 64 runs the one-wave kernels of
temporal.hip, L > 64 its long-lag kernels; at L <= 64 the long-lag kernels are timed as well (library
option "temporal_long" = 1, toggled here), interleaved with the short ones: the one like-for-like comparison there is.
MEANT_PROBE_LONG_AT_SHORT=0 (read only here) leaves those rows out.

Per row: median ms of ROUNDS interleaved rounds and the kv traffic the shapes imply over that time, as GB/s and as a share of
the 8 TB/s HBM peak: forward reads K and V once (B L 2D elements); backward reads K and V once and writes dkv once (twice that;
the long-lag backward reads V a second time only past L = 2048).  q, o, dq and the fp32 p [B, H, L] are left out (< 2 %).
kv smaller than the 256 MiB Infinity Cache is re-read on-die between repetitions: the MB column says which rows those are.
usage: python tools/probe_temporal_lag.py [B, default 128]"""
import math, os, statistics, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from meant_amd import _lib
from meant_amd._lib import lib, check
dev = torch.device("cuda")
st = torch.cuda.current_stream().cuda_stream
B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
H, Dh, ROUNDS, PEAK = 12, 128, 5, 8e12
D = H * Dh
LONG_AT_SHORT = os.environ.get("MEANT_PROBE_LONG_AT_SHORT", "1") == "1"


def timeit(f):
    f(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); f(); e1.record(); torch.cuda.synchronize()
    n = max(5, min(200, int(30.0 / max(e0.elapsed_time(e1), 1e-3))))      # ~30 ms of work per timed window
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


print(f"temporal core, B {B} H {H} Dh {Dh}; median of {ROUNDS} interleaved rounds; share = kv bytes / time / 8 TB/s")
print("tier  L    kernel  kv MB |  fwd ms   GB/s  share |  bwd ms   GB/s  share | max |diff| vs short: o, dq, dkv")
for dtype, name, code in ((torch.float32, "f32 ", 0), (torch.bfloat16, "bf16", 1)):
    for L in (12, 64, 65, 128, 512):
        scale = 1.0 / math.sqrt(D)
        q = torch.randn(B, D, device=dev).to(dtype); kv = torch.randn(B * L, 2 * D, device=dev).to(dtype)
        do = torch.randn(B, D, device=dev).to(dtype)
        variants = (["short"] if L <= 64 else []) + (["long"] if L > 64 or LONG_AT_SHORT else [])
        buf = {v: dict(o=torch.empty_like(q), p=torch.empty(B, H, L, device=dev), dq=torch.empty_like(q), dkv=torch.empty_like(kv))
               for v in variants}

        def fwd(v):
            b = buf[v]
            check(lib.meant_temporal_attn_fwd(q.data_ptr(), kv.data_ptr(), b["o"].data_ptr(), b["p"].data_ptr(), B, L, H, Dh, scale, code, st))

        def bwd(v):
            b = buf[v]
            check(lib.meant_temporal_attn_bwd(q.data_ptr(), kv.data_ptr(), b["p"].data_ptr(), do.data_ptr(), b["dq"].data_ptr(),
                                              b["dkv"].data_ptr(), B, L, H, Dh, scale, code, st))

        for v in variants:                                                   # which kernels ran, and warm-up
            _lib.set_option("temporal_long", 1 if v == "long" else 0)
            _lib.route_reset(); fwd(v); bwd(v); torch.cuda.synchronize()
            assert _lib.route_count("temporal_long") == (2 if v == "long" else 0), (v, L)
        tf, tb = {v: [] for v in variants}, {v: [] for v in variants}
        for _ in range(ROUNDS):
            for v in variants:
                _lib.set_option("temporal_long", 1 if v == "long" else 0)
                tf[v].append(timeit(lambda: fwd(v))); tb[v].append(timeit(lambda: bwd(v)))
        _lib.set_option("temporal_long", 0)
        kvb = kv.numel() * kv.element_size()
        for v in variants:
            mf, mb = statistics.median(tf[v]), statistics.median(tb[v])
            gf, gb = kvb / mf / 1e6, 2 * kvb / mb / 1e6
            line = (f"{name} {L:4d} {v:>7s} {kvb / 1e6:7.1f} | {mf:7.4f} {gf:6.0f} {gf * 1e9 / PEAK:6.1%} | {mb:7.4f} {gb:6.0f} {gb * 1e9 / PEAK:6.1%}")
            if v == "long" and "short" in buf:
                d = [(buf["long"][k].float() - buf["short"][k].float()).abs().max().item() for k in ("o", "dq", "dkv")]
                line += f" | {d[0]:.1e} {d[1]:.1e} {d[2]:.1e}"
            print(line, flush=True)
        del q, kv, do, buf
        torch.cuda.empty_cache()
