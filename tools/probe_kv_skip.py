#!/usr/bin/env python3
"""dev probe: the GEMMs around the text stack's key-masked attention with option "kv_skip" on and off, timed directly at the benchmark's
text shape (M = 1536 x 512 = 786432 token rows, q|k|v = 2304 columns, d = 768).

Masks: `bench` (bench.make_batch: a trailing pad drawn uniformly from [0, 384) per sequence), `pad0` (no padding: the lists are full, the
option must cost nothing) and `pad75` (384 trailing pads of 512 in every sequence).  Per product and mask: off and on take turns within
every round; printed are the median, the fastest and the slowest of ROUNDS rounds and on / off of the medians.  The dY operand of the
weight gradient carries exact zeros in the k|v columns of the dead blocks, as the attention backward leaves them.
  dW : off = meant_linear_bwd_dw over all rows and 2304 columns; on = the q columns over all rows + the k|v columns over the live blocks
  fwd: off = meant_qkv_proj_fwd (one launch, rotary epilogue); on = meant_qkv_proj_fwd_live (q over all row panels, k|v over the live
       ones, zero fill of the dead ones)
usage: python tools/probe_kv_skip.py [rounds, default 7]"""
import os, statistics, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
import meant_amd
from meant_amd import _lib, ops
from meant_amd._lib import lib, check, BF16

dev = torch.device("cuda")
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
BF = torch.bfloat16
G, S, D = 1536, 512, 768
M, N, K = G * S, 3 * D, D


def timeit(f, n=6):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def mask_of(kind):
    m = np.ones((G, S), dtype=np.float32)
    pad = {"bench": np.random.RandomState(99).randint(0, 384, G), "pad0": np.zeros(G, dtype=np.int64), "pad75": np.full(G, 384)}[kind]
    for g in range(G):
        if pad[g]:
            m[g, S - pad[g]:] = 0
    return torch.from_numpy(m).to(dev)


gen = torch.Generator(device=dev).manual_seed(1)
x = torch.randn(M, K, device=dev, generator=gen).to(BF)
dy = torch.randn(M, N, device=dev, generator=gen).to(BF)
dw = torch.zeros(N, K, device=dev)
db = torch.zeros(N, device=dev)
w = (torch.randn(N, K, device=dev, generator=gen) * K ** -0.5).to(BF)
bias = torch.randn(N, device=dev, generator=gen) * 0.1
qa, qb, ka, kb = meant_amd.RotaryEmbedding(dim=48, use_xpos=True).tables(S, dev)
qkv = torch.empty(M, N, device=dev, dtype=BF)
H, Dh, R = 12, 64, qa.shape[1]
print(f"kv_skip probe at (M, N, K) = ({M}, {N}, {K}); {ROUNDS} rounds, off / on interleaved; ms: median [fastest .. slowest]")
for kind in ("pad0", "bench", "pad75"):
    km = mask_of(kind)
    lists = ops.kv_live_rows(km, True)
    nlive, npan, ndead = lists[:3].tolist()
    live = torch.zeros(M // 64, dtype=torch.bool, device=dev)
    live[lists[ops.KV_LIST_HEADER:ops.KV_LIST_HEADER + nlive].long()] = True
    dyk = dy.clone()
    dyk.view(M // 64, 64, N)[~live, :, D:] = 0

    def dw_off():
        ops._bwd_dw(dyk, x, dw, db)

    def dw_on():
        ops._bwd_dw(dyk[:, :D], x, dw[:D], db[:D])
        ops._bwd_dw_rows(dyk[:, D:], x, dw[D:], db[D:], lists)

    def fwd_off():
        check(lib.meant_qkv_proj_fwd(x.data_ptr(), K, w.data_ptr(), bias.data_ptr(), qkv.data_ptr(), M, K, S, H, Dh, R, qa.data_ptr(), qb.data_ptr(),
                                     ka.data_ptr(), kb.data_ptr(), BF16, torch.cuda.current_stream().cuda_stream), "qkv_proj_fwd")

    def fwd_on():
        check(lib.meant_qkv_proj_fwd_live(x.data_ptr(), K, w.data_ptr(), bias.data_ptr(), qkv.data_ptr(), M, K, S, H, Dh, R, qa.data_ptr(), qb.data_ptr(),
                                          ka.data_ptr(), kb.data_ptr(), lists.data_ptr(), BF16, torch.cuda.current_stream().cuda_stream), "qkv_proj_fwd_live")

    # same sums (the "+=" contract: from zero, once each)
    dw.zero_(); db.zero_(); dw_off(); ref_w, ref_b = dw.clone(), db.clone()
    dw.zero_(); db.zero_(); dw_on()
    ew = ((dw - ref_w).abs().max() / ref_w.abs().max()).item()
    eb = ((db - ref_b).abs().max() / ref_b.abs().max()).item()
    print(f"{kind:6s}: live blocks {nlive}/{M // 64} ({100.0 * nlive / (M // 64):.1f} %), live panels {npan}/{M // 256}; "
          f"dW on vs off: max |diff| / max |dW| = {ew:.2e}, db {eb:.2e}")
    times = {"dW off": [], "dW on": [], "fwd off": [], "fwd on": []}
    for f in (dw_off, dw_on, fwd_off, fwd_on): f()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        times["dW off"].append(timeit(dw_off))
        times["dW on"].append(timeit(dw_on))
        times["fwd off"].append(timeit(fwd_off))
        times["fwd on"].append(timeit(fwd_on))
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        print(f"  {k:7s} {med[k]:7.3f} [{min(v):7.3f} .. {max(v):7.3f}]", flush=True)
    print(f"  dW on / off = {med['dW on'] / med['dW off']:.3f}, fwd on / off = {med['fwd on'] / med['fwd off']:.3f}", flush=True)
    del dyk
