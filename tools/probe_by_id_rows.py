#!/usr/bin/env python
"""dev probe: the kernels that move whole token rows by vocabulary id around the first text layer, at the benchmark step's shape
(T = 786 432 tokens in sequences of 512, V = 64 001, d = 768, 3 H Dh = 2304, 12 heads of 64, R = 48, uniform ids, every sequence's pad
length uniform in [0, 384)), through the C entry points that launch them:

  gather_rows     meant_gather_rows, bf16 rows of 768 out of the table image by id (gather_rows_kernel)
  emb_bwd_sorted  meant_embedding_bwd_sorted, bf16 rows of 768 (embedding_bwd_sorted_kernel: seg_walk)
  fwd_by_id       meant_qkv_embed_fwd_by_id, the whole route (norm on the table, NT GEMM, qkv_gather_kernel)
  bwd_by_id       meant_qkv_embed_bwd_by_id, both stages (qkv_seg_kernel, the table GEMMs, the table tail, the residual sum by id)

One line per entry: ms per call, median and min .. max over --reps timed calls after two warm-up calls, device events around each
call.  The two routes hold more than the kernel in question; for the kernels alone run the probe under `rocprofv3 --kernel-trace
--stats` and read the per-kernel averages (tools/rocprof_stats.py).  To compare two builds, run it in alternating processes with
MEANT_LIB_PATH naming each build's library.
    python tools/probe_by_id_rows.py [label] [--reps 9]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from meant_amd import _lib, ops  # noqa: E402

lib, p = _lib.lib, ops._p
T, V, D_MODEL, H, DH, R, S, EPS = 786432, 64001, 768, 12, 64, 48, 512, 1e-8
N3 = 3 * H * DH


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("label", nargs="?", default="build")
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    bf = lambda *shape: torch.randn(*shape, device=dev, generator=g).to(torch.bfloat16)
    ids = torch.randint(0, V, (T,), device=dev, generator=g)
    idx32 = ids.to(torch.int32)
    tb, dres, dqkv = bf(V, D_MODEL), bf(T, D_MODEL), bf(T, N3)
    w = (torch.randn(N3, D_MODEL, device=dev, generator=g) / D_MODEL ** 0.5).to(torch.bfloat16)
    wT = w.t().contiguous()
    bias = 0.1 * torch.randn(N3, device=dev, generator=g)
    gain = 1 + 0.1 * torch.randn(D_MODEL, device=dev, generator=g)
    rot = [torch.rand(S, R, device=dev, generator=g) * 2 - 1 for _ in range(4)]
    pad = np.random.RandomState(0).randint(0, 384, T // S)
    mask = torch.ones(T // S, S, device=dev)
    for i, n in enumerate(pad):
        if n:
            mask[i, S - n:] = 0
    lists = ops.kv_live_rows(mask, True)
    dead = (mask.view(-1, 64).sum(1) == 0).repeat_interleave(64)
    dqkv[dead, N3 // 3:] = 0
    s_ids, s_ord = ops._sort_ids(ids, V)
    st = ops._stream()

    x = torch.empty(T, D_MODEL, device=dev, dtype=torch.bfloat16)
    dtab = torch.zeros(V, D_MODEL, device=dev)
    qkv = torch.empty(T, N3, device=dev, dtype=torch.bfloat16)
    ws_f = torch.empty(lib.meant_qkv_embed_fwd_by_id_ws(T, D_MODEL, N3, V), device=dev, dtype=torch.uint8)
    ws_b = torch.empty(lib.meant_qkv_embed_bwd_by_id_ws(T, D_MODEL, N3, V), device=dev, dtype=torch.uint8)
    dw, db, dgain = torch.zeros(N3, D_MODEL, device=dev), torch.zeros(N3, device=dev), torch.empty(D_MODEL, device=dev)
    qa, qb, ka, kb = rot

    entries = {
        "gather_rows": lambda: _lib.check(lib.meant_gather_rows(p(tb), p(idx32), None, p(x), T, D_MODEL, _lib.BF16, st), "gather_rows"),
        "emb_bwd_sorted": lambda: _lib.check(lib.meant_embedding_bwd_sorted(p(dres), p(s_ids), p(s_ord), p(dtab), T, D_MODEL, V, _lib.BF16, st),
                                             "embedding_bwd_sorted"),
        "fwd_by_id": lambda: _lib.check(lib.meant_qkv_embed_fwd_by_id(p(tb), p(gain), EPS, p(w), p(bias), p(s_ids), p(s_ord), p(lists), p(qa), p(qb),
                                                                      p(ka), p(kb), p(qkv), T, S, D_MODEL, H, DH, R, V, p(ws_f), ws_f.numel(), st),
                                        "qkv_embed_fwd_by_id"),
        "bwd_by_id": lambda: _lib.check(lib.meant_qkv_embed_bwd_by_id(p(dqkv), p(dres), p(s_ids), p(s_ord), p(tb), p(gain), EPS, p(wT), p(lists), p(dw),
                                                                      p(db), p(dgain), p(dtab), T, D_MODEL, N3, V, 0, V,
                                                                      _lib.BY_ID_SHARED | _lib.BY_ID_TABLE, p(ws_b), ws_b.numel(), st),
                                        "qkv_embed_bwd_by_id"),
    }
    times = {k: [] for k in entries}
    for i in range(args.reps + 2):                           # the entries alternate; two warm-up rounds
        for k, f in entries.items():
            t = timed(f)
            if i >= 2:
                times[k].append(t)
    for k, v in times.items():
        print(f"{args.label} {k:15s} {statistics.median(v):8.4f} ms  ({min(v):.4f} .. {max(v):.4f})", flush=True)


if __name__ == "__main__":
    main()
