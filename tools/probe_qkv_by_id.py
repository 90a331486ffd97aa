#!/usr/bin/env python
"""Where does the by-id backward of the first text layer (meant_qkv_embed_bwd_by_id) overtake the per-token sequence?

For T / V in --ratios (V = 64001 rows of d = 768, 3 H Dh = 2304, sequences of 512 tokens, uniform ids -- the worst case for repeats --
and --pad of every sequence's keys padded) both routes run on the same operands, interleaved, --reps times each after a warm-up:
  per token   dX GEMM of the q|k|v projection, dW over q and over the live k|v rows, RMSNorm backward with the residual gradient,
              meant_embedding_bwd_sorted
  by id       the one entry point (segmented sum, table-sized GEMMs and norm backward, residual gradient summed by id)
Times are device events around each route's launches (its output allocations included, the same for both); the table prints the
median and the min .. max of the repetitions.
    python tools/probe_qkv_by_id.py [--ratios 1,2,4,8,12] [--reps 7] [--pad 0.37]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from meant_amd import _lib, ops  # noqa: E402

lib, p = _lib.lib, ops._p
V, D_MODEL, N3, S, EPS = 64001, 768, 2304, 512, 1e-8


def operands(T, pad, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    bf = lambda *shape: torch.randn(*shape, device=dev, generator=g).to(torch.bfloat16)
    c = dict(T=T)
    c["ids"] = torch.randint(0, V, (T,), device=dev, generator=g)
    c["tb"], c["dres"], c["dqkv"] = bf(V, D_MODEL), bf(T, D_MODEL), bf(T, N3)
    c["wT"] = (torch.randn(D_MODEL, N3, device=dev, generator=g) / D_MODEL ** 0.5).to(torch.bfloat16)
    c["gain"] = torch.ones(D_MODEL, device=dev)
    mask = torch.ones(T // S, S, device=dev)
    mask[:, S - int(pad * S):] = 0
    c["lists"] = ops.kv_live_rows(mask, True)
    dead = (mask.view(-1, 64).sum(1) == 0).repeat_interleave(64)
    c["dqkv"][dead, N3 // 3:] = 0
    c["sorted"] = ops._sort_ids(c["ids"], V)
    c["x"] = c["tb"][c["ids"]].contiguous()
    c["n"], c["sc"], c["rinv"] = ops._rmsnorm_fwd_raw(c["x"], c["gain"], EPS, 0.0, 0)
    return c


def per_token(c, dev):
    T, D = c["T"], N3 // 3
    dn = torch.empty(T, D_MODEL, device=dev, dtype=torch.bfloat16)
    _lib.check(lib.meant_linear_bwd_dx(p(c["dqkv"]), N3, p(c["wT"]), p(dn), D_MODEL, T, N3, D_MODEL, _lib.BF16, ops._stream()), "linear_bwd_dx")
    dw, db = torch.zeros(N3, D_MODEL, device=dev), torch.zeros(N3, device=dev)
    ops._bwd_dw(c["dqkv"][:, :D], c["n"], dw[:D], db[:D])
    ops._bwd_dw_rows(c["dqkv"][:, D:], c["n"], dw[D:], db[D:], c["lists"])
    dx, _ = ops._rmsnorm_bwd_raw(dn, c["x"], c["sc"], c["rinv"], EPS, 0.0, 0, dres=c["dres"])
    dtab = torch.zeros(V, D_MODEL, device=dev)
    _lib.check(lib.meant_embedding_bwd_sorted(p(dx), p(c["sorted"][0]), p(c["sorted"][1]), p(dtab), T, D_MODEL, V, _lib.BF16, ops._stream()),
               "embedding_bwd_sorted")


def by_id(c, dev, ws):
    T = c["T"]
    dw, db = torch.zeros(N3, D_MODEL, device=dev), torch.zeros(N3, device=dev)
    dgain, dtab = torch.empty(D_MODEL, device=dev), torch.zeros(V, D_MODEL, device=dev)
    _lib.check(lib.meant_qkv_embed_bwd_by_id(p(c["dqkv"]), p(c["dres"]), p(c["sorted"][0]), p(c["sorted"][1]), p(c["tb"]), p(c["gain"]), EPS,
                                             p(c["wT"]), p(c["lists"]), p(dw), p(db), p(dgain), p(dtab), T, D_MODEL, N3, V, 0, V,
                                             _lib.BY_ID_SHARED | _lib.BY_ID_TABLE, p(ws), ws.numel(), ops._stream()), "qkv_embed_bwd_by_id")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ratios", default="1,2,4,8,12")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pad", type=float, default=0.37)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    dev = torch.device("cuda:0")
    print(f"V = {V}, d = {D_MODEL}, 3 H Dh = {N3}, S = {S}, {args.pad:.0%} of every sequence padded, {args.reps} interleaved repetitions; ms")
    print(f"{'T/V':>5} {'T':>8} {'per token: median (min .. max)':>34} {'by id: median (min .. max)':>32} {'saved':>7}")
    for r in (float(v) for v in args.ratios.split(",")):
        T = max(S, int(round(r * V / S)) * S)
        c = operands(T, args.pad, dev)
        ws = torch.empty(lib.meant_qkv_embed_bwd_by_id_ws(T, D_MODEL, N3, V), device=dev, dtype=torch.uint8)
        tok, bid = [], []
        for i in range(args.reps + 2):
            a, b = timed(lambda: per_token(c, dev)), timed(lambda: by_id(c, dev, ws))
            if i >= 2:                                       # two warm-up rounds
                tok.append(a)
                bid.append(b)
        mt, mb = statistics.median(tok), statistics.median(bid)
        print(f"{r:5.1f} {T:8d} {mt:12.3f} ({min(tok):.3f} .. {max(tok):.3f}) {mb:12.3f} ({min(bid):.3f} .. {max(bid):.3f}) {mt - mb:7.3f}")
        del c, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
