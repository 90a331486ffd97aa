#!/usr/bin/env python3
"""dev probe: bf16 attention at head dims 160 / 192 / 256 on the native MFMA kernels against the fp32 detour the same shapes took
before (reached here through meant_attn_drop_* at drop_p = 0, which runs the same widening detour).  Per shape: forward and
backward time, useful TFLOP/s (4 G H S'^2 Dh forward, 2.5x that backward; S'^2 halved under the causal mask) and the fraction
of the bf16 dense peak.  The two routes run interleaved, ROUNDS times each; the median is printed.
usage: python tools/probe_attn_wide.py [G, default 384] [peak TFLOP/s, default 2500]"""
import math, os, statistics, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from meant_amd import _lib
from meant_amd._lib import lib, check
dev = torch.device("cuda")
st = torch.cuda.current_stream().cuda_stream
G = int(sys.argv[1]) if len(sys.argv) > 1 else 384
PEAK = float(sys.argv[2]) * 1e12 if len(sys.argv) > 2 else 2.5e15
H, ROUNDS, BF16 = 2, 5, 1


def timeit(f, n=5):
    f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


for Dh in (160, 192, 256):
    for S, causal in ((196, 0), (512, 1)):
        D, T = H * Dh, G * S
        qkv = torch.randn(T, 3 * D, device=dev).bfloat16(); do = torch.randn(T, D, device=dev).bfloat16()
        o = torch.empty(T, D, device=dev, dtype=torch.bfloat16); dqkv = torch.empty_like(qkv)
        o2 = torch.empty_like(o); dqkv2 = torch.empty_like(qkv)
        lse = torch.empty(G, H, S, 2, device=dev); lse2 = torch.empty_like(lse)
        mask = None
        if causal:                                                           # suffix padding of up to half the sequence
            g = torch.Generator().manual_seed(S)
            keep = S - torch.randint(0, S // 2, (G,), generator=g)
            mask = (torch.arange(S)[None, :] < keep[:, None]).float().to(dev)
        mp = mask.data_ptr() if mask is not None else None
        scale = 1.0 / math.sqrt(D)
        wsb = lib.meant_attn_ws(G, S, H, Dh, BF16); ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
        wsd = lib.meant_attn_drop_ws(G, S, H, Dh, BF16); wsdt = torch.empty(wsd, device=dev, dtype=torch.uint8)
        nf = lambda: check(lib.meant_attn_fwd(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), mp, G, S, H, Dh, scale, causal, BF16, ws.data_ptr(), wsb, st))
        nb = lambda: check(lib.meant_attn_bwd(qkv.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), mp, dqkv.data_ptr(), G, S, H, Dh, scale,
                                              causal, None, None, None, None, 0, BF16, ws.data_ptr(), wsb, st))
        df = lambda: check(lib.meant_attn_drop_fwd(qkv.data_ptr(), o2.data_ptr(), lse2.data_ptr(), mp, G, S, H, Dh, scale, causal, 0.0, 1, BF16,
                                                   wsdt.data_ptr(), wsd, st))
        db = lambda: check(lib.meant_attn_drop_bwd(qkv.data_ptr(), o2.data_ptr(), do.data_ptr(), lse2.data_ptr(), mp, dqkv2.data_ptr(), G, S, H, Dh,
                                                   scale, causal, 0.0, 1, BF16, wsdt.data_ptr(), wsd, st))
        _lib.route_reset()
        nf(); nb(); df(); db(); torch.cuda.synchronize()
        assert _lib.route_count(f"attn_fwd_d{Dh}") == 1 and _lib.route_count(f"attn_bwd_d{Dh}") == 1 and _lib.route_count("attn_generic") == 2
        diff = ((o.float() - o2.float()).abs().max().item(), (dqkv.float() - dqkv2.float()).abs().max().item())
        t = {k: [] for k in ("nf", "nb", "df", "db")}
        for _ in range(ROUNDS):                                              # interleaved: native, detour, native, ...
            t["nf"].append(timeit(nf)); t["nb"].append(timeit(lambda: (nf(), nb())) - t["nf"][-1])
            t["df"].append(timeit(df)); t["db"].append(timeit(lambda: (df(), db())) - t["df"][-1])
        m = {k: statistics.median(v) for k, v in t.items()}
        pairs = S * S / 2 if causal else S * S
        ff = 4.0 * G * H * pairs * Dh
        fb = 2.5 * ff
        line = f"Dh {Dh} S {S:3d} {'causal+pad' if causal else 'full      '} G {G}"
        for name, kf, kb in (("native", "nf", "nb"), ("detour", "df", "db")):
            line += (f" | {name} fwd {m[kf]:7.3f} ms {ff / m[kf] / 1e9:6.1f} TF {ff / m[kf] * 1e3 / PEAK:5.1%}"
                     f" bwd {m[kb]:7.3f} ms {fb / m[kb] / 1e9:6.1f} TF {fb / m[kb] * 1e3 / PEAK:5.1%}")
        line += f" | speed-up fwd {m['df'] / m['nf']:.1f}x bwd {m['db'] / m['nb']:.1f}x | max |diff| o {diff[0]:.2e} dqkv {diff[1]:.2e}"
        print(line, flush=True)
        del qkv, do, o, o2, dqkv, dqkv2, ws, wsdt
        torch.cuda.empty_cache()
