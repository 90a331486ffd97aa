#!/usr/bin/env python3
"""dev probe: the one-row-per-workgroup RMSNorm forward / backward (d > 2048, or d % 8 != 0) in bf16, one line per shape: time and
the bytes the shape must move (from the shapes alone) per second, as a fraction of the HBM peak.  (65536, 1000) is a multiple of 8
and runs the one-row-per-wave kernel; it is printed beside the odd width next to it for comparison.
usage: python tools/probe_norm_wide.py [peak TB/s, default 8.0]"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from meant_amd._lib import lib, check
dev = torch.device("cuda")
st = torch.cuda.current_stream().cuda_stream
PEAK = float(sys.argv[1]) * 1e12 if len(sys.argv) > 1 else 8.0e12


def timeit(f, n=20):
    for _ in range(3): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


SHAPES = [(16384, 2304), (8192, 4096), (4096, 12288), (65536, 1000), (65536, 1001)]
for rows, d in SHAPES:
    x = torch.randn(rows, d, device=dev).bfloat16(); g = torch.ones(d, device=dev); r = torch.empty(rows, device=dev)
    y = torch.empty_like(x); dy = torch.randn(rows, d, device=dev).bfloat16(); dx = torch.empty_like(x); ds = torch.empty(d, device=dev)
    wsb = lib.meant_rmsnorm_bwd_ws(rows, d); ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
    route = "wide" if (d > 2048 or d % 8) else "per-wave"
    fwd_bytes = rows * d * 2 * 2 + rows * 4 + d * 4                   # x read, y written, rinv, gain
    bwd_bytes = rows * d * 2 * 3 + rows * 4 + d * 4                   # x, dy read, dx written, rinv, gain (partials not counted)
    tf = timeit(lambda: check(lib.meant_rmsnorm_fwd(x.data_ptr(), g.data_ptr(), y.data_ptr(), r.data_ptr(), rows, d, 1e-8, 0.0, 77, 1, st)))
    tb = timeit(lambda: check(lib.meant_rmsnorm_bwd(dy.data_ptr(), x.data_ptr(), g.data_ptr(), r.data_ptr(), dx.data_ptr(), ds.data_ptr(), rows, d,
                                                    1e-8, 0.0, 77, None, None, 1, ws.data_ptr(), wsb, st)))
    print(f"({rows:6d}, {d:5d}) {route:8s}  fwd {tf:.3f} ms {fwd_bytes / tf / 1e9:5.2f} TB/s {fwd_bytes / tf * 1e3 / PEAK:5.1%}   "
          f"bwd {tb:.3f} ms {bwd_bytes / tb / 1e9:5.2f} TB/s {bwd_bytes / tb * 1e3 / PEAK:5.1%}", flush=True)
    del x, y, dy, dx, ws
