#!/usr/bin/env python3
"""dev probe: the row-wise entries at shapes that take their element forms (profiles/rows_forms_refactor.txt), at the C ABI: a
TimeSformer at dim 99 (128 videos of 12 frames of 196 patches: 301 184 rows of 99, GEGLU of 4 x 99), a MEANT model at text_dim 100 /
image_dim 50 (pools into rows of 150, the embedding lookup at 100).  One line per (entry, tier): ms per call over a window of about
250 ms after a warm-up; the shapes are large enough that the shortest call is tens of microseconds, well above what a launch from
Python costs.  Takes no part in any test.  To compare two builds, run it in alternating processes with MEANT_LIB_PATH naming each
build's library, the reference build first in every round.

usage: python tools/probe_rows_forms.py [label]"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from meant_amd import _lib
from meant_amd._lib import lib, check

label = sys.argv[1] if len(sys.argv) > 1 else "build"
dev = torch.device("cuda")
st = torch.cuda.current_stream().cuda_stream
VID, F, N, DIM = 128, 12, 196, 99
ROWS = VID * (1 + F * N)


def timeit(f):
    f(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); f(); e1.record(); torch.cuda.synchronize()
    n = max(3, min(20000, int(250.0 / max(e0.elapsed_time(e1), 1e-3))))
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def entries(dtype, code):
    g = torch.Generator(device=dev).manual_seed(7)
    rnd = lambda *shape, dt=dtype: torch.randn(*shape, device=dev, generator=g).to(dt)
    p = lambda t: t.data_ptr()
    x, y = rnd(ROWS, DIM), torch.empty(ROWS, DIM, device=dev, dtype=dtype)
    idx = torch.randperm(ROWS, device=dev, generator=g).to(torch.int32)
    yield "gather_rows", lambda: check(lib.meant_gather_rows(p(x), p(idx), None, p(y), ROWS, DIM, code, st))
    yield "token_shift", lambda: check(lib.meant_token_shift(p(x), p(y), VID, F, N, DIM, 0, code, st))
    h, dh = rnd(ROWS, 8 * DIM), torch.empty(ROWS, 8 * DIM, device=dev, dtype=dtype)
    dy, gy = rnd(ROWS, 4 * DIM), torch.empty(ROWS, 4 * DIM, device=dev, dtype=dtype)
    yield "geglu_fwd", lambda: check(lib.meant_geglu_fwd(p(h), p(gy), ROWS, 4 * DIM, code, st))
    yield "geglu_bwd", lambda: check(lib.meant_geglu_bwd(p(h), p(dy), p(dh), ROWS, 4 * DIM, code, st))
    n = (ROWS - 1) * DIM                                  # odd: 16-byte groups and an element tail from aligned bases
    xo, yo = torch.empty(n + 1, device=dev, dtype=dtype), torch.empty(n + 1, device=dev, dtype=dtype)
    xo[1:] = x.view(-1)[:n]
    yield "dropout", lambda: check(lib.meant_dropout(p(x), p(y), n, 0.1, 1234, code, st))
    yield "dropout base+1", lambda: check(lib.meant_dropout(p(xo[1:]), p(yo[1:]), n, 0.1, 1234, code, st))
    xa, ya, v = rnd(262144, 150), torch.empty(262144, 150, device=dev, dtype=dtype), rnd(12, 150, dt=torch.float32)
    yield "add_rowvec", lambda: check(lib.meant_add_rowvec(p(xa), p(v), p(ya), 262144, 150, 12, code, st))
    G = 1536                                              # 128 samples x 12 days
    xt, xi, cat = rnd(G, 512, 100), rnd(G, 196, 50), torch.empty(G, 150, device=dev, dtype=torch.float32)
    dxt, dxi = torch.empty_like(xt), torch.empty_like(xi)
    yield "meanpool_fwd text", lambda: check(lib.meant_meanpool_fwd(p(xt), p(cat), 150, 0, G, 512, 100, code, _lib.F32, st))
    yield "meanpool_fwd image", lambda: check(lib.meant_meanpool_fwd(p(xi), p(cat), 150, 100, G, 196, 50, code, _lib.F32, st))
    yield "meanpool_bwd text", lambda: check(lib.meant_meanpool_bwd(p(cat), 150, 0, p(dxt), G, 512, 100, code, _lib.F32, st))
    yield "meanpool_bwd image", lambda: check(lib.meant_meanpool_bwd(p(cat), 150, 100, p(dxi), G, 196, 50, code, _lib.F32, st))
    T = 786432
    table, ids, out = rnd(2000, 100, dt=torch.float32), torch.randint(0, 2000, (T,), device=dev, generator=g), torch.empty(T, 100, device=dev, dtype=dtype)
    yield "embedding_fwd", lambda: check(lib.meant_embedding_fwd(p(table), p(ids), p(out), T, 100, 2000, code, st))


for dtype, tier, code in ((torch.float32, "f32", _lib.F32), (torch.bfloat16, "bf16", _lib.BF16)):
    for name, call in entries(dtype, code):
        print(f"{label} {name:18s} {tier:4s} {timeit(call):9.4f} ms", flush=True)
    torch.cuda.empty_cache()
