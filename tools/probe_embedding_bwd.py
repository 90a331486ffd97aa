#!/usr/bin/env python3
"""dev probe: the embedding gradient at n = 786 432 tokens, V = 64 001, d in {768, 1280, 2048}, both tiers, two id distributions
(uniform; half of all tokens on one id, as padding is), through the raw C entry points.

  sort     meant_sort_ids against torch.sort, with the kernel launches of each (counted by torch.profiler)
  reduce   meant_embedding_bwd_seg against the route the same input took before it existed:
             default        d <= 1024: meant_embedding_bwd_sorted (run atomics at the stretch ends);  d > 1024: meant_embedding_bwd (atomics)
             deterministic  d <= 1024: meant_embedding_bwd_sorted under option "deterministic" (one wave follows a run to its end);
                            d > 1024: meant_embedding_bwd again (the option did not reach that width)
           Both read the same (sorted ids, order) where they read one.

Times are HIP events around ~30 ms of back-to-back calls after a warm-up call, median of ROUNDS rounds that alternate the variants;
launches are counted by torch.profiler.  The old deterministic kernel on the hot-id input (a single wave's walk over 393 216 rows) is
left out of the plain run: `--slow-only` runs that case alone, one timed call per tier after a warm-up of the same kernel on uniform
ids, so that it can be given a time limit of its own.
usage: python tools/probe_embedding_bwd.py [--slow-only] [n, default 786432]"""
import os, statistics, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from meant_amd import _lib
from meant_amd._lib import lib, check
dev = torch.device("cuda")
st = torch.cuda.current_stream().cuda_stream
SLOW_ONLY = "--slow-only" in sys.argv
_args = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(_args[0]) if _args else 786432
V, ROUNDS = 64001, 3


def timeit(f, once=False):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if not once:
        f(); torch.cuda.synchronize()
    e0.record(); f(); e1.record(); torch.cuda.synchronize()
    if once:
        return e0.elapsed_time(e1)
    n = max(3, min(200, int(30.0 / max(e0.elapsed_time(e1), 1e-3))))      # ~30 ms of work per timed window
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def launches(f):
    from torch.profiler import profile, ProfilerActivity
    f(); torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        f(); torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def make_ids(kind):
    g = torch.Generator().manual_seed(17)
    ids = torch.randint(0, V, (N,), generator=g)
    if kind == "hot":
        ids[torch.randperm(N, generator=g)[: N // 2]] = 1
    return ids.to(dev)


def hip_sort(ids):
    sorted_ids, order = torch.empty_like(ids), torch.empty_like(ids)
    wsb = lib.meant_sort_ids_ws(N, V)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    f = lambda: check(lib.meant_sort_ids(ids.data_ptr(), N, V, sorted_ids.data_ptr(), order.data_ptr(), ws.data_ptr(), wsb, st))
    return f, sorted_ids, order


print(f"embedding gradient, n {N}, V {V}; median of {ROUNDS} alternating rounds, ms")
ids_of = {k: make_ids(k) for k in ("uniform", "hot")}
if SLOW_ONLY:
    d = 768
    srt = {k: torch.sort(v, stable=True) for k, v in ids_of.items()}
    for dtype, name, code in ((torch.float32, "f32 ", 0), (torch.bfloat16, "bf16", 1)):
        dout = torch.randn(N, d, device=dev).to(dtype)
        tab = torch.zeros(V, d, device=dev)
        _lib.set_option("deterministic", 1)
        try:
            run = lambda k: check(lib.meant_embedding_bwd_sorted(dout.data_ptr(), srt[k].values.data_ptr(), srt[k].indices.data_ptr(),
                                                                 tab.data_ptr(), N, d, V, code, st))
            run("uniform"); torch.cuda.synchronize()                        # the code object is loaded
            ms = timeit(lambda: run("hot"), once=True)
        finally:
            _lib.set_option("deterministic", 0)
        print(f"reduce {d:5d} {name} hot     | parent deterministic (sorted, follow-the-run), 1 call: {ms:10.3f} ms", flush=True)
    sys.exit(0)
sorted_of = {}
print("sort      ids     |  torch.sort  launches |  meant_sort_ids  launches | equal to torch.sort(stable)")
for kind, ids in ids_of.items():
    f_hip, s_ids, s_ord = hip_sort(ids)
    f_torch = lambda: torch.sort(ids)
    tt, th = [], []
    for _ in range(ROUNDS):
        tt.append(timeit(f_torch)); th.append(timeit(f_hip))
    want = torch.sort(ids, stable=True)
    same = torch.equal(want.values, s_ids) and torch.equal(want.indices, s_ord)
    try:
        lt, lh = launches(f_torch), launches(f_hip)
    except Exception as e:                                                  # the counts are a convenience; the times are the probe
        lt = lh = f"n/a ({type(e).__name__})"
    print(f"sort      {kind:7s} | {statistics.median(tt):11.4f} {lt!s:>9s} | {statistics.median(th):15.4f} {lh!s:>9s} | {same}", flush=True)
    sorted_of[kind] = (s_ids, s_ord)

print("reduce    d    tier ids     | new seg  launches | parent default (kernel)        | parent deterministic (kernel)   | max |new - parent default| / max")
for d in (768, 1280, 2048):
    for dtype, name, code in ((torch.float32, "f32 ", 0), (torch.bfloat16, "bf16", 1)):
        dout = torch.randn(N, d, device=dev).to(dtype)
        wsb = lib.meant_embedding_bwd_seg_ws(N, d)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        tab = {k: torch.zeros(V, d, device=dev) for k in ("new", "default", "det")}
        for kind, ids in ids_of.items():
            s_ids, s_ord = sorted_of[kind]

            def new():
                check(lib.meant_embedding_bwd_seg(dout.data_ptr(), s_ids.data_ptr(), s_ord.data_ptr(), tab["new"].data_ptr(), N, d, V, 0, V, code,
                                                  ws.data_ptr(), wsb, st))

            def old(det, key):
                _lib.set_option("deterministic", det)
                try:
                    if d <= 1024:
                        check(lib.meant_embedding_bwd_sorted(dout.data_ptr(), s_ids.data_ptr(), s_ord.data_ptr(), tab[key].data_ptr(), N, d, V, code, st))
                    else:
                        check(lib.meant_embedding_bwd(dout.data_ptr(), ids.data_ptr(), tab[key].data_ptr(), N, d, V, code, st))
                finally:
                    _lib.set_option("deterministic", 0)

            slow_det = d <= 1024 and kind == "hot"                          # the single wave's walk: --slow-only
            tn, td, tdet = [], [], []
            for r in range(ROUNDS):
                tn.append(timeit(new)); td.append(timeit(lambda: old(0, "default")))
                if not slow_det:
                    tdet.append(timeit(lambda: old(1, "det")))
            for k in tab: tab[k].zero_()
            new(); old(0, "default"); torch.cuda.synchronize()
            diff = (tab["new"] - tab["default"]).abs().max().item() / tab["default"].abs().max().item()
            for k in tab: tab[k].zero_()
            try:
                ln, lo = launches(new), launches(lambda: old(0, "default"))
            except Exception as e:
                ln = lo = f"n/a ({type(e).__name__})"
            for k in tab: tab[k].zero_()
            kd = "sorted" if d <= 1024 else "atomics"
            kdet = "sorted, follow-the-run" if d <= 1024 else "atomics"
            det_ms = "see --slow-only" if slow_det else f"{statistics.median(tdet):9.4f}"
            print(f"reduce {d:5d} {name} {kind:7s} | {statistics.median(tn):7.4f} {ln!s:>9s} | {statistics.median(td):9.4f} ({kd:8s}) {lo!s:>3s} launches | "
                  f"{det_ms} ({kdet}) | {diff:.1e}", flush=True)
        del dout, ws, tab
        torch.cuda.empty_cache()
