#!/usr/bin/env python3
"""dev probe: ops.qkv_attention in the bf16 tier at head dims off the 8-grid (Dh = 76 and 100, H = 2, no rotary tables), forward and
forward + backward, projection GEMM, padding and slicing included.  A build that pads such heads to a native dim of the MFMA
attention kernels (76 -> 96, 100 -> 128) is compared with one that runs them on the fp32 detour.

    python tools/probe_attn_any_heads.py [G, default 384]                 one run of the tree this file is in: one JSON line
    python tools/probe_attn_any_heads.py [G] --against OTHER_TREE         ROUNDS runs of this tree and of OTHER_TREE (a built
                                                                          checkout of another commit), alternating, each in a
                                                                          fresh process; medians, spreads and the verdict per shape

A shape's padded route counts as faster only if the other tree's median exceeds this tree's by more than the larger of the two
run-to-run spreads (max - min over the rounds)."""
import json, math, os, statistics, subprocess, sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROUNDS = 5
SHAPES = [(Dh, S, causal) for Dh in (76, 100) for S, causal in ((196, 0), (512, 1))]
H = 2


def one_run(G):
    sys.path.insert(0, os.path.join(HERE, ".."))
    import torch
    from meant_amd import _lib, ops
    dev = torch.device("cuda")

    def timeit(f, n=5):
        f()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n): f()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    out = {}
    for Dh, S, causal in SHAPES:
        D = H * Dh
        gen = torch.Generator().manual_seed(Dh + S)
        x = torch.randn(G, S, D, generator=gen).to(dev).bfloat16().requires_grad_()
        do = torch.randn(G, S, D, generator=gen).to(dev).bfloat16()
        w = [(torch.randn(D, D, generator=gen) / math.sqrt(D)).to(dev).requires_grad_() for _ in range(3)]
        b = [torch.zeros(D, device=dev, requires_grad=True) for _ in range(3)]
        mask = None
        if causal:                                                           # suffix padding of up to half the sequence
            keep = S - torch.randint(0, S // 2, (G,), generator=gen)
            mask = (torch.arange(S)[None, :] < keep[:, None]).float().to(dev)
        fwd = lambda: ops.qkv_attention(x, w[0], b[0], w[1], b[1], w[2], b[2], None, mask, bool(causal), H)

        def both():
            for p in [x] + w + b:
                p.grad = None
            fwd().backward(do)

        _lib.route_reset()
        with torch.no_grad():
            fwd()
        torch.cuda.synchronize()
        route = "detour" if _lib.route_count("attn_generic") else "native"
        with torch.no_grad():
            tf = timeit(fwd)
        tb = timeit(both)
        out[f"Dh{Dh}_S{S}{'c' if causal else ''}"] = dict(route=route, fwd_ms=tf, fwd_bwd_ms=tb)
        del x, do, w, b
        torch.cuda.empty_cache()
    print("PROBE " + json.dumps(out), flush=True)


def child(tree, G):
    r = subprocess.run([sys.executable, os.path.join(tree, "tools", "probe_attn_any_heads.py"), str(G)], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.exit(f"{tree}: probe run failed ({r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    line = [l for l in r.stdout.splitlines() if l.startswith("PROBE ")][-1]
    return json.loads(line[6:])


def compare(other, G):
    this = os.path.abspath(os.path.join(HERE, ".."))
    runs = {"this": [], "other": []}
    for _ in range(ROUNDS):                                                  # interleaved: this, other, this, ...
        runs["this"].append(child(this, G))
        runs["other"].append(child(os.path.abspath(other), G))
    print(f"G {G} H {H} bf16, no tables; {ROUNDS} alternating runs per tree, each a fresh process; median [min .. max] ms")
    for Dh, S, causal in SHAPES:
        key = f"Dh{Dh}_S{S}{'c' if causal else ''}"
        for what in ("fwd_ms", "fwd_bwd_ms"):
            col = {side: [r[key][what] for r in runs[side]] for side in runs}
            med = {s: statistics.median(v) for s, v in col.items()}
            spread = max(max(v) - min(v) for v in col.values())
            gain = med["other"] - med["this"]
            verdict = "faster" if gain > spread else "slower" if -gain > spread else "within the spread"
            print(f"Dh {Dh:3d} S {S:3d} {'causal+pad' if causal else 'full      '} {what[:-3]:8s}"
                  f" | this ({runs['this'][0][key]['route']}) {med['this']:8.3f} [{min(col['this']):8.3f} .. {max(col['this']):8.3f}]"
                  f" | other ({runs['other'][0][key]['route']}) {med['other']:8.3f} [{min(col['other']):8.3f} .. {max(col['other']):8.3f}]"
                  f" | {med['other'] / med['this']:5.2f}x, this tree is {verdict}", flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    other = None
    if "--against" in args:
        i = args.index("--against")
        other = args[i + 1]
        del args[i:i + 2]
    G = int(args[0]) if args else 384
    compare(other, G) if other else one_run(G)
