"""Same calls, same bits: one forward + backward of every wrapper route in meant_amd/ops.py and meant_amd/modules.py, with a trace of
every C ABI call and a sha256 of every result.  Run it on two checkouts that share ONE built library and compare the files:

    git worktree add ../parent HEAD~1
    export MEANT_LIB_PATH=$PWD/meant_amd/libmeant_hip.so
    python tools/step_digest.py --pkg-root ../parent --out parent_a      # twice: what differs between these two runs is not
    python tools/step_digest.py --pkg-root ../parent --out parent_b      # reproducible on the parent and is exempt
    python tools/step_digest.py --out this
    python tools/step_digest.py --compare parent_a parent_b this

(A change to the kernels alone is the other way round: one checkout, MEANT_LIB_PATH set to the parent's library for parent_a and parent_b
and to this tree's for the third run.)

Writes OUT.trace (one line per library call: name, every non-pointer argument, null / ptr for the pointers) and OUT.digests (per case:
sha256 of the output, of the input gradient, of every parameter gradient in named_parameters() order, and the peak of allocated bytes).
Library option `deterministic` is on and every case starts from the same torch.manual_seed."""
import argparse
import ctypes
import gc
import hashlib
import os
import sys

import numpy as np
import torch


def trace_calls(lib, signatures, log):
    """wrap every entry of `signatures` on the CDLL instance `lib`; pointers are recorded only as null / ptr"""
    def word(a, t):
        if t is ctypes.c_void_p:
            return "null" if a is None or (isinstance(a, int) and a == 0) else "ptr"
        return repr(a) if isinstance(a, (int, float, bytes)) else "ref"
    for name, (_, argtypes) in signatures.items():
        def call(*args, _fn=getattr(lib, name), _name=name, _types=argtypes):
            log.append(" ".join([_name] + [word(a, t) for a, t in zip(args, _types)]))
            return _fn(*args)
        setattr(lib, name, call)


def sha(t):
    return "none" if t is None else hashlib.sha256(t.detach().contiguous().view(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16]


def cases(M, ops, _lib, dev):
    """yields (name, thunk); a thunk returns (output, {name: gradient})"""
    F32, BF = torch.float32, torch.bfloat16
    tier = {F32: "f32", BF: "bf16"}

    def model(cls, td, idim, heads, dtype, ckpt=False, encoders=None):
        def run():
            emb = torch.nn.Embedding(50, td)
            if cls == "meant":
                m = M.meant(td, idim, 4, 32, 64, 16, 2, 3, emb, num_heads=heads, num_encoders=encoders or 2, channels=4)
            elif cls == "meant_vqa":
                m = M.meant_vqa(td, idim, 4, 32, 64, 16, 1, 5, emb, num_heads=heads, num_encoders=1, channels=4)
            else:
                m = M.meant_tweet(td, 4, 2, 3, emb, num_heads=heads, num_encoders=1)
            m = m.to(dev).train()
            m.compute_dtype = dtype
            m.activation_checkpointing = ckpt
            rs = np.random.RandomState(8)
            lag = 1 if cls == "meant_vqa" else 2
            ids = torch.from_numpy(rs.randint(0, 50, (3, lag, 24))).to(dev)
            img = torch.from_numpy(rs.standard_normal((3, lag, 4, 32, 64)).astype("float32")).to(dev)
            mask = torch.ones(3, lag, 24, device=dev)
            mask[1, :, 17:] = 0
            if cls == "meant_vqa":
                ids, img, mask = ids[:, 0], img[:, 0], mask[:, 0]
            out = m(*{"meant": (ids, img, mask), "meant_vqa": (ids, img, mask), "meant_tweet": (ids, mask)}[cls])
            (out * torch.arange(1, out.numel() + 1, device=dev).view_as(out)).sum().backward()
            return out, {k: p.grad for k, p in m.named_parameters()}
        return run

    for cls, dim in (("meant", 128), ("meant_tweet", 768), ("meant_vqa", 256)):
        for dtype in (F32, BF):
            for fold in (False, True):
                def run(f=model(cls, dim, dim, dim // 64, dtype), fold=fold):
                    ops.FUSE_NORM_LINEAR = fold
                    return f()
                yield f"{cls}-{dim}-{tier[dtype]}-fold{int(fold)}", run
    ops.FUSE_NORM_LINEAR = None
    yield "meant-100x50-bf16", model("meant", 100, 50, 2, BF)
    yield "meant-128-bf16-checkpointed", model("meant", 128, 128, 2, BF, ckpt=True)

    def fused(mask_name, kv_skip):                        # tests/test_gpu_kv_skip.py: G = 24, S = 512, d = 768, 12 heads, bf16, causal
        def run():
            G, S, D, H = 24, 512, 768, 12
            mk = np.ones((G, S), dtype=np.float32)
            for g in range(G):
                if mask_name == "trailing":
                    p = (0, 1, 63, 64, 65, 255, 256, 257, 383, 448)[g % 10]
                    if p:
                        mk[g, S - p:] = 0
                else:
                    lo = 192 if g % 2 == 0 else 200
                    mk[g, lo:lo + 128] = 0
            gen = torch.Generator().manual_seed(2024)
            x = torch.randn(G, S, D, generator=gen).to(dev).to(BF).requires_grad_()
            w = (torch.randn(3 * D, D, generator=gen) / D ** 0.5).to(dev).requires_grad_()
            b = (torch.randn(3 * D, generator=gen) * 0.1).to(dev).requires_grad_()
            do = torch.randn(G, S, D, generator=gen).to(dev).to(BF)
            tables = M.RotaryEmbedding(dim=48, use_xpos=True).tables(S, dev)
            old = _lib.get_option("kv_skip")
            _lib.set_option("kv_skip", kv_skip)
            try:
                o = ops._QKVAttention.apply(x, w, b, tables, torch.from_numpy(mk).to(dev), True, H)
                o.backward(do)
            finally:
                _lib.set_option("kv_skip", old)
            return o, {"x": x.grad, "w": w.grad, "b": b.grad}
        return run

    for mask_name in ("trailing", "hole"):
        for kv in (0, 3):
            yield f"qkv_attention-{mask_name}-kv_skip{kv}", fused(mask_name, kv)

    def core(dtype, drop_p, masked):
        def run():
            G, S, H, Dh = 2, 24, 2, 64
            gen = torch.Generator().manual_seed(31)
            qkv = torch.randn(G * S, 3 * H * Dh, generator=gen).to(dev).to(dtype).requires_grad_()
            do = torch.randn(G * S, H * Dh, generator=gen).to(dev).to(dtype)
            tables = M.RotaryEmbedding(dim=48, use_xpos=True).tables(S, dev)
            km = None
            if masked:
                km = torch.ones(G, S, device=dev)
                km[1, 17:] = 0
            if drop_p is None:
                o = ops.attention_core(qkv, G, S, H, Dh ** -0.5, tables, masked, km)
            else:
                o = ops.attention_core_score_dropout(qkv, G, S, H, Dh ** -0.5, drop_p, 1234567, tables, masked, km)
            o.backward(do)
            return o, {"qkv": qkv.grad}
        return run

    for dtype in (F32, BF):
        yield f"attention_core-tables-{tier[dtype]}", core(dtype, None, False)
        yield f"attention_core_score_dropout-p0.5-causal-masked-{tier[dtype]}", core(dtype, 0.5, True)
        yield f"attention_core_score_dropout-p0-{tier[dtype]}", core(dtype, 0.0, False)

    def divided(dtype):                                   # tests/test_gpu_divided.py, the "d32" shape, time half
        def run():
            b, f, hp, wp, H, Dh = 2, 4, 6, 6, 4, 32
            L, D = 1 + f * hp * wp, H * Dh
            ts = M.TimeSformer(dim=8, num_frames=f, num_classes=2, image_size=16, patch_size=16, depth=0, heads=H, dim_head=Dh)
            t_time, _, p_time, _, _, _ = ts._plan(b, f, hp, wp, dev)
            rs = np.random.RandomState(17)
            qkv = torch.from_numpy(rs.standard_normal((b, L, 3 * D)).astype("float32")).to(dev).to(dtype).requires_grad_()
            dout = torch.from_numpy(rs.standard_normal((b, L, D)).astype("float32")).to(dev).to(dtype)
            out = ops.divided_attention(qkv, p_time, t_time, H, Dh ** -0.5)
            out.backward(dout)
            return out, {"qkv": qkv.grad}
        return run

    for dtype in (F32, BF):
        yield f"divided_attention-{tier[dtype]}", divided(dtype)

    def timesformer_odd(dim, heads, dim_head, dtype):     # layers at a width off the 8-grid: gather_rows, token_shift, geglu and dropout
        def run():                                        # by element access (tests/test_gpu_timesformer_any.py, the "dim99" / "dim100" shapes)
            m = M.TimeSformer(dim=dim, heads=heads, dim_head=dim_head, num_frames=3, image_size=32, patch_size=16, depth=1, num_classes=3,
                              channels=3, shift_tokens=True, attn_dropout=0.1, ff_dropout=0.1).to(dev).train()
            m.compute_dtype = dtype
            video = torch.from_numpy(np.random.RandomState(dim).standard_normal((2, 3, 3, 32, 32)).astype("float32")).to(dev)
            out = m(video)
            (out.float() * torch.arange(1, out.numel() + 1, device=dev).view_as(out)).sum().backward()
            return out, {k: p.grad for k, p in m.named_parameters()}
        return run

    for dim, heads, dim_head in ((99, 3, 20), (100, 2, 16)):
        for dtype in (F32, BF):
            yield f"timesformer-{dim}-depth1-{tier[dtype]}", timesformer_odd(dim, heads, dim_head, dtype)

    def rows_elem(entry, dtype):                          # one call per row-wise entry at a shape of its element form
        def run():
            lib, check, code, st = _lib.lib, _lib.check, (_lib.BF16 if dtype == BF else _lib.F32), torch.cuda.current_stream().cuda_stream
            rs = np.random.RandomState(len(entry))

            def rnd(*shape, dt=dtype):
                return torch.from_numpy(rs.standard_normal(shape).astype("float32")).to(dev).to(dt)

            def full(*shape, dt=dtype):                   # outputs start from a fill, so an element that is not written shows in the digest
                return torch.full(shape, 7.0, device=dev, dtype=dt)
            p = lambda t: t.data_ptr()
            if entry == "add_rowvec":
                x, v, y = rnd(10, 150), rnd(5, 150, dt=F32), full(10, 150)
                check(lib.meant_add_rowvec(p(x), p(v), p(y), 10, 150, 5, code, st), entry)
                return y, {}
            if entry == "meanpool":                       # the image means of a model at text_dim = 100, image_dim = 50
                x, out, dx = rnd(3, 5, 50), full(3, 150, dt=F32), full(3, 5, 50)
                check(lib.meant_meanpool_fwd(p(x), p(out), 150, 100, 3, 5, 50, code, _lib.F32, st), entry)
                check(lib.meant_meanpool_bwd(p(out), 150, 100, p(dx), 3, 5, 50, code, _lib.F32, st), entry)
                return out, {"dx": dx}
            if entry == "gather_rows":
                src, fill, dst = rnd(41, 99), rnd(99), full(47, 99)
                idx = torch.from_numpy(np.concatenate((rs.permutation(41), [-1, -2, 0, -2, -1, 40])).astype("int32")).to(dev)
                check(lib.meant_gather_rows(p(src), p(idx), p(fill), p(dst), 47, 99, code, st), entry)
                return dst, {}
            if entry == "token_shift":
                x, y, yt = rnd(2, 13, 99), full(2, 13, 99), full(2, 13, 99)
                check(lib.meant_token_shift(p(x), p(y), 2, 3, 4, 99, 0, code, st), entry)
                check(lib.meant_token_shift(p(x), p(yt), 2, 3, 4, 99, 1, code, st), entry)
                return y, {"transpose": yt}
            if entry == "geglu":
                h, dy, y, dh = rnd(131, 396), rnd(131, 198), full(131, 198), full(131, 396)
                check(lib.meant_geglu_fwd(p(h), p(y), 131, 198, code, st), entry)
                check(lib.meant_geglu_bwd(p(h), p(dy), p(dh), 131, 198, code, st), entry)
                return y, {"dh": dh}
            if entry == "dropout":                        # aligned bases: 16-byte groups and an element tail; one element off: all by element
                x, y, yo = rnd(8005), full(8005), full(8006)
                xo = torch.cat((x[:1], x))[1:]
                check(lib.meant_dropout(p(x), p(y), 8005, 0.25, 1234, code, st), entry)
                check(lib.meant_dropout(p(xo), p(yo[1:]), 8005, 0.25, 1234, code, st), entry)
                return y, {"off_by_one": yo}
            table, out = rnd(50, 100, dt=F32), full(37, 100)
            ids = torch.from_numpy(rs.randint(-1, 52, 37).astype("int64")).to(dev)
            check(lib.meant_embedding_fwd(p(table), p(ids), p(out), 37, 100, 50, code, st), entry)
            return out, {}
        return run

    for entry in ("add_rowvec", "meanpool", "gather_rows", "token_shift", "geglu", "dropout", "embedding_fwd"):
        for dtype in (F32, BF):
            yield f"rows_elem-{entry}-{tier[dtype]}", rows_elem(entry, dtype)

    def folded(pooled):
        def run():
            d, G, S, p, seed = 128, 4, 24, 0.5, 1234567
            gen = torch.Generator().manual_seed(d + S)
            x = torch.randn(G, S, d, generator=gen).to(dev).to(BF).requires_grad_()
            W = (torch.randn(d, d, generator=gen) / d ** 0.5).to(dev).requires_grad_()
            bias = (torch.randn(d, generator=gen) * 0.1).to(dev).requires_grad_()
            g0 = (1 + 0.1 * torch.randn(d, generator=gen)).to(dev).requires_grad_()
            g3 = (1 + 0.1 * torch.randn(d, generator=gen)).to(dev).requires_grad_()
            fn = ops.norm_linear_gelu_norm_pooled if pooled else ops.norm_linear_gelu_norm
            y, res = fn(x, g0, 1e-8, W, bias, g3, 1e-8, p, seed)
            wy = torch.randn(y.shape, generator=gen).to(dev)
            wr = torch.randn(res.shape, generator=gen).to(dev)
            ((y.float() * wy).sum() + (res.float() * wr).sum()).backward()
            return torch.cat((y.float().reshape(-1), res.float().reshape(-1))), {"x": x.grad, "W": W.grad, "b": bias.grad, "g0": g0.grad, "g3": g3.grad}
        return run

    yield "norm_linear_gelu_norm", folded(False)
    yield "norm_linear_gelu_norm_pooled", folded(True)


def run(args):
    sys.path.insert(0, os.path.abspath(args.pkg_root))
    import meant_amd as M
    from meant_amd import _lib, ops
    assert os.path.abspath(M.__file__).startswith(os.path.abspath(args.pkg_root)), M.__file__
    log = []
    trace_calls(_lib.lib, _lib.SIGNATURES, log)
    _lib.set_option("deterministic", 1)
    dev = torch.device("cuda:0")
    lines = []
    for name, thunk in cases(M, ops, _lib, dev):
        log.append(f"# {name}")
        torch.manual_seed(5)
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        out, grads = thunk()
        torch.cuda.synchronize()
        lines.append(f"{name} peak_bytes {torch.cuda.max_memory_allocated()}")
        lines.append(f"{name} out {sha(out)}")
        lines += [f"{name} grad {k} {sha(g)}" for k, g in grads.items()]
        del out, grads
    with open(args.out + ".trace", "w") as f:
        f.write("\n".join(log) + "\n")
    with open(args.out + ".digests", "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{args.out}: {len(log)} trace lines, {len(lines)} digest lines")


def compare(a, b, c):
    """a, b: two runs of the parent; c: this tree.  Exit status 1 on a trace difference, a digest that the parent reproduces and
    this tree does not, or a larger peak"""
    def table(path):
        return {ln.rsplit(" ", 1)[0]: ln.rsplit(" ", 1)[1] for ln in open(path).read().splitlines()}
    ta, tc = (open(p + ".trace").read().splitlines() for p in (a, c))
    bad = ta != tc
    print(f"trace: parent {len(ta)} lines, this tree {len(tc)} lines, {'IDENTICAL' if not bad else 'DIFFERENT'}")
    if bad:
        i = next((i for i, (x, y) in enumerate(zip(ta, tc)) if x != y), min(len(ta), len(tc)))
        print(f"  first difference at line {i + 1}:\n  parent: {ta[i] if i < len(ta) else '-'}\n  this:   {tc[i] if i < len(tc) else '-'}")
    da, db, dc = table(a + ".digests"), table(b + ".digests"), table(c + ".digests")
    bad |= da.keys() != dc.keys()
    for key in da:
        if key.endswith("peak_bytes"):
            over = int(dc.get(key, 1 << 62)) > int(da[key])
            bad |= over
            print(f"{key}: parent {da[key]} this {dc.get(key)}{'  LARGER' if over else ''}")
        elif da[key] != db.get(key):
            print(f"{key}: EXEMPT (parent {da[key]} / {db.get(key)}, this {dc.get(key)})")
        else:
            same = da[key] == dc.get(key)
            bad |= not same
            print(f"{key}: parent {da[key]} this {dc.get(key)} {'same' if same else 'DIFFERENT'}")
    return int(bad)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pkg-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="tree to import meant_amd from")
    ap.add_argument("--out", default="step_digest", help="prefix of the .trace and .digests files")
    ap.add_argument("--compare", nargs=3, metavar=("PARENT_A", "PARENT_B", "THIS"), help="compare three --out prefixes instead of running")
    a = ap.parse_args()
    sys.exit(compare(*a.compare) if a.compare else run(a))
