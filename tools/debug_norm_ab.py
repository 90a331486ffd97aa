#!/usr/bin/env python3
"""dev probe: every norm entry point (RMSNorm full / partial / pooled / statistics / chained, LayerNorm) on fixed inputs, outputs
saved to argv[1] (run once per build with MEANT_LIB_PATH), or with two files: compare them.  The model shapes first, then the
smallest shape of every route of csrc/norm.hip's classifier, in both dtypes."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
if len(sys.argv) == 3:
    a, b = torch.load(sys.argv[1]), torch.load(sys.argv[2])
    for k in a:
        x, y = a[k].float(), b[k].float()
        print(f"{k:40s} max|a-b| {(x - y).abs().max().item():.3e}  rel norm {((x - y).norm() / max(y.norm().item(), 1e-30)).item():.3e}  |b| {y.norm().item():.3e}")
    sys.exit(0)
from meant_amd._lib import lib, check
dev = torch.device("cuda"); st = torch.cuda.current_stream().cuda_stream
out = {}
for rows, d, S, DT in ((12288, 768, 512, 1), (4704, 768, 196, 1), (12288, 768, 512, 0), (24, 768, 12, 1), (1024, 768, 512, 1), (24, 1536, 12, 1), (392, 768, 196, 1), (24, 768, 12, 0), (24, 1536, 12, 0), (1024, 768, 512, 0), (26, 1536, 13, 0), (26, 1536, 13, 1)):
    gen = torch.Generator().manual_seed(rows + d)
    cast = (lambda z: z.bfloat16()) if DT else (lambda z: z.float())
    x = cast(torch.randn(rows, d, generator=gen).to(dev)); dy = cast(torch.randn(rows, d, generator=gen).to(dev))
    g = (1 + 0.1 * torch.randn(d, generator=gen)).to(dev); r = torch.empty(rows, device=dev)
    y = torch.empty_like(x); dx = torch.empty_like(x); ds = torch.empty(d, device=dev)
    wsb = lib.meant_rmsnorm_bwd_ws(rows, d); ws = torch.empty(max(wsb, 16), device=dev, dtype=torch.uint8)
    tag = f"{rows}x{d}{'b' if DT else 'f'}"
    check(lib.meant_rmsnorm_fwd(x.data_ptr(), g.data_ptr(), y.data_ptr(), r.data_ptr(), rows, d, 1e-8, 0.0, 0, DT, st))
    out[tag + " fwd y"] = y.clone(); out[tag + " fwd rinv"] = r.clone()
    for nm, dres, gp in (("bwd", None, None), ("bwd+dres", dy, None), ("bwd+gelu", dy, x)):
        check(lib.meant_rmsnorm_bwd(dy.data_ptr(), x.data_ptr(), g.data_ptr(), r.data_ptr(), dx.data_ptr(), ds.data_ptr(), rows, d, 1e-8, 0.0, 0,
                                    dres.data_ptr() if dres is not None else None, gp.data_ptr() if gp is not None else None, DT, ws.data_ptr(), wsb, st))
        out[f"{tag} {nm} dx"] = dx.clone(); out[f"{tag} {nm} dscale"] = ds.clone()
    if lib.meant_rmsnorm_pooled_ok(rows, d, S):
        G = rows // S
        pooled = torch.empty(G, d, device=dev); dyp = torch.randn(G, d, generator=gen).to(dev)
        for gelu in (0, 1):
            check(lib.meant_rmsnorm_fwd_pooled(x.data_ptr(), g.data_ptr(), None, r.data_ptr(), pooled.data_ptr(), rows, d, S, 0, gelu, 1e-8, 0.0, 0, DT, st))
            out[f"{tag} fwd_pooled gelu={gelu} pooled"] = pooled.clone(); out[f"{tag} fwd_pooled gelu={gelu} rinv"] = r.clone()
            check(lib.meant_rmsnorm_bwd_pooled(dyp.data_ptr(), 1, None if gelu else x.data_ptr(), g.data_ptr(), r.data_ptr(), dx.data_ptr(), ds.data_ptr(), rows, d, S, 1e-8, 0.0, 0,
                                               None, 0, x.data_ptr() if gelu else None, DT, ws.data_ptr(), wsb, st))
            out[f"{tag} bwd_pooled gelu={gelu} dx"] = dx.clone(); out[f"{tag} bwd_pooled gelu={gelu} dscale"] = ds.clone()
        check(lib.meant_rmsnorm_fwd_pooled(x.data_ptr(), g.data_ptr(), y.data_ptr(), r.data_ptr(), pooled.data_ptr(), rows, d, S, 1, 0, 1e-8, 0.0, 0, DT, st))
        out[f"{tag} fwd pool_input y"] = y.clone(); out[f"{tag} fwd pool_input pooled"] = pooled.clone()
        check(lib.meant_rmsnorm_bwd_pooled(dy.data_ptr(), 0, x.data_ptr(), g.data_ptr(), r.data_ptr(), dx.data_ptr(), ds.data_ptr(), rows, d, S, 1e-8, 0.0, 0,
                                           dyp.data_ptr(), 1, None, DT, ws.data_ptr(), wsb, st))
        out[f"{tag} bwd dres_pooled dx"] = dx.clone()
        check(lib.meant_rmsnorm_bwd_pooled(dyp.data_ptr(), 1, x.data_ptr(), g.data_ptr(), r.data_ptr(), dx.data_ptr(), ds.data_ptr(), rows, d, S, 1e-8, 0.0, 0,
                                           dyp.data_ptr(), 1, None, DT, ws.data_ptr(), wsb, st))
        out[f"{tag} bwd both pooled dx"] = dx.clone(); out[f"{tag} bwd both pooled dscale"] = ds.clone()
        check(lib.meant_rmsnorm_fwd_pooled(x.data_ptr(), g.data_ptr(), None, r.data_ptr(), pooled.data_ptr(), rows, d, S, 1, 0, 1e-8, 0.0, 0, DT, st))
        out[f"{tag} fwd stats+means rinv"] = r.clone(); out[f"{tag} fwd stats+means pooled"] = pooled.clone()
    check(lib.meant_rmsnorm_stats(x.data_ptr(), r.data_ptr(), rows, d, 1e-8, DT, st))
    out[f"{tag} stats rinv"] = r.clone()


def p_(t):
    return t.data_ptr() if t is not None else None


def chain(tag, rows, d, DT, x, dy, g, r, pre, gen, group_rows):
    """meant_rmsnorm_bwd_chain: token-level dy with the stored x, and pooled dy (float [rows / group_rows, d]) with x from gelu_pre"""
    up_r = (0.5 + torch.rand(rows, generator=gen)).to(dev); up_b = (0.1 * torch.randn(d, generator=gen)).to(dev)
    dyp = torch.randn(rows // group_rows, d, generator=gen).to(dev)
    wsb = lib.meant_rmsnorm_bwd_ws(rows, d); ws = torch.empty(max(wsb, 16), device=dev, dtype=torch.uint8)
    for nm, dyv, pooled, xv in (("token", dy, 0, x), (f"pooled/{group_rows}", dyp, 1, None)):
        dxs = torch.empty_like(x); ds = torch.empty(d, device=dev); kc = torch.empty(rows, device=dev); db = torch.zeros(d, device=dev)
        check(lib.meant_rmsnorm_bwd_chain(p_(dyv), pooled, p_(xv), p_(g), p_(r), p_(dxs), p_(ds), rows, d, group_rows, 1e-8, 0.0, 0, p_(pre), p_(up_r),
                                          p_(up_b), 1e-8, 256, p_(kc), p_(db), DT, p_(ws), wsb, st))
        for k, v in (("dx_scaled", dxs), ("dscale", ds), ("kcoef", kc), ("dbias_up", db)):
            out[f"{tag} chain {nm} {k}"] = v.clone()


# the smallest shape of each route: packed R = 4 C = 1 | packed C = 2 | packed R = 2 C = 3 | one wave per row (odd row count) |
# one wave per row (C would be 4) | wide V = 8 | wide V = 1 | wide, two slices | one wave per row with ragged lanes (65 chunks) and a
# second grid-stride pass (more than 4 x 1024 rows)
for rows, d in ((8, 128), (4, 1024), (4, 768), (5, 768), (4, 2048), (3, 2056), (3, 100), (2, 8200), (4103, 520)):
    for DT in (1, 0):
        gen = torch.Generator().manual_seed(1000 * rows + d)
        cast = (lambda z: z.bfloat16()) if DT else (lambda z: z.float())
        x = cast(torch.randn(rows, d, generator=gen).to(dev)); dy = cast(torch.randn(rows, d, generator=gen).to(dev))
        g = (1 + 0.1 * torch.randn(d, generator=gen)).to(dev); b = (0.1 * torch.randn(d, generator=gen)).to(dev)
        r = torch.empty(rows, device=dev); stats = torch.empty(rows, 2, device=dev)
        y = torch.empty_like(x); dx = torch.empty_like(x); ds = torch.empty(d, device=dev); do = torch.empty(d, device=dev)
        wsb = lib.meant_rmsnorm_bwd_ws(rows, d); ws = torch.empty(max(wsb, 16), device=dev, dtype=torch.uint8)
        tag = f"small {rows}x{d}{'b' if DT else 'f'}"
        for nm, p, seed in (("", 0.0, 0), (" drop", 0.5, 1234)):
            check(lib.meant_rmsnorm_fwd(p_(x), p_(g), p_(y), p_(r), rows, d, 1e-8, p, seed, DT, st))
            out[f"{tag} fwd{nm} y"] = y.clone(); out[f"{tag} fwd{nm} rinv"] = r.clone()
            check(lib.meant_rmsnorm_bwd(p_(dy), p_(x), p_(g), p_(r), p_(dx), p_(ds), rows, d, 1e-8, p, seed, None, None, DT, p_(ws), wsb, st))
            out[f"{tag} bwd{nm} dx"] = dx.clone(); out[f"{tag} bwd{nm} dscale"] = ds.clone()
        for nm, dres, gp in (("bwd+dres", dy, None), ("bwd+dres+gelu", dy, x)):
            check(lib.meant_rmsnorm_bwd(p_(dy), p_(x), p_(g), p_(r), p_(dx), p_(ds), rows, d, 1e-8, 0.0, 0, p_(dres), p_(gp), DT, p_(ws), wsb, st))
            out[f"{tag} {nm} dx"] = dx.clone(); out[f"{tag} {nm} dscale"] = ds.clone()
        check(lib.meant_layernorm_fwd(p_(x), p_(g), p_(b), p_(y), p_(stats), rows, d, 1e-5, DT, st))
        out[f"{tag} ln fwd y"] = y.clone(); out[f"{tag} ln fwd stats"] = stats.clone()
        check(lib.meant_layernorm_bwd(p_(dy), p_(x), p_(g), p_(stats), p_(dx), p_(ds), p_(do), rows, d, DT, p_(ws), wsb, st))
        out[f"{tag} ln bwd dx"] = dx.clone(); out[f"{tag} ln bwd dgamma"] = ds.clone(); out[f"{tag} ln bwd dbeta"] = do.clone()
        for nm, off in (("partial", None), ("partial+offset", b)):
            check(lib.meant_rmsnorm_partial_fwd(p_(x), p_(g), p_(off), p_(y), p_(r), rows, d, d // 2, 1e-8, DT, st))
            out[f"{tag} {nm} fwd y"] = y.clone(); out[f"{tag} {nm} fwd rinv"] = r.clone()
            check(lib.meant_rmsnorm_partial_bwd(p_(dy), p_(x), p_(g), p_(r), p_(dx), p_(ds), p_(do) if off is not None else None, rows, d, d // 2, 1e-8,
                                                DT, p_(ws), wsb, st))
            out[f"{tag} {nm} bwd dx"] = dx.clone(); out[f"{tag} {nm} bwd dscale"] = ds.clone()
            if off is not None:
                out[f"{tag} {nm} bwd doffset"] = do.clone()
        if (rows, d) in ((4, 768), (8, 128)):
            check(lib.meant_rmsnorm_fwd(p_(x), p_(g), p_(y), p_(r), rows, d, 1e-8, 0.0, 0, DT, st))
            chain(tag, rows, d, DT, x, dy, g, r, dy, gen, 4)
torch.cuda.synchronize()
torch.save({k: v.cpu() for k, v in out.items()}, sys.argv[1])
