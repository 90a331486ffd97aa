"""Temporal (lag-axis) attention at lags past 64: the long-lag kernels of temporal.hip behind meant_temporal_attn_fwd / _bwd,
against fp64 on the device (core), against the CPU oracle (module and models), in both precision tiers."""
import math

import numpy as np
import pytest
import torch

from tests.util import DTYPES, IDS, TOL, t, assert_close, assert_grad_close, pair, compare_param_grads, norm_floor

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def M():
    import meant_amd
    return meant_amd


@pytest.fixture(scope="module")
def O():
    from oracle import meant_oracle
    return meant_oracle


def _raw_fwd(q, kv, B, L, H, Dh, scale):
    """the C entry point itself: returns (o, p) with p [B, H, L] the stored softmax weights"""
    from meant_amd import ops
    o = torch.empty_like(q)
    p = torch.full((B, H, L), float("nan"), device=q.device, dtype=torch.float32)
    ops.check(ops.lib.meant_temporal_attn_fwd(ops._p(q), ops._p(kv), ops._p(o), ops._p(p), B, L, H, Dh, scale, ops._dt(q), ops._stream()),
              "temporal_attn_fwd")
    return o, p


def _raw_bwd(q, kv, p, do, B, L, H, Dh, scale):
    """dq, dkv of the C entry point; the outputs start as NaN so that an element no thread wrote shows"""
    from meant_amd import ops
    dq = torch.full_like(q, float("nan"))
    dkv = torch.full_like(kv, float("nan"))
    ops.check(ops.lib.meant_temporal_attn_bwd(ops._p(q), ops._p(kv), ops._p(p), ops._p(do), ops._p(dq), ops._p(dkv), B, L, H, Dh, scale,
                                              ops._dt(q), ops._stream()), "temporal_attn_bwd")
    return dq, dkv


# (B, L, H, Dh).  The first seven are the shapes the feature was specified with; the rest are the other places where
# temporal.hip changes path: one lane per row and 64 lanes per row of the row-sweep kernels (Dh = 8, 512), the scalar
# kernels' second sweep over the head (Dh > 512), and the backward past its LDS cache of dp_l (L > 2048).
CORE_SHAPES = [
    (2, 65, 12, 128),       # one key past the cap and past one 64-key chunk
    (1, 127, 2, 64), (1, 128, 2, 64), (1, 129, 2, 64),      # the chunk boundary from both sides
    (5, 257, 3, 40),        # a head slice shorter than the lanes that sweep it (5 of 8 lanes live)
    (2, 100, 2, 100),       # Dh % 8 != 0: scalar kernels
    (1, 1000, 12, 128),     # many trips of every wave, four-wave merge
    (2, 300, 3, 8),         # one lane per row: 256 rows per trip, the second trip partly empty
    (1, 66, 1, 512),        # 64 lanes per row: one row per wave per trip, no shuffle merge
    (1, 66, 1, 520),        # Dh > 512: scalar kernels, two sweeps over the head in backward
    (1, 2050, 2, 64),       # backward recomputes dp_l from V instead of caching it in LDS
]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,L,H,Dh", CORE_SHAPES)
def test_core_against_fp64(dev, dtype, B, L, H, Dh):
    """ops.temporal_attention with identity projections and small biases against fp64 PyTorch on the same tier-rounded inputs:
    o, dx, and the six weight / bias gradients.  The key projection's bias gradient is zero in exact arithmetic (a softmax does
    not see a shift of all scores), so gradients are compared the way tests.util.compare_param_grads does: norms against
    max(reference, floor), elements only where the reference norm is above the floor."""
    from meant_amd import ops
    D = H * Dh
    gen = torch.Generator().manual_seed(1000 * L + Dh)
    x = torch.randn(B, L, D, generator=gen).to(dev).to(dtype).requires_grad_()
    do = torch.randn(B, 1, D, generator=gen).to(dev).to(dtype)
    ws = [torch.nn.Parameter(torch.eye(D, device=dev)) for _ in range(3)]
    bs = [torch.nn.Parameter((0.02 * torch.randn(D, generator=gen)).to(dev)) for _ in range(3)]
    o = ops.temporal_attention(x, ws[0], bs[0], ws[1], bs[1], ws[2], bs[2], H)
    o.backward(do)

    xd = x.detach().double().requires_grad_()
    wd = [w.detach().to(dtype).double().requires_grad_() for w in ws]
    bd = [b.detach().double().requires_grad_() for b in bs]
    q = (xd[:, -1] @ wd[0].T + bd[0]).view(B, H, Dh)
    k = (xd @ wd[1].T + bd[1]).view(B, L, H, Dh)
    v = (xd @ wd[2].T + bd[2]).view(B, L, H, Dh)
    p = torch.softmax(torch.einsum("bhd,blhd->bhl", q, k) / math.sqrt(D), dim=-1)
    od = torch.einsum("bhl,blhd->bhd", p, v).reshape(B, 1, D)
    od.backward(do.double())

    tol = TOL[dtype]
    assert o.shape == (B, 1, D) and o.dtype == dtype
    assert_close(o, od, tol["out"] * (1 if dtype == torch.float32 else 4), "o")
    assert_grad_close(x.grad, xd.grad, tol["gelem"], "dx")
    names = ["wq", "wk", "wv", "bq", "bk", "bv"]
    got, ref = [w.grad for w in ws + bs], [w.grad for w in wd + bd]
    floor = norm_floor([r.norm().item() for r in ref], dtype)
    for nm, a, r in zip(names, got, ref):
        na, nr = a.double().norm().item(), r.norm().item()
        assert abs(na - nr) <= tol["gnorm"] * max(nr, floor) + 1e-7, f"{nm}: grad norm {na} vs {nr}"
        if nr > floor:
            assert_grad_close(a, r, tol["gelem"], nm)


@pytest.mark.parametrize("peak", [0, 199], ids=["max_first", "max_last"])
def test_online_softmax_under_stress(dev, peak):
    """fp32, L = 200, H = 2, Dh = 64, scores spanning about +-60 with the largest at l = 0 (the running maximum is set by the first
    row a lane group sees) or at l = 199 (it moves in the last one).  The stored p against an fp64 softmax of the same q, k within
    TOL[float32]["out"], and |sum_l p_l - 1| <= L * 2^-23, the worst case of an fp32 sum of L terms."""
    B, L, H, Dh = 1, 200, 2, 64
    D = H * Dh
    scale = 1.0 / math.sqrt(D)
    rs = np.random.RandomState(77 + peak)
    q = rs.standard_normal((B, H, Dh))
    target = rs.uniform(-60.0, 57.0, (B, H, L))             # the score each key is built to give
    near = [(peak + 71) % L, (peak + 142) % L]
    target[:, :, near[0]], target[:, :, near[1]] = 59.0, 59.5
    target[:, :, peak] = 60.0
    qn = (q * q).sum(-1, keepdims=True)                     # [B, H, 1]
    k = q[:, None] * (target.transpose(0, 2, 1)[..., None] / (scale * qn[:, None]))     # [B, L, H, Dh]
    k = k + 0.1 * rs.standard_normal(k.shape)
    v = rs.standard_normal((B, L, H, Dh))
    qt = t(q.reshape(B, D).astype("float32")).to(dev)
    kv = t(np.concatenate([k.reshape(B * L, D), v.reshape(B * L, D)], axis=1).astype("float32")).to(dev)
    o, p = _raw_fwd(qt, kv, B, L, H, Dh, scale)

    qd = qt.double().view(B, H, Dh)
    kd, vd = kv[:, :D].double().view(B, L, H, Dh), kv[:, D:].double().view(B, L, H, Dh)
    s = torch.einsum("bhd,blhd->bhl", qd, kd) * scale
    assert (s.max(-1).values - s.min(-1).values).min().item() > 100 and (s.argmax(-1) == peak).all()
    pd = torch.softmax(s, dim=-1)
    od = torch.einsum("bhl,blhd->bhd", pd, vd).reshape(B, D)
    err = (p.double() - pd).abs().max().item()
    dsum = (p.double().sum(-1) - 1).abs().max().item()
    print(f"stress peak={peak}: max |p - p64| {err:.3e}, max |sum p - 1| {dsum:.3e} (bound {L * 2.0 ** -23:.3e})")
    assert err <= TOL[torch.float32]["out"]
    assert dsum <= L * 2.0 ** -23
    assert_close(o, od, TOL[torch.float32]["out"], "o")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_route_counter(dev, dtype):
    """L = 64 stays on the short-lag kernels, L = 65 takes the long-lag ones in forward and in backward"""
    from meant_amd import _lib
    B, H, Dh = 2, 2, 64
    D = H * Dh
    scale = 1.0 / math.sqrt(D)
    gen = torch.Generator().manual_seed(5)
    for L, want in ((64, 0), (65, 2)):
        q = torch.randn(B, D, generator=gen).to(dev).to(dtype)
        kv = torch.randn(B * L, 2 * D, generator=gen).to(dev).to(dtype)
        do = torch.randn(B, D, generator=gen).to(dev).to(dtype)
        _lib.route_reset()
        o, p = _raw_fwd(q, kv, B, L, H, Dh, scale)
        dq, dkv = _raw_bwd(q, kv, p, do, B, L, H, Dh, scale)
        torch.cuda.synchronize()
        assert _lib.route_count("temporal_long") == want, (L, _lib.route_count("temporal_long"))
        assert torch.isfinite(o.float()).all() and torch.isfinite(dq.float()).all() and torch.isfinite(dkv.float()).all()


def test_backward_bit_reproducible(dev):
    """two backward runs at (2, 257, 12, 128) in bf16 give the same dq and dkv bits (no atomics, one writer per element), and
    every element of both is written"""
    B, L, H, Dh = 2, 257, 12, 128
    D = H * Dh
    scale = 1.0 / math.sqrt(D)
    gen = torch.Generator().manual_seed(9)
    q = torch.randn(B, D, generator=gen).to(dev).to(torch.bfloat16)
    kv = torch.randn(B * L, 2 * D, generator=gen).to(dev).to(torch.bfloat16)
    do = torch.randn(B, D, generator=gen).to(dev).to(torch.bfloat16)
    _, p = _raw_fwd(q, kv, B, L, H, Dh, scale)
    dq1, dkv1 = _raw_bwd(q, kv, p, do, B, L, H, Dh, scale)
    dq2, dkv2 = _raw_bwd(q, kv, p, do, B, L, H, Dh, scale)
    assert not torch.isnan(dq1.float()).any() and not torch.isnan(dkv1.float()).any()
    assert torch.equal(dq1.view(torch.int16), dq2.view(torch.int16))
    assert torch.equal(dkv1.view(torch.int16), dkv2.view(torch.int16))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_temporal_module_lag96(M, O, dev, dtype):
    ref, hip = pair(O.temporal(12, 1536), M.temporal(12, 1536), 4321, dev)
    rs = np.random.RandomState(96)
    x = t(rs.standard_normal((3, 96, 1536)).astype("float32"))
    dy = t(rs.standard_normal((3, 1, 1536)).astype("float32"))
    xr = x.clone().requires_grad_()
    yr = ref(xr)
    yr.backward(dy)
    xh = x.to(dev).to(dtype).requires_grad_()
    y = hip(xh)
    y.backward(dy.to(dev).to(dtype))
    tol = TOL[dtype]
    assert y.shape == (3, 1, 1536)
    assert_close(y, yr, tol["out"] * (1 if dtype == torch.float32 else 4), "y")
    assert_grad_close(xh.grad, xr.grad, tol["gelem"], "dx")
    compare_param_grads(ref, hip, dtype, "temporal lag 96")


LAG = 70
MODELS = {      # the tiny dims of the meant_tiny fixture at lag 70: 128 / 128, 32 x 32 images, patch 16, S = 16, 2 heads, B = 2
    "meant": ((128, 128, 4, 32, 32, 16, LAG, 2), dict(num_heads=2, num_encoders=1, channels=4), (100, 128)),
    "meant_tweet": ((128, 4, LAG, 2), dict(num_heads=2, num_encoders=1), (100, 128)),
    "meant_vision": ((128, 4, 32, 32, 16, LAG, 2), dict(num_heads=2, num_encoders=1, channels=4), None),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cls", list(MODELS))
def test_models_lag70(M, O, dev, dtype, cls):
    """meant (temporalEncoder with norms), meant_tweet and meant_vision (without) at lag 70 against the oracle in eval mode: output
    probabilities, every parameter's gradient, and the whole temp_embedding gradient [1, 70, dim]"""
    args, kw, emb = MODELS[cls]
    mk = lambda pkg: getattr(pkg, cls)(*(list(args) + ([torch.nn.Embedding(*emb)] if emb else [])), **kw)
    ref, hip = pair(mk(O), mk(M), 1234, dev)
    r = np.random.RandomState(70)
    ids = t(r.randint(0, 100, (2, LAG, 16)).astype("int64"))
    img = t(r.standard_normal((2, LAG, 4, 32, 32)).astype("float32"))
    mask = torch.ones(2, LAG, 16)
    mask[1, :, 11:] = 0                                     # one padded sample
    inputs = {"meant": (ids, img, mask), "meant_tweet": (ids, mask), "meant_vision": (img,)}[cls]
    tgt = torch.tensor([1, 0])
    out_r = ref(*inputs)
    torch.nn.functional.cross_entropy(out_r, tgt).backward()
    hip.compute_dtype = dtype
    out = hip(*[a.to(dev) for a in inputs])
    torch.nn.functional.cross_entropy(out, tgt.to(dev)).backward()
    assert out.shape == (2, 2) and out.dtype == torch.float32
    assert_close(out, out_r, TOL[dtype]["out"], "out")
    compare_param_grads(ref, hip, dtype, f"{cls} lag {LAG}")
    key = "temporal_encoding.0.temp_embedding"
    ge, gr = dict(hip.named_parameters())[key].grad, dict(ref.named_parameters())[key].grad
    assert ge.shape == (1, LAG, hip.dim)
    assert_grad_close(ge, gr, TOL[dtype]["gelem"], key)
