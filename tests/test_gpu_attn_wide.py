"""bf16 attention at head dims 160, 192 and 256 (csrc/attn_bf16.hip: the flash forward and the dQ + dK/dV backward at three or
four 64-column sub-tiles; the dK/dV pass at 256 splits its columns over two workgroups).  Through the C ABI against float64 on the
host (outputs, the (m, log2 l) statistics, dQ / dK / dV, the rotary adjoint in the backward), which route every call takes, bit
reproducibility, the zero-padding of other head dims up to them in ops.qkv_attention, and modules and models that reach them
against the oracle.  The workspace test at the end needs no GPU."""
import math

import numpy as np
import pytest
import torch

from tests.attn_ref import BF16, LOG2E, _check, _mask, _reference, _rel, _run
from tests.util import TOL, t, assert_close, assert_grad_close, pair, compare_param_grads

WIDE = (160, 192, 256)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rot_tables(S, R, xpos, seed):
    """float32 [S, R] tables (qa, qb, ka, kb) of a rotation in pairs: y[2j] = a[2j] x[2j] - b[2j] x[2j+1],
    y[2j+1] = a[2j+1] x[2j+1] + b[2j+1] x[2j]; xpos: q scaled by s^pos, k by s^-pos"""
    pos = np.arange(S, dtype=np.float64)[:, None]
    freq = np.repeat(1.0 / (10000.0 ** (np.arange(0, R, 2) / R)), 2)[None, :] * (1.0 + 0.1 * seed)
    c, s = np.cos(pos * freq), np.sin(pos * freq)
    sc = (0.9 + 0.2 * np.arange(R) / R)[None, :] ** ((pos - S // 2) / 64.0) if xpos else np.ones((1, R))
    return [torch.from_numpy(a.astype(np.float32)) for a in (c * sc, s * sc, c / sc, s / sc)]


def _inputs(G, S, H, Dh, seed, dev):
    gen = torch.Generator().manual_seed(seed)
    qkv = torch.randn(G * S, 3 * H * Dh, generator=gen).bfloat16().to(dev)
    do = torch.randn(G * S, H * Dh, generator=gen).bfloat16().to(dev)
    return qkv, do


def _assert_native(routes, Dh, what):
    assert routes[f"attn_fwd_d{Dh}"] == 1 and routes[f"attn_bwd_d{Dh}"] == 1, f"{what}: {routes}"
    assert routes["attn_generic"] == 0 and routes["attn_short"] == 0 and routes["attn_bwd1"] == 0, f"{what}: {routes}"


# ------------------------------------------------------------------------------------------------------------------------------
# 1 + 2. the C ABI against float64, and the route of every call
MASKS = ("none", "suffix", "holes", "dead_group")


@pytest.mark.gpu
@pytest.mark.parametrize("mask_kind", MASKS)
@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("S", [1, 5, 16, 17, 64, 130, 196, 512])
@pytest.mark.parametrize("Dh", WIDE)
def test_wide_attention_against_float64(dev, Dh, S, causal, mask_kind):
    G, H = (3, 2) if S <= 196 else (2, 2)
    seed = Dh * 1000 + S * 10 + causal + 3 * MASKS.index(mask_kind)
    qkv, do = _inputs(G, S, H, Dh, seed, dev)
    mask = _mask(mask_kind, G, S, np.random.RandomState(seed))
    scale = 0.7 / math.sqrt(Dh)                     # not the modules' 1/sqrt(H*Dh): the caller's scale is what the kernels use
    o, lse, dqkv, routes = _run(qkv, do, mask, G, S, H, Dh, scale, causal)
    what = f"Dh={Dh} S={S} causal={causal} mask={mask_kind}"
    _assert_native(routes, Dh, what)
    _check(o, lse, dqkv, _reference(qkv, do, mask, G, S, H, Dh, scale, causal), H, Dh, what)
    if mask_kind == "dead_group":                    # every key of group 0 masked: a uniform softmax over its visible keys
        o0, v0 = o[:S].double().cpu().view(S, H, Dh), qkv[:S, 2 * H * Dh:].double().cpu().view(S, H, Dh)
        vis = torch.arange(1, S + 1, dtype=torch.float64)[:, None, None] if causal else float(S)
        uni = v0.cumsum(0) / vis if causal else v0.mean(0, keepdim=True).expand(S, H, Dh)
        assert _rel(o0, uni) <= TOL[torch.bfloat16]["out"], f"{what}: group 0 not uniform"


# ------------------------------------------------------------------------------------------------------------------------------
# 3. rotary adjoint in the backward: R <= 64 in the kernels' epilogue, R > 64 by the adjoint after a table-free backward
@pytest.mark.gpu
@pytest.mark.parametrize("Dh", WIDE)
@pytest.mark.parametrize("R,causal,S", [(48, 1, 130), (80, 0, 196), ("Dh", 0, 64)])
def test_wide_attention_rotary_backward(dev, Dh, R, causal, S):
    R = Dh if R == "Dh" else R
    G, H = 3, 2
    seed = 7 * Dh + R + S
    qkv, do = _inputs(G, S, H, Dh, seed, dev)
    mask = _mask("suffix", G, S, np.random.RandomState(seed))
    tables = _rot_tables(S, R, xpos=(R == 48), seed=R % 3)
    scale = 1.0 / math.sqrt(H * Dh)
    o, lse, dqkv, routes = _run(qkv, do, mask, G, S, H, Dh, scale, causal, tables)
    what = f"Dh={Dh} R={R}"
    _assert_native(routes, Dh, what)
    _check(o, lse, dqkv, _reference(qkv, do, mask, G, S, H, Dh, scale, causal, tables), H, Dh, what)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. determinism: no float atomics, so the same backward twice is the same bits
@pytest.mark.gpu
@pytest.mark.parametrize("Dh", WIDE)
def test_wide_attention_is_bit_reproducible(dev, Dh):
    G, S, H = 24, 512, 2
    qkv, do = _inputs(G, S, H, Dh, 99 + Dh, dev)
    mask = _mask("suffix", G, S, np.random.RandomState(Dh))
    tables = _rot_tables(S, 48, True, 0)
    scale = 1.0 / math.sqrt(H * Dh)
    o1, _, d1, r1 = _run(qkv, do, mask, G, S, H, Dh, scale, 1, tables)
    o2, _, d2, r2 = _run(qkv, do, mask, G, S, H, Dh, scale, 1, tables)
    _assert_native(r1, Dh, "run 1")
    assert torch.equal(o1, o2), "forward output differs"
    ne = d1.view(torch.int16) != d2.view(torch.int16)
    assert not ne.any(), f"{int(ne.sum())} gradient elements differ between two runs"


# ------------------------------------------------------------------------------------------------------------------------------
# 5. ops.qkv_attention pads head dims 136..248 (multiples of 8) up to the next native dim
def _module_pair(kind, H, d, dev, seed=4321):
    import meant_amd as M
    from oracle import meant_oracle as O
    if kind == "pixel":
        ref = O.attention(H, d, O.RotaryTable(math.floor(d / H / 2), "pixel"))
        hip = M.attention(H, d, M.RotaryEmbedding(dim=math.floor(d / H / 2), freqs_for="pixel"))
    else:
        ref = O.xPosAttention(H, d, O.RotaryTable(48, "lang", use_xpos=True))
        hip = M.xPosAttention(H, d, M.RotaryEmbedding(dim=48, use_xpos=True))
    return pair(ref, hip, seed, dev)


def _module_case(kind, H, d, G, S, dev, mask_rows=True):
    from meant_amd import _lib
    ref, hip = _module_pair(kind, H, d, dev)
    rs = np.random.RandomState(d + S)
    x = t(rs.standard_normal((G, S, d)).astype("float32"))
    dy = t(rs.standard_normal((G, S, d)).astype("float32"))
    mask = torch.ones(G, S)
    if mask_rows:
        mask[0, S // 3:] = 0
        mask[G - 1, :] = 0
    xq, dyq = x.bfloat16().float(), dy.bfloat16().float()
    xr = xq.clone().requires_grad_()
    yr = ref(xr, mask) if kind == "xpos" else ref(xr)
    yr.backward(dyq)
    _lib.route_reset()
    xh = x.to(dev).bfloat16().requires_grad_()
    yh = hip(xh, mask.to(dev)) if kind == "xpos" else hip(xh)
    yh.backward(dy.to(dev).bfloat16())
    torch.cuda.synchronize()
    routes = {r: _lib.route_count(r) for r in ("attn_fwd_d160", "attn_fwd_d192", "attn_fwd_d256", "attn_bwd_d160", "attn_bwd_d192",
                                               "attn_bwd_d256", "attn_generic")}
    tol = TOL[torch.bfloat16]
    assert_close(yh, yr, tol["out"] * 4, "y")
    assert_grad_close(xh.grad, xr.grad, tol["gelem"], "dx")
    compare_param_grads(ref, hip, torch.bfloat16, f"{kind}_{H}x{d // H}")
    return routes


@pytest.mark.gpu
@pytest.mark.parametrize("kind,H,Dh,Dp", [("xpos", 2, 144, 160), ("pixel", 2, 176, 192), ("xpos", 1, 200, 256)])
def test_qkv_attention_pads_to_the_next_native_dim(dev, kind, H, Dh, Dp):
    from meant_amd import ops
    assert ops._padded_head_dim(Dh) == Dp
    routes = _module_case(kind, H, H * Dh, 3, 70, dev)
    assert routes[f"attn_fwd_d{Dp}"] == 1 and routes[f"attn_bwd_d{Dp}"] == 1 and routes["attn_generic"] == 0, routes


# ------------------------------------------------------------------------------------------------------------------------------
# 6. modules and models against the oracle in the bf16 tier
@pytest.mark.gpu
@pytest.mark.parametrize("kind,H,d,Dh,S", [("pixel", 8, 1280, 160, 196), ("xpos", 8, 1536, 192, 130)])
def test_wide_attention_modules(dev, kind, H, d, Dh, S):
    """attention(8, 1280): Dh 160 with the pixel rotary of 80 lanes (the adjoint after the backward); xPosAttention(8, 1536): Dh 192,
    48 xPos lanes in the kernels' epilogue, a padding mask with a fully padded group"""
    routes = _module_case(kind, H, d, 3, S, dev)
    assert routes[f"attn_fwd_d{Dh}"] == 1 and routes[f"attn_bwd_d{Dh}"] == 1 and routes["attn_generic"] == 0, routes


@pytest.mark.gpu
def test_meant_1024_1280_heads8_vision_attention_is_native(dev):
    """meant(1024, 1280, num_heads=8): the vision encoder's attention at Dh 160 on the native kernels, every parameter gradient"""
    import meant_amd as M
    from meant_amd import _lib
    from oracle import meant_oracle as O
    args, kw = (1024, 1280, 4, 32, 32, 16, 2, 3), dict(num_heads=8, num_encoders=1, channels=4)
    ref = O.meant(*args, torch.nn.Embedding(100, 1024), **kw)
    hip = M.meant(*args, torch.nn.Embedding(100, 1024), **kw)
    ref, hip = pair(ref, hip, 1234, dev)
    r = np.random.RandomState(8)
    ids = t(r.randint(0, 100, (2, 2, 16)).astype("int64"))
    img = t(r.standard_normal((2, 2, 4, 32, 32)).astype("float32"))
    mask = torch.ones(2, 2, 16)
    mask[1, :, 11:] = 0
    tgt = torch.tensor([2, 0])
    out_r = ref(ids, img, mask)
    torch.nn.functional.cross_entropy(out_r, tgt).backward()
    hip.compute_dtype = torch.bfloat16
    _lib.route_reset()
    out = hip(ids.to(dev), img.to(dev), mask.to(dev))
    torch.nn.functional.cross_entropy(out, tgt.to(dev)).backward()
    torch.cuda.synchronize()
    assert _lib.route_count("attn_fwd_d160") >= 1 and _lib.route_count("attn_bwd_d160") >= 1
    assert _lib.route_count("attn_generic") == 0
    assert_close(out, out_r, TOL[torch.bfloat16]["out"], "out")
    compare_param_grads(ref, hip, torch.bfloat16, "meant_1024_1280_h8")


@pytest.mark.gpu
def test_timesformer_dim_head_256(dev):
    """TimeSformer(dim_head=256): the space and time halves of divided attention on the 256-wide kernels, the rotary over all 256
    lanes by the adjoint after the backward; against oracle.TimeSformer in float64"""
    import meant_amd as M
    from meant_amd import _lib
    from oracle import meant_oracle as O
    kw = dict(dim=128, heads=2, dim_head=256, num_frames=4, image_size=64, depth=1, num_classes=3, patch_size=16, channels=3)
    ref, hip = pair(O.TimeSformer(**kw), M.TimeSformer(**kw), 4321, dev)
    ref = ref.double()
    rs = np.random.RandomState(256)
    video = torch.from_numpy(rs.standard_normal((2, 4, 3, 64, 64)).astype("float32"))
    target = torch.tensor([1, 2])
    x_r = ref.meant_forward(video.double())
    logits_r = ref.to_out(x_r[:, 0])
    torch.nn.functional.cross_entropy(logits_r, target).backward()
    hip.compute_dtype = torch.bfloat16
    _lib.route_reset()
    x = hip.meant_forward(video.to(dev))
    logits = hip.to_out(x[:, 0])
    torch.nn.functional.cross_entropy(logits.float(), target.to(dev)).backward()
    torch.cuda.synchronize()
    assert _lib.route_count("attn_fwd_d256") >= 2 and _lib.route_count("attn_bwd_d256") >= 2     # space + time halves
    assert _lib.route_count("attn_generic") == 0
    assert _rel(x, x_r) <= 4e-2, f"tokens {_rel(x, x_r):.2e}"
    assert _rel(logits, logits_r) <= 4e-2
    compare_param_grads(ref, hip, torch.bfloat16, "timesformer_dh256")


# ------------------------------------------------------------------------------------------------------------------------------
# 7. workspace (host only)
@pytest.mark.parametrize("Dh", WIDE)
def test_wide_workspace(Dh):
    from meant_amd._lib import lib
    for G, S, H in ((384, 196, 8), (128 * 12, 197, 8), (64, 512, 4)):
        full, fwd = lib.meant_attn_ws(G, S, H, Dh, BF16), lib.meant_attn_fwd_ws(G, S, H, Dh, BF16)
        detour = 32 * G * S * H * Dh                    # what the fp32 detour's four copies alone take
        assert 0 < fwd < full, (G, S, H, fwd, full)
        assert full * 8 < detour, (G, S, H, full, detour)


# ------------------------------------------------------------------------------------------------------------------------------
# 7. the route table of the bf16 entry points: which counters one forward + one backward move, at every head-dim tier
ATTN_ROUTES = ("attn_fwd", "attn_fwd_d96", "attn_fwd_d128", "attn_fwd_d160", "attn_fwd_d192", "attn_fwd_d256", "attn_bwd", "attn_bwd_d96",
               "attn_bwd_d128", "attn_bwd_d160", "attn_bwd_d192", "attn_bwd_d256", "attn_bwd1", "attn_generic", "attn_short", "attn_cls")
ROUTE_TABLE = [(17, 64, None, {"attn_fwd": 1, "attn_bwd1": 1}),
               (17, 64, ("attn_bwd1", 0), {"attn_fwd": 1, "attn_bwd": 1}),
               (17, 72, None, {"attn_generic": 2}),
               (16, 64, None, {"attn_short": 2})] + \
              [(17, n, None, {f"attn_fwd_d{n}": 1, "attn_bwd": 1, f"attn_bwd_d{n}": 1}) for n in (96, 128, 160, 192, 256)]


@pytest.mark.gpu
@pytest.mark.parametrize("S,Dh,option,expected", ROUTE_TABLE, ids=[f"S{s}-Dh{n}" + ("-two_pass" if o else "") for s, n, o, _ in ROUTE_TABLE])
def test_attention_route_table(dev, S, Dh, option, expected):
    """the forward hits attn_fwd at Dh = 64 only and attn_fwd_dN otherwise; the two-pass backward hits attn_bwd at every head dim and
    attn_bwd_dN on top at N != 64; every other attn_* counter stays 0.  No mask, not causal; results against float64 as above."""
    from meant_amd import _lib
    G, H = 2, 2
    qkv, do = _inputs(G, S, H, Dh, 31 * Dh + S, dev)
    scale = 0.7 / math.sqrt(Dh)
    old = _lib.get_option(option[0]) if option else None
    try:
        if option:
            _lib.set_option(*option)
        o, lse, dqkv, counts = _run(qkv, do, None, G, S, H, Dh, scale, 0, route_names=ATTN_ROUTES)   # counters reset, one forward, one backward
    finally:
        if option:
            _lib.set_option(option[0], old)
    assert counts == {r: expected.get(r, 0) for r in ATTN_ROUTES}, f"S={S} Dh={Dh} {option}: {counts}"
    if expected.get("attn_generic"):                 # the detour is the f32 tier's core: its (m, log l) are in natural-log units
        lse = lse * LOG2E                            # (include/meant_hip.h, "attention core"); _check compares in log2 units
    _check(o, lse, dqkv, _reference(qkv, do, None, G, S, H, Dh, scale, 0), H, Dh, f"route table S={S} Dh={Dh} {option}")
