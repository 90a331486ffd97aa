"""Attention at any head count: head dims and rotary dims that are no multiple of 8.

meant_rotary_qk through the C ABI against a float64 rotation on the host (forward, adjoint, what it must leave untouched); the
encoders, two models and the TimeSformer at such shapes against the oracle in both tiers, with the routes the bf16 tier takes:
heads zero-padded to a native dim of the MFMA attention kernels (never the fp32 detour), rotary tables padded to ceil8(R) identity
columns so that the projection GEMM keeps its rotary epilogue.

Tolerances are tests.util.TOL, unchanged.  Encoder outputs are token tensors whose entries reach several units; a bf16 result
carries a rounding error of 2^-9 of its own magnitude, so their `out` bound is taken relative to the largest reference value (never
below 1), as the attention tests at the C ABI do.  Model outputs are probabilities and are compared in absolute terms.  The
TimeSformer's bf16 tokens and logits are held to TOL too, or, where the tier itself misses it, to a control run on unchanged code
(test_timesformer_any_dim_head)."""

import numpy as np
import pytest
import torch

from tests.util import DTYPES, IDS, TOL, t, assert_close, assert_grad_close, pair, compare_param_grads

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1.0)


def _bits(x):
    return x.view(torch.int32 if x.dtype == torch.float32 else torch.int16)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. meant_rotary_qk at the C ABI
ROTARY_SHAPES = [(8, 6), (12, 12), (20, 10), (29, 14), (40, 20), (76, 38), (76, 48), (100, 50), (64, 32)]
GUARD = 64


def _tables(S, R, seed):
    """float32 [S, R] (qa, qb, ka, kb): an xPos-like rotation, q and k sides different"""
    pos = np.arange(S, dtype=np.float64)[:, None]
    freq = np.repeat(1.0 / (10000.0 ** (np.arange(0, R, 2) / R)), 2)[None, :] * (1.0 + 0.1 * seed)
    c, s = np.cos(pos * freq), np.sin(pos * freq)
    sc = (0.9 + 0.2 * np.arange(R) / R)[None, :] ** ((pos - S // 2) / 4.0)
    return [torch.from_numpy(a.astype(np.float32)).contiguous() for a in (c * sc, s * sc, c / sc, s / sc)]


def _rotate64(x, a, b, transpose):
    """x [T, H, Dh] float64 (row r at position r % S), a / b [S, R] float64: the map of include/meant_hip.h on lanes < R, or its adjoint"""
    S, R = a.shape
    T = x.shape[0]
    A, B = a.repeat(T // S, 1)[:, None, :], b.repeat(T // S, 1)[:, None, :]
    xr = x[..., :R]
    x0, x1 = xr[..., 0::2], xr[..., 1::2]
    a0, a1, b0, b1 = A[..., 0::2], A[..., 1::2], B[..., 0::2], B[..., 1::2]
    if not transpose:
        y0, y1 = x0 * a0 - x1 * b0, x1 * a1 + x0 * b1
    else:
        y0, y1 = x0 * a0 + x1 * b1, x1 * a1 - x0 * b0
    y = torch.stack((y0, y1), dim=-1).reshape(xr.shape)
    return torch.cat((y, x[..., R:]), dim=-1)


def _call_rotary(buf, T, S, H, Dh, R, tabs, transpose, dt):
    from meant_amd._lib import lib, check
    check(lib.meant_rotary_qk(buf.data_ptr(), T, S, H, Dh, R, *[a.data_ptr() for a in tabs], transpose, dt,
                              torch.cuda.current_stream().cuda_stream), "rotary_qk")
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "base+1"])
@pytest.mark.parametrize("Dh,R", ROTARY_SHAPES)
def test_rotary_qk_any_dims(dev, Dh, R, offset, dtype):
    """forward against float64, the adjoint by <R x, y> == <x, R^T y>, and bit-unchanged lanes >= R, v block and guard elements.
    offset = 1: the same on a base that is only element-aligned (every shape then runs pair by pair)"""
    from meant_amd import _lib
    H, S, T = 3, 5, 10
    ld, D = 3 * H * Dh, H * Dh
    dt = F32 if dtype == torch.float32 else BF16
    gen = torch.Generator().manual_seed(1000 * Dh + R)
    x = torch.randn(T, ld, generator=gen).to(dtype)
    y = torch.randn(T, ld, generator=gen).to(dtype)
    x5 = x.view(T, 3, H, Dh)
    x5[:, 2, :, ::3] = float("nan")                       # NaN sentinels in the v block ...
    x5[:, :2, :, R:][..., ::2] = float("nan")             # ... and in the lanes >= R of q and k
    tabs = [a.to(dev) for a in _tables(S, R, R % 3)]
    tabs64 = [a.double().cpu() for a in tabs]
    pairs = int(Dh % 8 != 0 or offset != 0)

    def run(src, transpose):
        store = torch.full((offset + T * ld + GUARD,), float("nan"), dtype=dtype, device=dev)
        buf = store[offset:offset + T * ld]
        buf.copy_(src.reshape(-1))
        before = _bits(store).clone()
        _lib.route_reset()
        _call_rotary(buf, T, S, H, Dh, R, tabs, transpose, dt)
        assert _lib.route_count("rotary_qk") == 1 and _lib.route_count("rotary_pairs") == pairs
        after = _bits(store)
        assert torch.equal(after[:offset], before[:offset]) and torch.equal(after[offset + T * ld:], before[offset + T * ld:]), "guard touched"
        a5, b5 = after[offset:offset + T * ld].view(T, 3, H, Dh), before[offset:offset + T * ld].view(T, 3, H, Dh)
        assert torch.equal(a5[:, 2], b5[:, 2]), "v block touched"
        assert torch.equal(a5[:, :2, :, R:], b5[:, :2, :, R:]), "lanes >= R touched"
        return buf.clone().view(T, 3, H, Dh)

    tol = TOL[dtype]["out"]
    what = f"Dh={Dh} R={R} offset={offset}"
    rx = run(x, 0)
    for blk, (a, b) in enumerate(((tabs64[0], tabs64[1]), (tabs64[2], tabs64[3]))):
        want = _rotate64(x5[:, blk].double(), a, b, False)[..., :R]
        assert _rel(rx[:, blk, :, :R], want) <= tol, f"{what}: forward block {blk} {_rel(rx[:, blk, :, :R], want):.2e}"
    y5 = y.view(T, 3, H, Dh)
    rty = run(y, 1)
    for blk, (a, b) in enumerate(((tabs64[0], tabs64[1]), (tabs64[2], tabs64[3]))):
        want = _rotate64(y5[:, blk].double(), a, b, True)[..., :R]
        assert _rel(rty[:, blk, :, :R], want) <= tol, f"{what}: adjoint block {blk}"
        xs, ys = x5[:, blk, :, :R].double(), y5[:, blk, :, :R].double()
        lhs = (rx[:, blk, :, :R].double().cpu() * ys).sum().item()
        rhs = (xs * rty[:, blk, :, :R].double().cpu()).sum().item()
        assert abs(lhs - rhs) <= tol * xs.norm().item() * ys.norm().item(), f"{what}: <Rx, y> = {lhs} but <x, R^T y> = {rhs}"


def test_rotary_qk_rejects_odd_or_oversized_rotary_dims(dev):
    from meant_amd._lib import lib
    buf = torch.zeros(10 * 3 * 3 * 20, device=dev)
    tabs = [torch.zeros(5, 24, device=dev) for _ in range(4)]
    for R in (7, 22, -2):
        rc = lib.meant_rotary_qk(buf.data_ptr(), 10, 5, 3, 20, R, *[a.data_ptr() for a in tabs], 0, F32, None)
        assert rc != 0 and b"rotary_qk" in lib.meant_last_error(), R


# ------------------------------------------------------------------------------------------------------------------------------
# 2. encoders against the oracle: forward, input gradient, every parameter gradient, both tiers
_ORACLE = {}


def _fwd_route(Dp):
    return "attn_fwd" if Dp == 64 else f"attn_fwd_d{Dp}"


def _bwd_routes(Dp):
    return ("attn_bwd", "attn_bwd1") if Dp == 64 else (f"attn_bwd_d{Dp}",)     # 64 has no counter of its own: either backward form


def _encoder_case(kind, d, H, G, S, dtype, dev):
    import meant_amd as M
    from meant_amd import _lib, ops
    from oracle import meant_oracle as O
    ref, hip = pair(getattr(O, kind)(d, H), getattr(M, kind)(d, H), 4321, dev)
    key = (kind, d, H)
    rs = np.random.RandomState(d + H + S)
    x = t(rs.standard_normal((G, S, d)).astype("float32")).bfloat16().float()    # bf16-exact: one oracle run serves both tiers
    dy = t(rs.standard_normal((G, S, d)).astype("float32")).bfloat16().float()
    mask = None
    if kind == "languageEncoder":
        mask = torch.ones(G, S)
        mask[0, S // 3:] = 0
        mask[G - 1, :] = 0                                                       # one fully padded row
    if key not in _ORACLE:
        xr = x.clone().requires_grad_()
        yr = ref(xr, mask) if mask is not None else ref(xr)
        yr.backward(dy)
        _ORACLE[key] = (yr.detach(), xr.grad.clone(), {k: p.grad.clone() for k, p in ref.named_parameters() if p.grad is not None})
    yr, dxr, grads = _ORACLE[key]
    for k, p in ref.named_parameters():
        p.grad = grads.get(k)
    Dh = d // H
    R = hip.encode[2].pos_emb.rot_dim if kind == "visionEncoder" else hip.encode[2].xPos.rot_dim
    bf16 = dtype == torch.bfloat16
    Dp = ops.run_head_dim(Dh, dtype)
    R8 = (R + 7) & ~7
    tol = TOL[dtype]
    # bf16 tier at S <= 16 and a head padded to 64 / 96 / 128: the short-sequence kernels by default, the tiled flash kernels with
    # that option off; both are native routes, both are run
    shorts = (1, 0) if bf16 and S <= 16 and Dp <= 128 else (1,)
    old = _lib.get_option("attn_short")
    try:
        for short in shorts:
            what = f"{kind}({d}, {H}) {dtype} attn_short={short}"
            _lib.set_option("attn_short", short)
            hip.zero_grad(set_to_none=True)
            xh = x.to(dev).to(dtype).requires_grad_()
            _lib.route_reset()
            yh = hip(xh, mask.to(dev)) if mask is not None else hip(xh)
            torch.cuda.synchronize()
            fwd = {r: _lib.route_count(r) for r in ("nt_rot", "rotary_qk", "attn_short") + ((_fwd_route(Dp),) if bf16 else ())}
            yh.backward(dy.to(dev).to(dtype))
            torch.cuda.synchronize()
            assert _lib.route_count("attn_generic") == 0, f"{what}: fp32 detour"
            if bf16:
                assert Dp in ops.NATIVE_HEAD_DIMS and R8 <= Dp
                # the projection rotated in its GEMM epilogue: exactly one NT GEMM with the rotary epilogue, no rotary launch of its own
                assert fwd["nt_rot"] == 1 and fwd["rotary_qk"] == 0, f"{what}: {fwd}"
                if short and len(shorts) == 2:
                    assert _lib.route_count("attn_short") == 2, f"{what}: {fwd}"
                else:
                    assert fwd[_fwd_route(Dp)] == 1 and fwd["attn_short"] == 0, f"{what}: {fwd}"
                    assert sum(_lib.route_count(r) for r in _bwd_routes(Dp)) == 1, what
                # the backward's adjoint inside the kernels up to 64 rotary lanes, one meant_rotary_qk launch on 16-byte chunks above
                assert _lib.route_count("rotary_qk") == int(R8 > 64) and _lib.route_count("rotary_pairs") == 0, what
            else:
                # fp32 tier: the rotation and its adjoint by meant_rotary_qk, pair by pair where the head is off the 8-grid
                assert _lib.route_count("rotary_qk") == 2 and _lib.route_count("rotary_pairs") == (2 if Dh % 8 else 0), what
            print(f"{what}: out {_rel(yh, yr):.3e} dx {_rel(xh.grad, dxr):.3e}")
            assert _rel(yh, yr) <= tol["out"], f"{what}: out {_rel(yh, yr):.3e}"
            assert_grad_close(xh.grad, dxr, tol["gelem"], f"{what}: dx")
            compare_param_grads(ref, hip, dtype, what)
    finally:
        _lib.set_option("attn_short", old)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d,H", [(40, 2), (80, 2), (88, 3), (152, 2), (344, 2)])
def test_vision_encoder_any_heads(dev, d, H, dtype):
    """Dh / R = 20 / 10, 40 / 20, 29 / 14, 76 / 38, 172 / 86 at 5 tokens: bf16 heads padded to 64, 128, 64, 96, 192"""
    _encoder_case("visionEncoder", d, H, 3, 5, dtype, dev)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d,H", [(152, 2), (200, 2)])
def test_language_encoder_any_heads(dev, d, H, dtype):
    """Dh = 76 and 100 with the 48 xPos lanes, causal, S = 80 with a key-padding mask that has one fully padded row: bf16 heads padded
    to 96 and 128"""
    _encoder_case("languageEncoder", d, H, 3, 80, dtype, dev)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. models against the oracle
def _model_case(ref, hip, inputs, tgt, dtype, dev, what):
    from meant_amd import _lib
    key = what
    if key not in _ORACLE:
        out_r = ref(*inputs)
        torch.nn.functional.cross_entropy(out_r, tgt).backward()
        _ORACLE[key] = (out_r.detach(), {k: p.grad.clone() for k, p in ref.named_parameters() if p.grad is not None})
    out_r, grads = _ORACLE[key]
    for k, p in ref.named_parameters():
        p.grad = grads.get(k)
    hip.compute_dtype = dtype
    _lib.route_reset()
    out = hip(*[a.to(dev) for a in inputs])
    torch.nn.functional.cross_entropy(out, tgt.to(dev)).backward()
    torch.cuda.synchronize()
    assert _lib.route_count("attn_generic") == 0, f"{what}: fp32 detour"
    print(f"{what} {dtype}: out {(out.float().cpu() - out_r).abs().max().item():.3e}")
    assert_close(out, out_r, TOL[dtype]["out"], f"{what}: out")
    compare_param_grads(ref, hip, dtype, what)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_meant_vision_image_dim_40_two_heads(dev, dtype):
    import meant_amd as M
    from oracle import meant_oracle as O
    kw = dict(image_dim=40, price_dim=4, height=32, width=32, patch_res=16, lag=2, num_classes=2, num_heads=2)
    ref, hip = pair(O.meant_vision(**kw), M.meant_vision(**kw), 1234, dev)
    r = np.random.RandomState(40)
    img = t(r.standard_normal((3, 2, 4, 32, 32)).astype("float32"))
    _model_case(ref, hip, (img,), torch.tensor([1, 0, 1]), dtype, dev, "meant_vision_40_h2")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_meant_text_152_image_40_two_heads(dev, dtype):
    """language heads of 76 columns (48 xPos lanes), vision heads of 20 (10 rotary lanes), temporal heads of 96"""
    import meant_amd as M
    from oracle import meant_oracle as O
    args, kw = (152, 40, 4, 32, 32, 16, 2, 2), dict(num_heads=2, num_encoders=1, channels=4)
    ref = O.meant(*args, torch.nn.Embedding(100, 152), **kw)
    hip = M.meant(*args, torch.nn.Embedding(100, 152), **kw)
    ref, hip = pair(ref, hip, 1234, dev)
    r = np.random.RandomState(152)
    ids = t(r.randint(0, 100, (3, 2, 21)).astype("int64"))
    img = t(r.standard_normal((3, 2, 4, 32, 32)).astype("float32"))
    mask = torch.ones(3, 2, 21)
    mask[1, :, 13:] = 0
    mask[2, 1, 1:] = 0
    _model_case(ref, hip, (ids, img, mask), torch.tensor([1, 0, 1]), dtype, dev, "meant_152_40_h2")


# ------------------------------------------------------------------------------------------------------------------------------
# 4. TimeSformer at dim_head 12, 20, 50
def _embedded_control(hip, kw, dim_head, Dp, dev):
    """The same function on code this feature leaves alone: a TimeSformer at the on-grid dim_head = Dp whose to_qkv / to_out weights
    are those of `hip` with every head zero-padded to Dp, the scale of the real dim_head, and `hip`'s rotary tables and index plan.
    Dp % 8 == 0, so its forward takes no padding branch of its own."""
    import meant_amd as M
    H = kw["heads"]
    ctl = M.TimeSformer(**dict(kw, dim_head=Dp))
    sd = {k: v for k, v in hip.state_dict().items() if "rot_emb" not in k}
    for k in list(sd):
        if k.endswith("fn.to_qkv.weight"):
            w = sd[k]
            sd[k] = torch.nn.functional.pad(w.view(3 * H, dim_head, w.shape[1]), (0, 0, 0, Dp - dim_head)).reshape(3 * H * Dp, w.shape[1])
        elif k.endswith("fn.to_out.0.weight"):
            w = sd[k]
            sd[k] = torch.nn.functional.pad(w.view(w.shape[0], H, dim_head), (0, Dp - dim_head)).reshape(w.shape[0], H * Dp)
    missing, unexpected = ctl.load_state_dict(sd, strict=False)
    assert not unexpected and all("rot_emb" in k for k in missing), (missing, unexpected)
    ctl = ctl.to(dev).eval()
    for ta, sa, _ in ctl.layers:
        ta.fn.scale = sa.fn.scale = dim_head ** -0.5
    ctl._cache = dict(hip._cache)                                                # same rotary tables (identity columns included), same regrouping
    return ctl


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rotary", [True, False], ids=["rotary", "posemb"])
@pytest.mark.parametrize("dim_head", [12, 20, 50])
def test_timesformer_any_dim_head(dev, dim_head, rotary, dtype):
    """heads zero-padded to 64 (bf16) or ceil8 (fp32) in the to_qkv weight, rotary tables of 12 / 20 / 50 (frames) and 12 / 20 / 48
    (axial) lanes padded to the 8-grid; against oracle.TimeSformer in float64: every gradient by compare_param_grads, tokens and
    logits at TOL's `out` bound relative to the largest value.

    bf16 tier: this model's tokens and logits sit at or beyond TOL's 1e-2 whatever the head dim (measured on code this feature does
    not touch, dim_head 8 / 16 / 24 / 64: tokens 0.6-0.9e-2, logits 0.5-2.5e-2 -- six logits behind a LayerNorm and a 48 -> 3 head).
    The bound is therefore tied to a control run in the same test (_embedded_control): the same function at dim_head = 64 through
    the unchanged code.  Control and padded run feed the same kernels the same values up to the K-tiling of to_out (K = 2 dim_head
    against 128, the extra products exact zeros), so
      * they agree to a final bf16 rounding, at most 2^-7 of a value: asserted at TOL's 1e-2 of the largest value;
      * against float64 the padded run may miss TOL only where the control misses it too, and then by no more than 1.5 x the
        control's error (a control error of a few roundings plus one more)."""
    import meant_amd as M
    from meant_amd import _lib, ops
    from oracle import meant_oracle as O
    kw = dict(dim=48, num_frames=2, num_classes=3, image_size=32, patch_size=16, channels=3, depth=1, heads=2, dim_head=dim_head,
              rotary_emb=rotary)
    ref, hip = pair(O.TimeSformer(**kw), M.TimeSformer(**kw), 4321, dev)
    ref = ref.double()
    rs = np.random.RandomState(dim_head)
    video = torch.from_numpy(rs.standard_normal((2, 2, 3, 32, 32)).astype("float32"))
    target = torch.tensor([1, 2])
    key = ("ts", dim_head, rotary)
    if key not in _ORACLE:
        x_r = ref.meant_forward(video.double())
        logits_r = ref.to_out(x_r[:, 0])
        torch.nn.functional.cross_entropy(logits_r, target).backward()
        _ORACLE[key] = (x_r.detach(), logits_r.detach(), {k: p.grad.clone() for k, p in ref.named_parameters() if p.grad is not None})
    x_r, logits_r, grads = _ORACLE[key]
    for k, p in ref.named_parameters():
        p.grad = grads.get(k)
    hip.compute_dtype = dtype
    _lib.route_reset()
    x = hip.meant_forward(video.to(dev))
    logits = hip.to_out(x[:, 0])
    torch.nn.functional.cross_entropy(logits.float(), target.to(dev)).backward()
    torch.cuda.synchronize()
    what = f"TimeSformer dim_head={dim_head} rotary={rotary} {dtype}"
    assert _lib.route_count("attn_generic") == 0, f"{what}: fp32 detour"
    assert _lib.route_count("attn_cls") == 2, what                               # the cls query of the time and of the space half
    tol = TOL[dtype]["out"]
    ex, el = _rel(x, x_r), _rel(logits, logits_r)
    if dtype == torch.float32:
        print(f"{what}: tokens {ex:.3e} logits {el:.3e}")
        assert ex <= tol, f"{what}: tokens {ex:.3e}"
        assert el <= tol, f"{what}: logits {el:.3e}"
    else:
        assert _lib.route_count("attn_short") == 4, what                         # groups of 3 and 5 tokens at the padded head dim 64
        Dp = ops.divided_head_dim(dim_head, dtype)
        ctl = _embedded_control(hip, kw, dim_head, Dp, dev)
        ctl.compute_dtype = dtype
        _lib.route_reset()
        with torch.no_grad():
            x_c = ctl.meant_forward(video.to(dev))
            logits_c = ctl.to_out(x_c[:, 0])
        torch.cuda.synchronize()
        assert _lib.route_count("attn_generic") == 0 and _lib.route_count("attn_short") == 2, f"{what}: control off the native kernels"
        cx, cl = _rel(x_c, x_r), _rel(logits_c, logits_r)
        dx, dl = _rel(x, x_c), _rel(logits, logits_c)
        print(f"{what}: tokens {ex:.3e} (control {cx:.3e}, padded - control {dx:.3e}) logits {el:.3e} (control {cl:.3e}, padded - control {dl:.3e})")
        assert dx <= tol, f"{what}: tokens differ from the control by {dx:.3e}"
        assert dl <= tol, f"{what}: logits differ from the control by {dl:.3e}"
        assert ex <= max(tol, 1.5 * cx), f"{what}: tokens {ex:.3e}, control {cx:.3e}"
        assert el <= max(tol, 1.5 * cl), f"{what}: logits {el:.3e}, control {cl:.3e}"
    compare_param_grads(ref, hip, dtype, what)
