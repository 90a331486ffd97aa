"""Divided space-time attention (meant_amd.TimeSformer, csrc/divided.hip) at the shapes DESIGN tunes for -- dim 768, 12 frames of
224^2, 12 heads of 64 -- and at the widths / head dims the constructor accepts, against float64 references on the host:
  1. the kernels through the C ABI: the cls query's attention (meant_attn_cls_fwd / _bwd) up to the LDS limit, the token shift
     and its adjoint, the group scatter on TimeSformer._plan's tables, GEGLU;
  2. ops.divided_attention (both halves) against the oracle's _TSAttention core, with the launch routes pinned so that the space
     half stays on the tiled flash kernels;
  3. meant_amd.TimeSformer against oracle.TimeSformer (float64), every parameter gradient element-wise."""
import numpy as np
import pytest
import torch

from tests.attn_ref import _cls_grad_given_out, _cls_reference
from tests.util import DTYPES, IDS, TOL, assert_close, assert_grad_close, compare_param_grads, pair

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED = -2
CLS_THREADS = 256
LDS_BYTES = 160 * 1024 - 1024          # what cls_check lets a workgroup take


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _lib():
    from meant_amd import _lib as L
    return L


def _rel(a, b):
    """max-abs error of a against the float64 reference b, over b's largest magnitude"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def cls_max_len(Dh, arrays):
    """the largest L cls_check accepts: (arrays * L + 4 reduction words + rpi * Dh partials) floats within the LDS budget"""
    rpi = CLS_THREADS // (Dh // 8)
    return (LDS_BYTES // 4 - 4 - rpi * Dh) // arrays


# ------------------------------------------------------------------------------------------------------------------------------
# 1. kernels through the C ABI
# ------------------------------------------------------------------------------------------------------------------------------
def _cls_masks(B, L, rs):
    m_rand = torch.from_numpy((rs.rand(B, L) > 0.5).astype("float32"))
    m_key0 = torch.zeros(B, L)
    m_key0[:, 0] = 1
    return {"none": None, "random": m_rand, "key0": m_key0, "all": torch.zeros(B, L)}


def _run_cls(dev, dtype, B, L, H, Dh, seed):
    from meant_amd.ops import _dt, _p, _stream, check
    lib = _lib().lib
    rs = np.random.RandomState(seed)
    D = H * Dh
    ld_out = D + 8                                                   # strided output rows: the pad columns must stay untouched
    scale = Dh ** -0.5
    qkv = torch.from_numpy(rs.standard_normal((B, L, 3 * D)).astype("float32")).to(dtype)
    qkv[:, 0, :D] *= 2.0                                             # a sharper softmax
    dout = torch.from_numpy(rs.standard_normal((B, ld_out)).astype("float32")).to(dtype)
    qkv_d, dout_d = qkv.to(dev), dout.to(dev)
    tol_o, tol_g = (1e-4, 1e-3) if dtype == torch.float32 else (8e-3, 2e-2)
    for name, mask in _cls_masks(B, L, rs).items():
        what = f"cls[{name}] B={B} L={L} H={H} Dh={Dh}"
        o_ref, g_ref, mx_ref, lse_ref = _cls_reference(qkv, mask, H, Dh, scale, dout[:, :D])
        out = torch.full((B, ld_out), 7.0, device=dev, dtype=dtype)
        stats = torch.empty((B, H, 2), device=dev, dtype=torch.float32)
        km = mask.to(dev).contiguous() if mask is not None else None
        check(lib.meant_attn_cls_fwd(_p(qkv_d), _p(out), ld_out, _p(stats), _p(km), B, L, H, Dh, scale, _dt(qkv_d), _stream()), "attn_cls_fwd")
        # accumulate contract: row 0's q block gets dQ, every row's k / v blocks get dK / dV, nothing else is touched.  The buffer
        # is pre-filled at each block's gradient scale so that after - before resolves the gradient in bf16 too.
        # A block whose gradient is structurally zero (dQ, dK with only key 0 live) is held to a floor of the largest gradient.
        g_exact = _cls_grad_given_out(qkv, mask, H, Dh, scale, dout[:, :D], o_ref)
        assert torch.allclose(g_exact, g_ref.view(B, L, 3, D), rtol=1e-9, atol=1e-9 * g_ref.abs().max().item()), f"{what}: reference"
        g3 = _cls_grad_given_out(qkv, mask, H, Dh, scale, dout[:, :D], out.cpu()[:, :D])
        floor = 1e-2 * max(g3.abs().max().item(), 1e-3)
        before = torch.from_numpy(rs.standard_normal((B, L, 3, D)).astype("float32"))
        for i in range(3):
            before[:, :, i] *= max(g3[:, :, i].abs().max().item(), floor)
        before = before.view(B, L, 3 * D).to(dtype)
        dqkv = before.to(dev)
        check(lib.meant_attn_cls_bwd(_p(qkv_d), _p(out), ld_out, _p(dout_d), ld_out, _p(stats), _p(km), _p(dqkv), B, L, H, Dh, scale,
                                     _dt(qkv_d), _stream()), "attn_cls_bwd")
        torch.cuda.synchronize()
        out_c, stats_c, after = out.cpu(), stats.cpu(), dqkv.cpu()
        assert _rel(out_c[:, :D], o_ref) <= tol_o, f"{what}: output {_rel(out_c[:, :D], o_ref):.2e}"
        assert torch.all(out_c[:, D:] == 7.0), f"{what}: wrote past H*Dh in a strided output row"
        dead = mask is not None and mask.sum(dim=1).eq(0)
        live = ~dead if mask is not None else torch.ones(B, dtype=torch.bool)
        if live.any():
            assert (stats_c[live, :, 0].double() - mx_ref[live]).abs().max().item() <= 1e-4 * (1 + mx_ref[live].abs().max().item()), f"{what}: max"
            assert (stats_c[live, :, 1].double() - lse_ref[live]).abs().max().item() <= 1e-4 * (1 + lse_ref[live].abs().max().item()), f"{what}: log-sum"
        if mask is not None and dead.any():                           # every key masked: uniform weights, log-sum = log L
            assert (stats_c[dead, :, 1].double() - np.log(L)).abs().max().item() <= 1e-4 * (1 + np.log(L)), f"{what}: masked log-sum"
        diff = (after.double() - before.double()).view(B, L, 3, D)
        assert torch.equal(after.view(B, L, 3, D)[:, 1:, 0], before.view(B, L, 3, D)[:, 1:, 0]), f"{what}: q block of a row >= 1 touched"
        for i, blk in enumerate(("dq", "dk", "dv")):
            rows = slice(0, 1) if i == 0 else slice(None)
            scale_i = max(g3[:, :, i].abs().max().item(), floor)
            e = (diff[:, rows, i] - g3[:, rows, i]).abs().max().item() / scale_i
            assert e <= tol_g, f"{what}: {blk} (accumulated) {e:.2e}"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("H", [1, 12])
@pytest.mark.parametrize("Dh", [32, 64, 96, 128, 256])
@pytest.mark.parametrize("L", [1, 5, 255, 256, 257, 2353])
def test_attn_cls_parity(dev, dtype, L, Dh, H):
    """every thread of the score loop with or without a key, one row per row group or many (strided loops, the part[] reduction),
    Dh = 96 whose 12 column chunks leave 4 threads without a row group; masks: none, random, only key 0, every key"""
    _run_cls(dev, dtype, 2, L, H, Dh, seed=L * 131 + Dh * 7 + H)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("Dh", [64, 96])
def test_attn_cls_at_lds_limit(dev, dtype, Dh):
    """the longest sequence the backward's score + d-score buffers fit, forward and backward; one past it is refused up front"""
    L = cls_max_len(Dh, 2)
    assert L > 2353
    _run_cls(dev, dtype, 2, L, 2, Dh, seed=Dh)


@pytest.mark.parametrize("Dh", [32, 64, 96, 256])
def test_attn_cls_past_lds_limit_is_unsupported(dev, Dh):
    from meant_amd.ops import _p, _stream
    lib = _lib().lib
    B, H = 2, 2
    buf = torch.zeros(4096, device=dev)                             # never read: the check is on the host, before any launch
    stats = torch.zeros(B * H * 2, device=dev)
    for arrays, fn in ((1, "fwd"), (2, "bwd")):
        L = cls_max_len(Dh, arrays) + 1
        if fn == "fwd":
            rc = lib.meant_attn_cls_fwd(_p(buf), _p(buf), H * Dh, _p(stats), None, B, L, H, Dh, 0.1, 0, _stream())
        else:
            rc = lib.meant_attn_cls_bwd(_p(buf), _p(buf), H * Dh, _p(buf), H * Dh, _p(stats), None, _p(buf), B, L, H, Dh, 0.1, 0, _stream())
        assert rc == ERR_UNSUPPORTED, f"attn_cls_{fn} L={L} Dh={Dh}: rc {rc}"
    rc = lib.meant_attn_cls_fwd(_p(buf), _p(buf), H * 100, _p(stats), None, B, 5, H, 100, 0.1, 0, _stream())
    assert rc == ERR_UNSUPPORTED                                    # Dh % 8 != 0


def _shift_reference(x, f):
    from oracle import meant_oracle as O
    return O._TSPreTokenShift(f, lambda y: y)(x)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d", [24, 128, 192, 200, 512, 768, 1024])
@pytest.mark.parametrize("n", [1, 196])
@pytest.mark.parametrize("f", [1, 2, 12])
def test_token_shift_exact(dev, dtype, f, n, d):
    """meant_token_shift moves data only: forward == the oracle's PreTokenShift and transpose == its autograd backward, element
    for element, at widths whose third is not a multiple of 8 and with 1-2 remainder columns; <S x, y> == <x, S^T y>"""
    from meant_amd.ops import _dt, _p, _stream, check
    lib = _lib().lib
    rs = np.random.RandomState(f * 1000 + n * 10 + d)
    B, L = 2, 1 + f * n
    x = torch.from_numpy(rs.standard_normal((B, L, d)).astype("float32")).to(dtype)
    yb = torch.from_numpy(rs.standard_normal((B, L, d)).astype("float32")).to(dtype)
    xr = x.float().requires_grad_(True)
    ref = _shift_reference(xr, f)
    ref.backward(yb.float())
    x_d, yb_d = x.to(dev), yb.to(dev)
    sx, sty = torch.empty_like(x_d), torch.empty_like(x_d)
    check(lib.meant_token_shift(_p(x_d), _p(sx), B, f, n, d, 0, _dt(x_d), _stream()), "token_shift")
    check(lib.meant_token_shift(_p(yb_d), _p(sty), B, f, n, d, 1, _dt(x_d), _stream()), "token_shift^T")
    torch.cuda.synchronize()
    assert torch.equal(sx.cpu(), ref.detach().to(dtype)), f"shift f={f} n={n} d={d}"
    assert torch.equal(sty.cpu(), xr.grad.to(dtype)), f"shift^T f={f} n={n} d={d}"
    lhs = (sx.cpu().double() * yb.double()).sum().item()
    rhs = (x.double() * sty.cpu().double()).sum().item()
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0), (lhs, rhs)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_token_shift_module_any_width(dev, dtype):
    """TimeSformer(shift_tokens=True) at dims whose third is not a multiple of 8 runs (the constructor accepts them)"""
    import meant_amd as M
    for dim in (128, 512, 1024):
        m = M.TimeSformer(dim=dim, num_frames=3, num_classes=2, image_size=32, patch_size=16, channels=3, depth=1, heads=2,
                          dim_head=64, shift_tokens=True).to(dev)
        m.compute_dtype = dtype
        out = m(torch.randn(2, 3, 3, 32, 32, device=dev))
        out.float().sum().backward()
        assert torch.isfinite(out.float()).all() and torch.isfinite(m.cls_token.grad).all()


def _plans(f, hp, wp, H, Dh, b, dev):
    import meant_amd as M
    m = M.TimeSformer(dim=8, num_frames=f, num_classes=2, image_size=16, patch_size=16, depth=0, heads=H, dim_head=Dh)
    return m._plan(b, f, hp, wp, dev)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("half", ["time", "space"])
def test_group_scatter(dev, dtype, half):
    """meant_group_scatter on TimeSformer._plan's tables at (b, f, n) = (2, 12, 196), rows of 3 * 768: the group rows come home
    bit-exact, the cls row is the sum over the groups, every row is written"""
    from meant_amd.ops import _dt, _p, _stream, check
    lib = _lib().lib
    b, f, hp, wp, W = 2, 12, 14, 14, 3 * 768
    L = 1 + f * hp * wp
    t_time, t_space, p_time, p_space, _, _ = _plans(f, hp, wp, 12, 64, b, dev)
    index = (p_time if half == "time" else p_space)[0]
    G, S = index.shape
    rs = np.random.RandomState(G)
    ddst = torch.from_numpy(rs.standard_normal((b * G * S, W)).astype("float32")).to(dtype)
    rows = ((torch.arange(b) * L)[:, None] + index.cpu().long().view(-1)[None, :]).view(-1)
    ref = torch.zeros(b * L, W, dtype=torch.float64).index_add_(0, rows, ddst.double()).view(b, L, W)
    dsrc = torch.full((b, L, W), float("nan"), device=dev, dtype=dtype)
    dd = ddst.to(dev)
    check(lib.meant_group_scatter(_p(dd), _p(index), _p(dsrc), b, L, G, S, W, _dt(dd), _stream()), "group_scatter")
    torch.cuda.synchronize()
    got = dsrc.cpu()
    assert torch.equal(got[:, 1:], ref[:, 1:].to(dtype)), f"{half}: group rows"
    tol = (1e-6 if dtype == torch.float32 else 8e-3) * ref[:, 0].abs().max().item()
    e = (got[:, 0].double() - ref[:, 0]).abs().max().item()
    assert e <= tol, f"{half}: cls rows {e:.2e} > {tol:.1e}"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("dim", [128, 768])
def test_geglu_parity(dev, dtype, dim):
    """ops.geglu at the feed-forward's width 2 * 4 * dim and a prime row count, forward and backward against float64"""
    from meant_amd import ops
    rs = np.random.RandomState(dim)
    rows, w = 1237, 4 * dim
    h = torch.from_numpy(rs.standard_normal((rows, 2 * w)).astype("float32")).to(dtype)
    dy = torch.from_numpy(rs.standard_normal((rows, w)).astype("float32")).to(dtype)
    hr = h.double().requires_grad_(True)
    a, g = hr.chunk(2, dim=-1)
    yr = a * torch.nn.functional.gelu(g)
    yr.backward(dy.double())
    hd = h.to(dev).requires_grad_(True)
    y = ops.geglu(hd)
    y.backward(dy.to(dev))
    tol_o, tol_g = (2e-5, 2e-5) if dtype == torch.float32 else (8e-3, 1e-2)
    assert _rel(y, yr) <= tol_o, f"geglu fwd {_rel(y, yr):.2e}"
    assert _rel(hd.grad, hr.grad) <= tol_g, f"geglu bwd {_rel(hd.grad, hr.grad):.2e}"


# ------------------------------------------------------------------------------------------------------------------------------
# 2. ops.divided_attention against the oracle's _TSAttention core
# ------------------------------------------------------------------------------------------------------------------------------
def _oracle_core(H, Dh):
    """the oracle's _TSAttention with its projections taken out: input = the packed q|k|v buffer, output = the heads' outputs"""
    from oracle import meant_oracle as O
    core = O._TSAttention(8, Dh, H)
    core.to_qkv, core.to_out = torch.nn.Identity(), torch.nn.Identity()
    return core.double()


def _frame_masks(b, f, rs):
    rand = torch.from_numpy(rs.rand(b, f) > 0.5)
    first = torch.ones(b, f, dtype=torch.bool)
    first[:, 0] = False
    one = torch.zeros(b, f, dtype=torch.bool)
    one[0, f // 2] = True
    one[-1, 0] = True
    return {"none": None, "random": rand, "frame0": first, "one_live": one}


DIVIDED_SHAPES = [(2, 12, 14, 14, 12, 64), (2, 5, 7, 9, 4, 128), (2, 4, 6, 6, 4, 32), (2, 8, 6, 10, 8, 96)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("half", ["time", "space"])
@pytest.mark.parametrize("shape", DIVIDED_SHAPES, ids=["design", "7x9_d128", "d32", "6x10_d96"])
def test_divided_attention_parity(dev, dtype, half, shape):
    """one half of the divided pair: regroup + rotary with the cls key slot, flash core, cls query over all tokens; forward and
    dqkv against float64, frame masks none / random / frame 0 / one live frame, and the kernels each half must reach"""
    from oracle import meant_oracle as O
    from meant_amd import ops
    L_ = _lib()
    b, f, hp, wp, H, Dh = shape
    n, D = hp * wp, H * Dh
    L = 1 + f * n
    scale = Dh ** -0.5
    t_time, t_space, p_time, p_space, _, _ = _plans(f, hp, wp, H, Dh, b, dev)
    plan, tables = (p_time, t_time) if half == "time" else (p_space, t_space)
    frame_rot, image_rot = O.TimeSformer(dim=8, num_frames=f, num_classes=2, depth=0, heads=H, dim_head=Dh).rotary_tables(f, hp, wp)
    rot = tuple(r.double() for r in (frame_rot if half == "time" else image_rot))
    core = _oracle_core(H, Dh)
    rs = np.random.RandomState(sum(shape) + len(half))
    qkv = torch.from_numpy(rs.standard_normal((b, L, 3 * D)).astype("float32")).to(dtype)
    dout = torch.from_numpy(rs.standard_normal((b, L, D)).astype("float32")).to(dtype)
    tol = TOL[dtype]
    tol_o = tol["out"] * (1 if dtype == torch.float32 else 2)
    for name, fm in _frame_masks(b, f, rs).items():
        what = f"{half}[{name}] {shape}"
        x = qkv.double().requires_grad_(True)
        frame_mask = cls_mask = None
        group_mask = cls_mask_d = None
        if fm is not None:
            one = torch.ones(b, 1, dtype=torch.bool)
            frame_mask = torch.cat((one, fm), dim=1)
            cls_mask = torch.cat((one, fm.repeat_interleave(n, dim=1)), dim=1)
            if half == "time":
                group_mask = frame_mask.float().repeat_interleave(n, dim=0).to(dev)
            cls_mask_d = cls_mask.float().to(dev)
        ref = core(x, half, f, n, (rot[0], rot[1]), mask=frame_mask if half == "time" else None, cls_mask=cls_mask)
        ref.backward(dout.double())
        xd = qkv.to(dev).requires_grad_(True)
        L_.route_reset()
        out = ops.divided_attention(xd, plan, tables, H, scale, group_mask, cls_mask_d)
        torch.cuda.synchronize()
        assert L_.route_count("attn_cls") == 1, what
        if dtype == torch.bfloat16:
            tiled = {64: "attn_fwd", 96: "attn_fwd_d96", 128: "attn_fwd_d128"}
            if Dh in tiled:
                if half == "space":
                    assert L_.route_count(tiled[Dh]) == 1 and L_.route_count("attn_short") == 0, f"{what}: space half off the tiled kernel"
                else:
                    assert L_.route_count("attn_short") == 1 and L_.route_count(tiled[Dh]) == 0, f"{what}: time half off attn_short"
            else:
                assert L_.route_count("attn_generic") == 1, f"{what}: Dh={Dh} should take the fp32 detour"
        out.backward(dout.to(dev))
        assert_close(out, ref, tol_o, f"{what}: out")
        g, gr = xd.grad.view(b, L, 3, D), x.grad.view(b, L, 3, D)
        for i, blk in enumerate(("dq", "dk", "dv")):
            assert_grad_close(g[:, :, i], gr[:, :, i], tol["gelem"], f"{what}: {blk}")


# ------------------------------------------------------------------------------------------------------------------------------
# 3. meant_amd.TimeSformer against oracle.TimeSformer in float64
# ------------------------------------------------------------------------------------------------------------------------------
MODEL_CASES = {
    "design": dict(kw=dict(dim=768, heads=12, dim_head=64, num_frames=12, image_size=224, depth=1), hw=(224, 224)),
    "design_mask": dict(kw=dict(dim=768, heads=12, dim_head=64, num_frames=12, image_size=224, depth=1), hw=(224, 224), mask=True),
    "design_posemb": dict(kw=dict(dim=768, heads=12, dim_head=64, num_frames=12, image_size=224, depth=1, rotary_emb=False), hw=(224, 224)),
    "mid": dict(kw=dict(dim=320, heads=4, dim_head=96, num_frames=5, image_size=112, depth=2), hw=(112, 80)),
    "mid_mask": dict(kw=dict(dim=320, heads=4, dim_head=96, num_frames=5, image_size=112, depth=2), hw=(112, 80), mask=True),
    "mid_shift": dict(kw=dict(dim=320, heads=4, dim_head=96, num_frames=5, image_size=112, depth=2, shift_tokens=True), hw=(112, 80)),
    "mid_posemb": dict(kw=dict(dim=320, heads=4, dim_head=96, num_frames=5, image_size=112, depth=2, rotary_emb=False), hw=(112, 80)),
}
_ORACLE_RUNS = {}


def _model_case(name):
    cfg = MODEL_CASES[name]
    f = cfg["kw"]["num_frames"]
    rs = np.random.RandomState(len(name) * 17 + f)
    b, (hh, ww) = 2, cfg["hw"]
    video = torch.from_numpy(rs.standard_normal((b, f, 3, hh, ww)).astype("float32"))
    mask = None
    if cfg.get("mask"):
        mask = torch.from_numpy(rs.rand(b, f) > 0.4)
        mask[0, 0], mask[1, :] = False, False
        mask[1, 2] = True                                                  # video 1: a single live frame
    target = torch.from_numpy(rs.randint(0, 3, b).astype("int64"))
    return video, mask, target


def _loss(x, logits, target):
    return torch.nn.functional.cross_entropy(logits, target) + 0.01 * x.pow(2).mean()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_timesformer_vs_oracle(dev, dtype, case):
    import meant_amd as M
    from oracle import meant_oracle as O
    cfg = MODEL_CASES[case]
    kw = dict(cfg["kw"], num_classes=3, patch_size=16, channels=3)
    video, mask, target = _model_case(case)
    ref, hip = pair(O.TimeSformer(**kw), M.TimeSformer(**kw), 4321, dev)
    ref = ref.double()
    if case not in _ORACLE_RUNS:                                            # one float64 run per case, shared by both tiers
        x_r = ref.meant_forward(video.double(), mask=mask)
        logits_r = ref.to_out(x_r[:, 0])
        loss_r = _loss(x_r, logits_r, target)
        loss_r.backward()
        _ORACLE_RUNS[case] = (x_r.detach(), logits_r.detach(), loss_r.item(), {k: p.grad.clone() for k, p in ref.named_parameters()})
    x_r, logits_r, loss_r, grads_r = _ORACLE_RUNS[case]
    for k, p in ref.named_parameters():
        p.grad = grads_r[k]
    hip.compute_dtype = dtype
    x = hip.meant_forward(video.to(dev), mask=mask.to(dev) if mask is not None else None)
    logits = hip.to_out(x[:, 0])
    loss = _loss(x.float(), logits.float(), target.to(dev))
    loss.backward()
    tol = 2e-4 if dtype == torch.float32 else 4e-2                          # the golden test's gates, relative to the largest value
    assert _rel(x, x_r) <= tol, f"{case}: tokens {_rel(x, x_r):.2e}"
    assert maxerr_scaled(logits, logits_r) <= tol, f"{case}: logits"
    assert abs(loss.item() - loss_r) <= (1e-4 if dtype == torch.float32 else 2e-2) * abs(loss_r), f"{case}: loss {loss.item()} vs {loss_r}"
    compare_param_grads(ref, hip, dtype, case)


def maxerr_scaled(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / max(1.0, b.abs().max().item())
