"""bf16 Linear at reduction lengths that are not a multiple of 64: the K-tail forms of the two one-tile NT kernels (route counters
"nt128k" / "nt256k"), the fused q|k|v projection on them, and the K % 8 != 0 path of ops.linear (operands padded to ceil8(K) by
meant_pad_copy2d).  Conventions of tests/test_gpu_gemm_stream.py: the reference is fp32 on the CPU on the bf16-rounded inputs, the
forward tolerance 3e-2 * max(1, |y|max), gradients assert_grad_close(..., 2e-2), options pinned by a fixture, and every case
asserts its ROUTE (on the code before these kernels the same shapes count under "gemm_f32").

Two route facts the assertions below spell out instead of a bare `gemm_f32 == 0`:
  * the weight gradient of M = 130 rows hands its 130 % 64 = 2 trailing rows to the exact kernel (route "tn_tail", which counts one
    "gemm_f32" launch) at every K, K % 64 == 0 included -- so after a backward the assertion is gemm_f32 == tn_tail (nothing but
    that row tail ran on the exact engine), and gemm_f32 == 0 after the forward;
  * the input gradient's reduction length is N.  With the forward on the 256 x 256 K-tail kernel N is a multiple of 256, so its dX
    is an ordinary K % 64 == 0 launch; the 256 x 256 K-tail kernel as a dX kernel is covered by the transposed shape."""
import math

import numpy as np
import pytest
import torch

from tests.util import TOL, assert_close, assert_grad_close, compare_param_grads, pair, t

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NT_ROUTES = ("nt128", "nt256", "nt256s", "nt_split", "nt_overlap", "nt128k", "nt256k", "gemm_f32", "tn128", "tn256", "tn_tail")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture()
def L():
    from meant_amd import _lib
    saved = {k: _lib.get_option(k) for k in ("nt_dynamic", "nt_grid_cap", "nt_stream", "deterministic", "nt_ragged")}
    for k, v in (("nt_dynamic", 1), ("nt_grid_cap", 0), ("nt_stream", 1), ("deterministic", 0), ("nt_ragged", 1)):
        _lib.set_option(k, v)                        # the route assertions are about the default dispatch, whatever the environment says
    _lib.route_reset()
    yield _lib
    for k, v in saved.items():
        _lib.set_option(k, v)


def _rand(rs, *shape, scale=1.0):
    return torch.from_numpy((rs.standard_normal(shape) * scale).astype("float32"))


def _routes(L):
    return {r: L.route_count(r) for r in NT_ROUTES}


def _linear_case(L, dev, M_, N, K, epi):
    """ops.linear forward + backward against fp32 on the CPU; returns (routes after the forward, routes after the backward)"""
    from meant_amd import ops
    from meant_amd._lib import EPI_NONE, EPI_GELU, EPI_SIGMOID
    rs = np.random.RandomState(M_ % 1000 + N + K)
    x, w, b = _rand(rs, M_, K), _rand(rs, N, K, scale=1 / math.sqrt(K)), _rand(rs, N, scale=0.1)
    res, dy = _rand(rs, M_, N), _rand(rs, M_, N)
    xq, wq, resq, dyq = [v.to(BF).float() for v in (x, w, res, dy)]
    xr, wr, br, rr = xq.clone().requires_grad_(), wq.clone().requires_grad_(), b.clone().requires_grad_(), resq.clone().requires_grad_()
    yr = torch.nn.functional.linear(xr, wr, br)
    if epi == "gelu":
        yr = torch.nn.functional.gelu(yr)
    elif epi == "sigmoid":
        yr = torch.sigmoid(yr)
    elif epi == "residual":
        yr = yr + rr
    yr.backward(dyq)
    xh = x.to(dev).to(BF).requires_grad_()
    wh, bh = wq.to(dev).requires_grad_(), b.to(dev).requires_grad_()
    rh = res.to(dev).to(BF).requires_grad_()
    e = {"none": EPI_NONE, "gelu": EPI_GELU, "sigmoid": EPI_SIGMOID, "residual": EPI_NONE}[epi]
    L.route_reset()
    yh = ops.linear(xh, wh, bh, rh if epi == "residual" else None, e)
    fwd = _routes(L)
    yh.backward(dy.to(dev).to(BF))
    torch.cuda.synchronize()
    bwd = _routes(L)
    assert yh.shape == (M_, N) and xh.grad.shape == (M_, K) and wh.grad.shape == (N, K)
    assert_close(yh, yr, 3e-2 * max(1.0, yr.abs().max().item()), "y")
    assert_grad_close(xh.grad, xr.grad, 2e-2, "dx")
    assert_grad_close(wh.grad, wr.grad, 2e-2, "dw")
    assert_grad_close(bh.grad, br.grad, 2e-2, "db")
    if epi == "residual":
        assert_grad_close(rh.grad, rr.grad, 2e-2, "dres")
    return fwd, bwd


# K = 8: the tail alone (seven zero chunks per row); 72 / 120: one full step + one / seven chunks; 200 = 3 * 64 + 8; 520 = 8 * 64 + 8
@pytest.mark.parametrize("K,epi", [(8, "none"), (72, "residual"), (120, "gelu"), (200, "none"), (200, "gelu"), (200, "sigmoid"),
                                   (200, "residual"), (520, "sigmoid")])
def test_tail_geometry_on_the_128_kernel(L, dev, K, epi):
    """M = 130: two row tiles, the second with 126 clamped rows; N = 136: two column tiles and, as dX's reduction length
    (136 = 2 * 64 + 8), a tail of its own"""
    fwd, bwd = _linear_case(L, dev, 130, 136, K, epi)
    assert fwd["nt128k"] == 1 and fwd["gemm_f32"] == 0 and fwd["nt128"] == 0 and fwd["nt256k"] == 0, fwd
    assert bwd["nt128k"] == 2 and bwd["nt128"] == 0, bwd                       # ... and so did dX
    assert bwd["tn128"] == 1 and bwd["tn_tail"] == 1 and bwd["gemm_f32"] == bwd["tn_tail"], bwd      # dW; see the module docstring


def test_tail_with_the_scalar_epilogue(L, dev):
    """N = 100: output rows are not 16-byte aligned, the element-wise epilogue stores them; dX (reduction length 100) and dW stay
    on the exact kernel"""
    fwd, _ = _linear_case(L, dev, 130, 100, 200, "gelu")
    assert fwd["nt128k"] == 1 and fwd["gemm_f32"] == 0, fwd


@pytest.mark.parametrize("K,epi", [(328, "residual"), (72, "gelu")])
def test_tail_on_the_256_kernel(L, dev, K, epi):
    """32 x 4 = 128 tiles of 256 x 256: at least half the CUs, so the launcher takes the 256 x 256 kernel.  dX reduces over
    N = 1024 (no tail) into K columns, not a multiple of 256: the 128 x 128 kernel, as before"""
    fwd, bwd = _linear_case(L, dev, 8192, 1024, K, epi)
    assert fwd["nt256k"] == 1 and fwd["nt128k"] == 0 and fwd["gemm_f32"] == 0 and fwd["nt256"] == 0 and fwd["nt256s"] == 0, fwd
    assert bwd["nt128k"] + bwd["nt256k"] == 1 and bwd["nt128"] == 1 and bwd["gemm_f32"] == 0, bwd
    assert bwd["tn128"] == 1 and bwd["tn_tail"] == 0, bwd


def test_tail_on_the_256_kernel_as_input_gradient(L, dev):
    """the transposed shape: dX[8192, 1024] reduces over N = 328 on the 256 x 256 K-tail kernel"""
    fwd, bwd = _linear_case(L, dev, 8192, 328, 1024, "none")
    assert fwd["nt128"] == 1 and fwd["nt128k"] == 0 and fwd["nt256k"] == 0, fwd
    assert bwd["nt256k"] == 1 and bwd["nt128k"] == 0 and bwd["gemm_f32"] == 0, bwd


def _in_nan_pool(v, dev, lead=64, trail=256):
    """a bf16 device copy of the contiguous tensor v that lies inside a larger allocation filled with NaN (lead elements in front:
    16-byte alignment is kept; trail elements behind)"""
    pool = torch.full((lead + v.numel() + trail,), float("nan"), device=dev, dtype=BF)
    view = pool[lead:lead + v.numel()].view(v.shape)
    view.copy_(v.to(dev).to(BF))
    return pool, view


@pytest.mark.parametrize("K", [72, 200])
def test_nothing_beyond_k_is_read(L, dev, K):
    """raw C ABI, ldx = K + 8, columns K .. K+7 of every row of x NaN: a chunk fetched from there would make the row of y NaN
    (NaN * 0 = NaN, whatever the weight side holds)"""
    M_, N = 130, 136
    rs = np.random.RandomState(K)
    x, w, b = _rand(rs, M_, K), _rand(rs, N, K, scale=1 / math.sqrt(K)), _rand(rs, N, scale=0.1)
    xbuf = torch.full((M_, K + 8), float("nan"), dtype=torch.float32)
    xbuf[:, :K] = x
    xh, wh, bh = xbuf.to(dev).to(BF), w.to(dev).to(BF), b.to(dev)
    assert torch.isnan(xh[:, K:]).all()
    y = torch.empty((M_, N), device=dev, dtype=BF)
    L.route_reset()
    L.check(L.lib.meant_linear_fwd(xh.data_ptr(), K + 8, wh.data_ptr(), bh.data_ptr(), None, 0, y.data_ptr(), N, None, M_, N, K, L.EPI_NONE,
                                   L.BF16, torch.cuda.current_stream().cuda_stream), "linear_fwd")
    torch.cuda.synchronize()
    assert L.route_count("nt128k") == 1 and L.route_count("gemm_f32") == 0
    assert torch.isfinite(y.float()).all()
    ref = torch.nn.functional.linear(x.to(BF).float(), w.to(BF).float(), b)
    assert_close(y, ref, 3e-2 * max(1.0, ref.abs().max().item()), "y")


@pytest.mark.parametrize("K", [72, 200])
def test_nothing_beyond_k_is_read_on_the_weight_side(L, dev, K):
    """the weight is [N, K] contiguous (the ABI fixes ldb = K), so what lies behind column K of its LAST row is whatever follows the
    matrix in memory: here NaN, w being a view into a NaN-filled allocation.  x is contiguous and finite, so its tail chunks are
    zeros in LDS whether redirected or not ... and 0 * NaN = NaN: a weight chunk fetched from behind the matrix would make column
    N - 1 of y NaN.  The same through meant_linear_bwd_dx, whose B operand is the transposed weight [K', N'] with reduction N'."""
    M_, N = 130, 136
    rs = np.random.RandomState(K + 1)
    x, w, b = _rand(rs, M_, K), _rand(rs, N, K, scale=1 / math.sqrt(K)), _rand(rs, N, scale=0.1)
    (xpool, xh), (wpool, wh) = _in_nan_pool(x, dev), _in_nan_pool(w, dev)
    bh = b.to(dev)
    assert xh.data_ptr() % 16 == 0 and wh.data_ptr() % 16 == 0 and torch.isnan(wpool[64 + N * K:]).all()
    st = torch.cuda.current_stream().cuda_stream
    y = torch.empty((M_, N), device=dev, dtype=BF)
    L.route_reset()
    L.check(L.lib.meant_linear_fwd(xh.data_ptr(), K, wh.data_ptr(), bh.data_ptr(), None, 0, y.data_ptr(), N, None, M_, N, K, L.EPI_NONE, L.BF16, st),
            "linear_fwd")
    # input gradient of a Linear with K_out = N columns and reduction length K: dy = x [M, K], wT = w [N, K] -> dx [M, N] = x w^T
    dx = torch.empty((M_, N), device=dev, dtype=BF)
    L.check(L.lib.meant_linear_bwd_dx(xh.data_ptr(), K, wh.data_ptr(), dx.data_ptr(), N, M_, K, N, L.BF16, st), "linear_bwd_dx")
    torch.cuda.synchronize()
    assert L.route_count("nt128k") == 2 and L.route_count("gemm_f32") == 0
    ref = torch.nn.functional.linear(x.to(BF).float(), w.to(BF).float())
    for got, want, what in ((y, ref + b, "y"), (dx, ref, "dx")):
        assert torch.isfinite(got.float()).all(), what
        assert_close(got, want, 3e-2 * max(1.0, want.abs().max().item()), what)


@pytest.mark.parametrize("M_,N,K,route", [(130, 136, 64, "nt128"), (130, 136, 768, "nt128"), (8192, 1024, 64, "nt256"),
                                          (8192, 1024, 768, "nt256s")])
def test_multiples_of_64_take_the_routes_they_took(L, dev, M_, N, K, route):
    fwd, bwd = _linear_case(L, dev, M_, N, K, "residual")
    assert fwd["nt128k"] == 0 and fwd["nt256k"] == 0 and fwd[route] == 1 and fwd["gemm_f32"] == 0, fwd
    assert sum(fwd[r] for r in ("nt128", "nt256", "nt256s")) == 1, fwd
    assert bwd["nt256k"] == 0 and bwd["nt128k"] == (1 if N % 64 else 0), bwd


def test_fused_projection_keeps_its_rotary_epilogue(L, dev):
    """xPosAttention(3 heads, dim 216): head dim 72 (padded to 128 by ops.qkv_attention), 48 xPos lanes, S = 80, B = 2, against the
    oracle's module.  The q|k|v projection reduces over 216 = 3 * 64 + 24: one launch on the K-tail kernel with the rotation in its
    epilogue, none on the exact engine.  Tolerances: those of the module comparisons of tests/test_gpu_attn_wide.py (the output has
    passed four bf16 roundings: q|k|v, the attention output, multi_mad's result and the input itself)"""
    import meant_amd as M
    from oracle import meant_oracle as O
    H, d, G, S = 3, 216, 2, 80
    ref, hip = pair(O.xPosAttention(H, d, O.RotaryTable(48, "lang", use_xpos=True)), M.xPosAttention(H, d, M.RotaryEmbedding(dim=48, use_xpos=True)),
                    4321, dev)
    rs = np.random.RandomState(d + S)
    x, dy = _rand(rs, G, S, d), _rand(rs, G, S, d)
    mask = torch.ones(G, S)
    mask[0, S // 3:] = 0
    xr = x.to(BF).float().requires_grad_()
    yr = ref(xr, mask)
    yr.backward(dy.to(BF).float())
    xh = x.to(dev).to(BF).requires_grad_()
    L.route_reset()
    core = hip.core(xh, mask.to(dev))
    after_core = _routes(L)
    yh = hip.multi_mad(core)                                 # == hip(xh, mask): xPosAttention.forward is multi_mad(core(...))
    yh.backward(dy.to(dev).to(BF))
    torch.cuda.synchronize()
    assert after_core["nt128k"] == 1 and after_core["gemm_f32"] == 0 and after_core["nt128"] == 0, after_core
    tol = TOL[BF]
    assert_close(yh, yr, tol["out"] * 4, "y")
    assert_grad_close(xh.grad, xr.grad, tol["gelem"], "dx")
    compare_param_grads(ref, hip, BF, "xpos_3x72")


@pytest.mark.parametrize("K", [588, 1540])
def test_reduction_lengths_that_are_no_multiple_of_8(L, dev, K):
    """588 = 14 * 14 * 3 (a ViT-L/14 patch of 3 channels), 1540: both operands padded to ceil8(K), forward and dX (reduction length
    136) on the K-tail kernel, dW through an [N, ceil8(K)] accumulator on the MFMA kernel"""
    fwd, bwd = _linear_case(L, dev, 130, 136, K, "none")
    assert fwd["nt128k"] == 1 and fwd["gemm_f32"] == 0, fwd
    assert bwd["nt128k"] == 2 and bwd["tn128"] == 1 and bwd["gemm_f32"] == bwd["tn_tail"] == 1, bwd      # see the module docstring


def test_pad_copy2d(dev):
    """the copy kernel on its own, exact: zero fill beyond cols_src, cut at cols_dst, odd source strides, aligned and unaligned
    destination rows (both store paths), all four dtype pairs"""
    from meant_amd import _lib
    rs = np.random.RandomState(1)
    code = {BF: _lib.BF16, torch.float32: _lib.F32}
    for rows, ld_src, cols_src, cols_dst in ((37, 21, 13, 16), (5, 592, 592, 588), (130, 589, 588, 592), (9, 588, 588, 592), (6, 30, 26, 32), (3, 7, 7, 7)):
        src = _rand(rs, rows, ld_src)
        for ds, dd in ((torch.float32, BF), (BF, BF), (torch.float32, torch.float32), (BF, torch.float32)):
            s = src.to(dev).to(ds)
            for ld_dst in (cols_dst + 3, (cols_dst + 7) & ~7):          # element-wise stores / rows that start on 16 bytes: vector stores
                out = torch.full((rows, ld_dst), 7.0, device=dev, dtype=dd)
                _lib.check(_lib.lib.meant_pad_copy2d(s.data_ptr(), ld_src, cols_src, code[ds], out.data_ptr(), ld_dst, cols_dst, code[dd], rows,
                                                     torch.cuda.current_stream().cuda_stream), "pad_copy2d")
                want = torch.full((rows, ld_dst), 7.0, dtype=torch.float32)
                n = min(cols_src, cols_dst)
                want[:, :cols_dst] = 0
                want[:, :n] = s.cpu().float()[:, :n].to(dd).float()
                assert torch.equal(out.cpu().float(), want), (rows, ld_src, cols_src, cols_dst, ld_dst, ds, dd)


@pytest.mark.parametrize("channels,patch_dim", [(4, 784), (3, 588)])
def test_vision_model_with_patch_14(L, dev, channels, patch_dim):
    """meant_vision at patch_res = 14 on 28 x 28 images (4 patches), image_dim 64, against the oracle at the bf16 tolerances of
    tests/test_gpu_models.py; the patch embedding (K = 784 = 12 * 64 + 16, or 588 -> 592 = 9 * 64 + 16) runs on a K-tail kernel"""
    import meant_amd
    from oracle import meant_oracle as O
    args, kw = (64, 4, 28, 28, 14, 3, 2), dict(num_heads=2, num_encoders=1, channels=channels)
    ref, hip = pair(O.meant_vision(*args, **kw), meant_amd.meant_vision(*args, **kw), 1234, dev)
    assert hip.patch_dim == patch_dim
    r = np.random.RandomState(14)
    img = t(r.standard_normal((2, 3, channels, 28, 28)).astype("float32"))
    tgt = torch.tensor([1, 0])
    out_r = ref(img)
    torch.nn.functional.cross_entropy(out_r, tgt).backward()
    seen = {}
    lin = hip.patchEmbed[1]
    h1 = lin.register_forward_pre_hook(lambda m, i: seen.update(before=_routes(L)))
    h2 = lin.register_forward_hook(lambda m, i, o: seen.update(after=_routes(L)))
    hip.compute_dtype = BF
    L.route_reset()
    out = hip(img.to(dev))
    h1.remove(); h2.remove()
    torch.nn.functional.cross_entropy(out, tgt.to(dev)).backward()
    torch.cuda.synchronize()
    assert seen["after"]["nt128k"] - seen["before"]["nt128k"] == 1 and seen["after"]["gemm_f32"] == seen["before"]["gemm_f32"], seen
    assert_close(out, out_r, TOL[BF]["out"], "out")
    compare_param_grads(ref, hip, BF, f"vision_p14_c{channels}")
