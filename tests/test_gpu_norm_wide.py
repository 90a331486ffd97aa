"""RMSNorm / LayerNorm at the widths one wave per row does not take (d > 2048, or d % 8 != 0): the one-row-per-workgroup form
(TEAM = 256) of the unpacked kernels of csrc/norm.hip (rmsnorm_*_wide_kernel, layernorm_*_wide_kernel) against the CPU oracle /
eager fp32 PyTorch, both tiers."""
import numpy as np
import pytest
import torch

from tests.util import DTYPES, IDS, TOL, t, assert_close, assert_grad_close

pytestmark = pytest.mark.gpu

WIDE_SHAPES = [(37, 2304), (5, 4096), (64, 2056), (3, 8200), (9, 12288), (17, 100), (130, 1000), (4, 3), (2, 2049)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _out_tol(dtype):
    return TOL[dtype]["out"] * (1 if dtype == torch.float32 else 4)


def _inputs(rows, d, seed):
    rs = np.random.RandomState(seed)
    x = t(rs.standard_normal((rows, d)).astype("float32"))
    dy = t(rs.standard_normal((rows, d)).astype("float32"))
    return x, dy, rs


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows,d", WIDE_SHAPES)
def test_rmsnorm_any_width(dev, dtype, rows, d):
    import meant_amd as M
    from oracle import meant_oracle as O
    x, dy, rs = _inputs(rows, d, rows * 7 + d)
    g = t((1 + 0.1 * rs.standard_normal(d)).astype("float32"))
    ref, hip = O.RMSNorm(d), M.RMSNorm(d).to(dev)
    with torch.no_grad():
        ref.scale.copy_(g)
        hip.scale.copy_(g)
    # the reference sees the inputs the device sees (rounded to the tier's storage type)
    xr = x.to(dtype).float().clone().requires_grad_()
    yr = ref(xr)
    yr.backward(dy.to(dtype).float())
    xh = x.to(dev).to(dtype).requires_grad_()
    yh = hip(xh)
    yh.backward(dy.to(dev).to(dtype))
    assert yh.dtype == dtype
    assert_close(yh, yr, _out_tol(dtype), "y")
    assert_grad_close(xh.grad, xr.grad, TOL[dtype]["gelem"], "dx")
    assert_grad_close(hip.scale.grad, ref.scale.grad, TOL[dtype]["gelem"], "dscale")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d,p,rows", [(2304, 0.5, 19), (100, 0.3, 23), (12288, 0.75, 3)])
def test_rmsnorm_partial_and_bias_forms_wide(dev, dtype, d, p, rows):
    import meant_amd as M
    from oracle import meant_oracle as O
    x, dy, rs = _inputs(rows, d, d + rows)
    g = t((1 + 0.1 * rs.standard_normal(d)).astype("float32"))
    off = t((0.1 * rs.standard_normal(d)).astype("float32"))
    ref, hip = O.RMSNorm(d, p=p, bias=True), M.RMSNorm(d, p=p, bias=True).to(dev)
    with torch.no_grad():
        for m in (ref, hip):
            m.scale.copy_(g)
            m.offset.copy_(off)
    xr = x.to(dtype).float().clone().requires_grad_()
    yr = ref(xr)
    yr.backward(dy.to(dtype).float())
    xh = x.to(dev).to(dtype).requires_grad_()
    yh = hip(xh)
    yh.backward(dy.to(dev).to(dtype))
    tol = TOL[dtype]
    assert_close(yh, yr, _out_tol(dtype), "y")
    assert_grad_close(xh.grad, xr.grad, tol["gelem"], "dx")
    assert_grad_close(hip.scale.grad, ref.scale.grad, tol["gelem"], "dscale")
    assert_grad_close(hip.offset.grad, ref.offset.grad, tol["gelem"], "doffset")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows,d", [(21, 2304), (6, 4100), (33, 100), (3, 12300)])
def test_layernorm_any_width(dev, dtype, rows, d):
    import meant_amd as M
    x, dy, rs = _inputs(rows, d, 3 * d + rows)
    x = x * 2 + 0.5                                        # a mean that the statistics have to take out
    w = t((1 + 0.1 * rs.standard_normal(d)).astype("float32"))
    b = t((0.1 * rs.standard_normal(d)).astype("float32"))
    ref, hip = torch.nn.LayerNorm(d), M.LayerNorm(d).to(dev)
    with torch.no_grad():
        for m in (ref, hip):
            m.weight.copy_(w)
            m.bias.copy_(b)
    xr = x.to(dtype).float().clone().requires_grad_()
    yr = ref(xr)
    yr.backward(dy.to(dtype).float())
    xh = x.to(dev).to(dtype).requires_grad_()
    yh = hip(xh)
    yh.backward(dy.to(dev).to(dtype))
    tol = TOL[dtype]
    assert yh.dtype == dtype
    assert_close(yh, yr, _out_tol(dtype), "y")
    assert_grad_close(xh.grad, xr.grad, tol["gelem"], "dx")
    assert_grad_close(hip.weight.grad, ref.weight.grad, tol["gelem"], "dweight")
    assert_grad_close(hip.bias.grad, ref.bias.grad, tol["gelem"], "dbias")


def _rms(x, g, eps):
    return g * x / (x.norm(dim=-1, keepdim=True) / x.shape[-1] ** 0.5 + eps)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows,d", [(40, 2560), (24, 1000), (7, 2051)])
def test_rmsnorm_fork_with_the_residual_gradient_wide(dev, dtype, rows, d):
    """ops.rmsnorm_fork: (RMSNorm(x), x), the residual branch's gradient added inside the backward kernel (dres)"""
    from meant_amd import ops
    gen = torch.Generator().manual_seed(rows + d)
    x = torch.randn(rows, d, generator=gen)
    g = 1 + 0.1 * torch.randn(d, generator=gen)
    w1, w2 = torch.randn(rows, d, generator=gen), torch.randn(rows, d, generator=gen)
    eps = 1e-8
    xr, gr = x.to(dtype).float().clone().requires_grad_(), g.clone().requires_grad_()
    y_ref = _rms(xr, gr, eps)
    ((y_ref * w1).sum() + (xr * xr * w2).sum()).backward()
    xd, gd = x.to(dev).to(dtype).requires_grad_(), g.to(dev).requires_grad_()
    y, res = ops.rmsnorm_fork(xd, gd, eps, any_width=True)
    ((y.float() * w1.to(dev)).sum() + (res.float() * res.float() * w2.to(dev)).sum()).backward()
    tol = TOL[dtype]
    assert_close(y, y_ref, _out_tol(dtype), "y")
    assert_grad_close(xd.grad, xr.grad, tol["gelem"], "dx")
    assert_grad_close(gd.grad, gr.grad, tol["gelem"], "dgain")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", [2560, 1000])
@pytest.mark.parametrize("p", [0.0, 0.5], ids=["eval", "dropout"])
def test_linear_gelu_rmsnorm_wide(dev, dtype, N, p):
    """ops.linear_gelu_rmsnorm: RMSNorm(gelu(x W^T + b)) with the GELU derivative inside the norm's backward (gelu_pre), and the
    train-mode dropout fused into the norm; mask read back from the plain kernel at the same shape"""
    from meant_amd import ops
    rows, K, seed, eps = 48, 256, 98765, 1e-8
    gen = torch.Generator().manual_seed(N)
    x = torch.randn(rows, K, generator=gen)
    W = torch.randn(N, K, generator=gen) / K ** 0.5
    b = torch.randn(N, generator=gen) * 0.1
    g = 1 + 0.1 * torch.randn(N, generator=gen)
    wy = torch.randn(rows, N, generator=gen)
    mask = _mask_of(rows, N, p, seed, dev).cpu() if p > 0 else torch.ones(rows, N)
    xr = x.to(dtype).float().clone().requires_grad_()
    Wr = (W.to(dtype).float() if dtype == torch.bfloat16 else W).clone().requires_grad_()
    br, gr = b.clone().requires_grad_(), g.clone().requires_grad_()
    y_ref = _rms(torch.nn.functional.gelu(xr @ Wr.t() + br), gr, eps) * mask
    (y_ref * wy).sum().backward()
    xd = x.to(dev).to(dtype).requires_grad_()
    Wd, bd, gd = (v.clone().to(dev).requires_grad_() for v in (W, b, g))
    y = ops.linear_gelu_rmsnorm(xd, Wd, bd, gd, eps, p, seed, any_width=True)
    (y.float() * wy.to(dev)).sum().backward()
    tol = TOL[dtype]
    assert_close(y, y_ref, _out_tol(dtype) * max(1.0, y_ref.abs().max().item()), "y")
    for name, a, r in (("x", xd, xr), ("W", Wd, Wr), ("b", bd, br), ("gain", gd, gr)):
        assert_grad_close(a.grad, r.grad, tol["gelem"], name)


def _mask_of(rows, d, p, seed, dev, dtype=torch.float32):
    """keep / (1 - p) factors of the norm kernels' dropout: RMSNorm(ones) = 1 / (1 + eps) wherever an element is kept"""
    from meant_amd import ops
    y = ops.rmsnorm(torch.ones(rows, d, device=dev, dtype=dtype), torch.ones(d, device=dev), 1e-8, p, seed, any_width=True)
    keep = (y != 0).float()
    return keep / (1.0 - p)


@pytest.mark.parametrize("rows,d,rows2,d2", [(8, 4096, 16, 2048), (16, 100, 2, 800), (6, 2049, 3, 4098)])
def test_dropout_mask_follows_the_flat_element_rule(dev, rows, d, rows2, d2):
    """element i = row * d + col is decided by the draw of i >> 3 alone: the same flat buffer viewed at another width gives the same
    mask, whether the other width runs on the packed / generic kernels (2048, 800) or on the wide ones (4098)"""
    p, seed = 0.5, 4242
    assert rows * d == rows2 * d2
    a = _mask_of(rows, d, p, seed, dev).reshape(-1)
    b = _mask_of(rows2, d2, p, seed, dev).reshape(-1)
    assert torch.equal(a, b)
    assert abs((a != 0).float().mean().item() - (1 - p)) < 0.03


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows,d", [(12, 4096), (16, 100), (3, 9000)])
def test_dropout_forward_and_backward_use_one_mask(dev, dtype, rows, d):
    """the backward regenerates the forward's mask: with RMSNorm of ones, dx is the masked gradient's projection, and the gain
    gradient is sum_rows(dy * mask) * rinv * x, zero exactly where every row dropped the column"""
    from meant_amd import ops
    p, seed, eps = 0.3, 777, 1e-8
    gen = torch.Generator().manual_seed(rows * d)
    x = torch.randn(rows, d, generator=gen)
    g = 1 + 0.1 * torch.randn(d, generator=gen)
    dy = torch.randn(rows, d, generator=gen)
    xd, gd = x.to(dev).to(dtype).requires_grad_(), g.to(dev).requires_grad_()
    y = ops.rmsnorm(xd, gd, eps, p, seed, any_width=True)
    y.backward(dy.to(dev).to(dtype))
    keep = (y != 0).float().cpu()
    mask = keep / (1 - p)
    xr, gr = x.to(dtype).float().clone().requires_grad_(), g.clone().requires_grad_()
    y_ref = _rms(xr, gr, eps) * mask
    y_ref.backward(dy.to(dtype).float())
    tol = TOL[dtype]
    assert_close(y, y_ref, _out_tol(dtype), "y")
    assert_grad_close(xd.grad, xr.grad, tol["gelem"], "dx")
    assert_grad_close(gd.grad, gr.grad, tol["gelem"], "dgain")


def test_zero_width_still_refused(dev):
    from meant_amd import lib, ops
    x = torch.ones(4, 8, device=dev)
    y = torch.empty_like(x)
    rinv = torch.empty(4, device=dev)
    sc = torch.ones(8, device=dev)
    st = torch.empty(4, 2, device=dev)
    p = ops._p
    assert lib.meant_rmsnorm_fwd(p(x), p(sc), p(y), p(rinv), 4, 0, 1e-8, 0.0, 0, ops._dt(x), ops._stream()) != 0
    assert lib.meant_rmsnorm_partial_fwd(p(x), p(sc), None, p(y), p(rinv), 4, 0, 1, 1e-8, ops._dt(x), ops._stream()) != 0
    assert lib.meant_layernorm_fwd(p(x), p(sc), p(sc), p(y), p(st), 4, 0, 1e-5, ops._dt(x), ops._stream()) != 0
    assert lib.meant_layernorm_fwd(p(x), p(sc), p(sc), p(y), p(st), 4, -8, 1e-5, ops._dt(x), ops._stream()) != 0
    ws = torch.empty(1 << 16, device=dev, dtype=torch.uint8)
    assert lib.meant_layernorm_bwd(p(x), p(x), p(sc), p(st), p(y), p(sc), p(sc), 4, 0, ops._dt(x), p(ws), ws.numel(), ops._stream()) != 0


def test_errors_are_loud_at_any_width(dev):
    """no CPU fallback and no silent dtype cast; the fused ops keep d % 8 == 0 unless the caller opts in (the norm modules do), and a
    bad d_part still raises through the C ABI"""
    import meant_amd as M
    from meant_amd import ops
    with pytest.raises(RuntimeError):
        ops.rmsnorm(torch.randn(4, 768), torch.ones(768))            # CPU tensor: no fallback
    with pytest.raises(TypeError):
        ops.rmsnorm(torch.randn(4, 768, device=dev).half(), torch.ones(768, device=dev))
    x, g = torch.randn(4, 100, device=dev), torch.ones(100, device=dev)
    for f in (lambda: ops.rmsnorm(x, g), lambda: ops.rmsnorm_fork(x, g), lambda: ops.layernorm(x, g, g),
              lambda: ops.rmsnorm_partial(x, g, None, 50)):
        with pytest.raises(M.MeantHipError, match="not a multiple of 8"):
            f()
    y = ops.rmsnorm(x, g, any_width=True)                          # d % 8 != 0: the one-row-per-workgroup kernels
    assert y.shape == (4, 100) and torch.isfinite(y).all()
    assert torch.equal(M.RMSNorm(100).to(dev)(x), y)               # the module opts in
    with pytest.raises(M.MeantHipError, match="rmsnorm_partial_fwd"):
        ops.rmsnorm_partial(x, g, None, 200, any_width=True)       # d_part > d: refused by the library
