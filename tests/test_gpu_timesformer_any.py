"""meant_amd.TimeSformer at any width and any video length ("TimeSformer at any width and any video length"):
  1. the cls query's attention over key segments (meant_attn_cls_split_fwd / _bwd) through the C ABI against float64, at the
     gates tests/test_gpu_divided.py holds the one-workgroup pair to, with segment counts that leave a shorter last segment, a
     single key per segment and an empty last segment; its refusals;
  2. two runs of it from identical buffers give identical bits;
  3. the element forms of gather_rows, token_shift, dropout and GEGLU at widths off the 8-grid: exact where they only move data;
  4. TimeSformer at dim 100, 99 and 50 against oracle.TimeSformer (float64), every parameter gradient;
  5. videos of 20 801 and 40 001 tokens, past the backward's and the forward's one-workgroup bound."""
import numpy as np
import pytest
import torch

from tests.util import DTYPES, IDS, compare_param_grads, pair

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -4
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
    """the largest L the one-workgroup kernels take: (arrays * L + 4 reduction words + rpi * Dh partials) floats within the budget"""
    rpi = CLS_THREADS // (Dh // 8)
    return (LDS_BYTES // 4 - 4 - rpi * Dh) // arrays


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the split kernels through the C ABI
# ------------------------------------------------------------------------------------------------------------------------------
def _cls_reference(qkv, mask, H, Dh, scale, dout):
    """float64: o = softmax(scale q0 . K^T, masked keys filled with -max) V per (video, head), its stats and d(o . dout)/d qkv"""
    B, L, _ = qkv.shape
    D = H * Dh
    x = qkv.double().clone().requires_grad_(True)
    q0 = x[:, 0, :D].reshape(B, H, Dh)
    k = x[:, :, D:2 * D].reshape(B, L, H, Dh)
    v = x[:, :, 2 * D:].reshape(B, L, H, Dh)
    s = torch.einsum("bhd,blhd->bhl", q0, k) * scale
    if mask is not None:
        s = s.masked_fill(mask[:, None, :] == 0, -torch.finfo(torch.float64).max)
    mx = s.max(dim=-1).values
    lse = torch.log(torch.exp(s - mx[..., None]).sum(dim=-1))
    o = torch.einsum("bhl,blhd->bhd", torch.softmax(s, dim=-1), v).reshape(B, D)
    (o * dout.double()).sum().backward()
    return o.detach(), x.grad, mx.detach(), lse.detach()


def _cls_grad_given_out(qkv, mask, H, Dh, scale, dout, out):
    """float64 gradient of the same attention with delta = dout . out taken from the output the backward is handed (the kernel's
    contract): ds = p (dout . v - delta), dq0 = scale ds K, dK = scale ds q0, dV = p dout; a masked key has no score gradient"""
    B, L, _ = qkv.shape
    D = H * Dh
    x = qkv.double()
    q0 = x[:, 0, :D].reshape(B, H, Dh)
    k = x[:, :, D:2 * D].reshape(B, L, H, Dh)
    v = x[:, :, 2 * D:].reshape(B, L, H, Dh)
    s = torch.einsum("bhd,blhd->bhl", q0, k) * scale
    if mask is not None:
        s = s.masked_fill(mask[:, None, :] == 0, -torch.finfo(torch.float64).max)
    p = torch.softmax(s, dim=-1)
    do = dout.double().reshape(B, H, Dh)
    delta = (do * out.double().reshape(B, H, Dh)).sum(dim=-1)
    ds = p * (torch.einsum("bhd,blhd->bhl", do, v) - delta[..., None])
    if mask is not None:
        ds = ds.masked_fill(mask[:, None, :] == 0, 0.0)
    g = torch.zeros(B, L, 3, D, dtype=torch.float64)
    g[:, 0, 0] = (scale * torch.einsum("bhl,blhd->bhd", ds, k)).reshape(B, D)
    g[:, :, 1] = (scale * torch.einsum("bhl,bhd->blhd", ds, q0)).reshape(B, L, D)
    g[:, :, 2] = torch.einsum("bhl,bhd->blhd", p, do).reshape(B, L, D)
    return g


def _cls_masks(B, L, rs):
    m_rand = torch.from_numpy((rs.rand(B, L) > 0.5).astype("float32"))
    m_key0 = torch.zeros(B, L)
    m_key0[:, 0] = 1
    return {"none": None, "random": m_rand, "key0": m_key0, "all": torch.zeros(B, L)}


def _split_ws(dev, B, L, H, Dh, nseg):
    lib = _lib().lib
    wsb = lib.meant_attn_cls_split_ws(B, L, H, Dh, nseg)
    assert wsb > 0
    return torch.empty(wsb, device=dev, dtype=torch.uint8), wsb


def _run_cls_split(dev, dtype, B, L, H, Dh, nseg, seed):
    """the checks of test_gpu_divided._run_cls on the split entries: output, both stats, accumulated dq / dk / dv on a pre-filled
    buffer, untouched pad columns, the q blocks of rows >= 1 bit-equal to before; and the route counter"""
    from meant_amd.ops import _dt, _p, _stream, check
    L_ = _lib()
    lib = L_.lib
    rs = np.random.RandomState(seed)
    D = H * Dh
    ld_out = D + 8                                                   # strided output rows: the pad columns must stay untouched
    scale = Dh ** -0.5
    qkv = torch.from_numpy(rs.standard_normal((B, L, 3 * D)).astype("float32")).to(dtype)
    qkv[:, 0, :D] *= 2.0                                             # a sharper softmax
    dout = torch.from_numpy(rs.standard_normal((B, ld_out)).astype("float32")).to(dtype)
    qkv_d, dout_d = qkv.to(dev), dout.to(dev)
    ws, wsb = _split_ws(dev, B, L, H, Dh, nseg)
    tol_o, tol_g = (1e-4, 1e-3) if dtype == torch.float32 else (8e-3, 2e-2)
    for name, mask in _cls_masks(B, L, rs).items():
        what = f"cls_split[{name}] B={B} L={L} H={H} Dh={Dh} nseg={nseg}"
        o_ref, g_ref, mx_ref, lse_ref = _cls_reference(qkv, mask, H, Dh, scale, dout[:, :D])
        out = torch.full((B, ld_out), 7.0, device=dev, dtype=dtype)
        stats = torch.empty((B, H, 2), device=dev, dtype=torch.float32)
        km = mask.to(dev).contiguous() if mask is not None else None
        before_hits = L_.route_count("attn_cls_split")
        check(lib.meant_attn_cls_split_fwd(_p(qkv_d), _p(out), ld_out, _p(stats), _p(km), B, L, H, Dh, scale, nseg, _dt(qkv_d), _p(ws), wsb,
                                           _stream()), "attn_cls_split_fwd")
        g_exact = _cls_grad_given_out(qkv, mask, H, Dh, scale, dout[:, :D], o_ref)
        assert torch.allclose(g_exact, g_ref.view(B, L, 3, D), rtol=1e-9, atol=1e-9 * g_ref.abs().max().item()), f"{what}: reference"
        g3 = _cls_grad_given_out(qkv, mask, H, Dh, scale, dout[:, :D], out.cpu()[:, :D])
        floor = 1e-2 * max(g3.abs().max().item(), 1e-3)
        before = torch.from_numpy(rs.standard_normal((B, L, 3, D)).astype("float32"))
        for i in range(3):
            before[:, :, i] *= max(g3[:, :, i].abs().max().item(), floor)
        before = before.view(B, L, 3 * D).to(dtype)
        dqkv = before.to(dev)
        check(lib.meant_attn_cls_split_bwd(_p(qkv_d), _p(out), ld_out, _p(dout_d), ld_out, _p(stats), _p(km), _p(dqkv), B, L, H, Dh, scale,
                                           nseg, _dt(qkv_d), _p(ws), wsb, _stream()), "attn_cls_split_bwd")
        torch.cuda.synchronize()
        assert L_.route_count("attn_cls_split") == before_hits + 2, f"{what}: route counter"
        out_c, stats_c, after = out.cpu(), stats.cpu(), dqkv.cpu()
        e = _rel(out_c[:, :D], o_ref)
        print(f"{what}: out {e:.2e}")
        assert e <= tol_o, f"{what}: output {e:.2e}"
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
            print(f"{what}: {blk} {e:.2e}")
            assert e <= tol_g, f"{what}: {blk} (accumulated) {e:.2e}"


SPLIT_SHAPES = [(1, 1), (5, 2), (5, 5), (257, 2), (257, 7), (2353, 3), (2353, 16)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("Dh", [8, 64, 96, 256])
@pytest.mark.parametrize("L,nseg", SPLIT_SHAPES, ids=[f"L{l}x{s}" for l, s in SPLIT_SHAPES])
def test_attn_cls_split_parity(dev, dtype, L, nseg, Dh, H):
    """one segment (the merge of a single partial), a last segment shorter than the others (5 = 3 + 2, 257 = 129 + 128, 2353 in 3 and
    in 16), one key per segment (5 in 5), segments shorter than the 256 threads and than the row groups; masks none / random / only
    key 0 (every segment but the first fully masked) / every key"""
    _run_cls_split(dev, dtype, 2, L, H, Dh, nseg, seed=L * 131 + Dh * 7 + H + nseg)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_attn_cls_split_empty_last_segment(dev, dtype):
    """5 keys in 4 segments of ceil(5 / 4) = 2: the fourth segment starts past the last key and must drop out of both merges"""
    _run_cls_split(dev, dtype, 2, 5, 3, 64, 4, seed=54)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("arrays", [2, 1], ids=["past_bwd_bound", "past_fwd_bound"])
def test_attn_cls_split_picks_its_segments_past_the_lds_bound(dev, dtype, arrays):
    """nseg = 0 one key past what meant_attn_cls_bwd and meant_attn_cls_fwd take at Dh = 64: 19 327 and 38 653 rows of 192 elements"""
    L = cls_max_len(64, arrays) + 1
    assert _lib().lib.meant_attn_cls_max_len(64, arrays - 1) == L - 1
    _run_cls_split(dev, dtype, 1, L, 1, 64, 0, seed=arrays)


def test_attn_cls_split_refusals(dev):
    from meant_amd.ops import _p, _stream
    lib = _lib().lib
    B, H, Dh = 2, 2, 64
    buf = torch.zeros(4096, device=dev)                             # never read: every check is on the host, before any launch
    stats = torch.zeros(B * H * 2, device=dev)
    big = torch.zeros(1 << 16, device=dev)
    nbig = big.numel() * 4

    def fwd(L, nseg, ws, wsb):
        return lib.meant_attn_cls_split_fwd(_p(buf), _p(buf), H * Dh, _p(stats), None, B, L, H, Dh, 0.1, nseg, 0, _p(ws), wsb, _stream())

    def bwd(L, nseg, ws, wsb):
        return lib.meant_attn_cls_split_bwd(_p(buf), _p(buf), H * Dh, _p(buf), H * Dh, _p(stats), None, _p(buf), B, L, H, Dh, 0.1, nseg, 0,
                                            _p(ws), wsb, _stream())
    # a given count whose segment does not fit
    assert fwd(cls_max_len(Dh, 1) + 1, 1, big, nbig) == ERR_UNSUPPORTED
    assert fwd(2 * cls_max_len(Dh, 1) + 1, 2, big, nbig) == ERR_UNSUPPORTED
    assert bwd(cls_max_len(Dh, 2) + 1, 1, big, nbig) == ERR_UNSUPPORTED
    assert bwd(2 * cls_max_len(Dh, 2) + 1, 2, big, nbig) == ERR_UNSUPPORTED
    # more segments than keys
    assert fwd(5, 6, big, nbig) == ERR_ARG and bwd(5, 6, big, nbig) == ERR_ARG
    assert fwd(5, -1, big, nbig) == ERR_ARG and bwd(5, -1, big, nbig) == ERR_ARG
    # head dim off the 8-grid, as the one-workgroup pair
    assert lib.meant_attn_cls_split_fwd(_p(buf), _p(buf), H * 100, _p(stats), None, B, 5, H, 100, 0.1, 1, 0, _p(big), nbig, _stream()) == ERR_UNSUPPORTED
    # a workspace one byte short
    for L, nseg in ((5, 2), (257, 7)):
        wsb = lib.meant_attn_cls_split_ws(B, L, H, Dh, nseg)
        assert wsb == B * H * nseg * (Dh + 2) * 4
        assert fwd(L, nseg, big, wsb - 1) == ERR_WORKSPACE and bwd(L, nseg, big, wsb - 1) == ERR_WORKSPACE
    # nseg = 0 sizes the workspace for the backward's count, which covers the forward's
    L = 2 * cls_max_len(Dh, 2) + 1
    assert lib.meant_attn_cls_split_ws(B, L, H, Dh, 0) == B * H * 3 * (Dh + 2) * 4
    assert lib.meant_attn_cls_split_ws(B, 5, H, Dh, 6) == 0 and lib.meant_attn_cls_split_ws(B, 5, H, 100, 1) == 0


# ------------------------------------------------------------------------------------------------------------------------------
# 2. bit-reproducibility
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_attn_cls_split_two_runs_same_bits(dev, dtype):
    from meant_amd.ops import _dt, _p, _stream, check
    lib = _lib().lib
    B, L, H, Dh, nseg = 2, 2353, 3, 64, 16
    D = H * Dh
    rs = np.random.RandomState(7)
    qkv = torch.from_numpy(rs.standard_normal((B, L, 3 * D)).astype("float32")).to(dtype).to(dev)
    dout = torch.from_numpy(rs.standard_normal((B, D)).astype("float32")).to(dtype).to(dev)
    before = torch.from_numpy(rs.standard_normal((B, L, 3 * D)).astype("float32")).to(dtype).to(dev)
    km = torch.from_numpy((rs.rand(B, L) > 0.3).astype("float32")).to(dev)
    runs = []
    for _ in range(2):
        ws, wsb = _split_ws(dev, B, L, H, Dh, nseg)
        ws.fill_(0xA5)                                                  # whatever the workspace held must not matter
        out = torch.empty((B, D), device=dev, dtype=dtype)
        stats = torch.empty((B, H, 2), device=dev, dtype=torch.float32)
        dqkv = before.clone()
        check(lib.meant_attn_cls_split_fwd(_p(qkv), _p(out), D, _p(stats), _p(km), B, L, H, Dh, Dh ** -0.5, nseg, _dt(qkv), _p(ws), wsb,
                                           _stream()), "attn_cls_split_fwd")
        check(lib.meant_attn_cls_split_bwd(_p(qkv), _p(out), D, _p(dout), D, _p(stats), _p(km), _p(dqkv), B, L, H, Dh, Dh ** -0.5, nseg,
                                           _dt(qkv), _p(ws), wsb, _stream()), "attn_cls_split_bwd")
        torch.cuda.synchronize()
        runs.append((out.cpu(), stats.cpu(), dqkv.cpu()))
    for a, b, what in zip(runs[0], runs[1], ("out", "stats", "dqkv")):
        assert torch.equal(a, b), what
    assert not torch.equal(runs[0][2], before.cpu())


# ------------------------------------------------------------------------------------------------------------------------------
# 3. element kernels
# ------------------------------------------------------------------------------------------------------------------------------
def _offset_by_one(t):
    """the same values in a buffer whose base is one element past a 16-byte boundary"""
    flat = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    flat[1:] = t.reshape(-1)
    v = flat[1:].view(t.shape)
    assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
    return v


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("W", [1, 3, 7, 99, 100, 1001])
def test_gather_rows_any_width_exact(dev, dtype, W):
    """meant_gather_rows at W % 8 != 0 against torch indexing, bit for bit: a permutation with -1 (zeros) and -2 (the fill row) among
    its entries, more rows than one grid pass of waves, from aligned bases and from bases one element off"""
    from meant_amd import ops
    L_ = _lib()
    rs = np.random.RandomState(W)
    n_src = 41
    src = torch.from_numpy(rs.standard_normal((n_src, W)).astype("float32")).to(dtype)
    fill = torch.from_numpy(rs.standard_normal(W).astype("float32")).to(dtype)
    idx = np.concatenate((rs.permutation(n_src), [-1, -2, 0, -2, -1, n_src - 1]))
    rs.shuffle(idx)
    idx_t = torch.from_numpy(idx.astype("int32"))
    ref = torch.zeros(len(idx), W, dtype=dtype)
    for r, i in enumerate(idx):
        if i >= 0:
            ref[r] = src[i]
        elif i == -2:
            ref[r] = fill
    src_d, fill_d, idx_d = src.to(dev), fill.to(dev), idx_t.to(dev)
    for name, s_, f_ in (("aligned", src_d, fill_d), ("base+1", _offset_by_one(src_d), _offset_by_one(fill_d))):
        hits = L_.route_count("rows_elem")
        got = ops.gather_rows(s_, idx_d, f_)
        torch.cuda.synchronize()
        assert L_.route_count("rows_elem") == hits + 1, f"W={W} {name}: route"
        assert torch.equal(got.cpu(), ref), f"W={W} {name}"
    no_fill = ops.gather_rows(src_d, idx_d)                           # -2 without a fill row: zeros, as the 16-byte kernel
    ref[torch.from_numpy(idx == -2)] = 0
    assert torch.equal(no_fill.cpu(), ref), f"W={W} no fill"


def _shift_reference(x, f):
    from oracle import meant_oracle as O
    return O._TSPreTokenShift(f, lambda y: y)(x)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d", [3, 4, 100, 770])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("f", [1, 3])
def test_token_shift_any_width_exact(dev, dtype, f, n, d):
    """meant_token_shift at d % 8 != 0: forward == the oracle's PreTokenShift and transpose == its autograd backward, element for
    element (thirds of 1 column, remainder columns, a last thread with 2 or 4 live columns); <S x, y> == <x, S^T y>"""
    from meant_amd.ops import _dt, _p, _stream, check
    L_ = _lib()
    lib = L_.lib
    rs = np.random.RandomState(f * 1000 + n * 10 + d)
    B, L = 2, 1 + f * n
    x = torch.from_numpy(rs.standard_normal((B, L, d)).astype("float32")).to(dtype)
    yb = torch.from_numpy(rs.standard_normal((B, L, d)).astype("float32")).to(dtype)
    xr = x.float().requires_grad_(True)
    ref = _shift_reference(xr, f)
    ref.backward(yb.float())
    x_d, yb_d = x.to(dev), yb.to(dev)
    sx, sty = torch.full_like(x_d, 9.0), torch.full_like(x_d, 9.0)
    hits = L_.route_count("rows_elem")
    check(lib.meant_token_shift(_p(x_d), _p(sx), B, f, n, d, 0, _dt(x_d), _stream()), "token_shift")
    check(lib.meant_token_shift(_p(yb_d), _p(sty), B, f, n, d, 1, _dt(x_d), _stream()), "token_shift^T")
    torch.cuda.synchronize()
    assert L_.route_count("rows_elem") == hits + 2
    assert torch.equal(sx.cpu(), ref.detach().to(dtype)), f"shift f={f} n={n} d={d}"
    assert torch.equal(sty.cpu(), xr.grad.to(dtype)), f"shift^T f={f} n={n} d={d}"
    lhs = (sx.cpu().double() * yb.double()).sum().item()
    rhs = (x.double() * sty.cpu().double()).sum().item()
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0), (lhs, rhs)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [1, 7, 8, 9, 8 * 1000 + 5])
def test_dropout_any_length(dev, dtype, n):
    """meant_dropout at n % 8 != 0: the first 8 * (n // 8) outputs are, bit for bit, what the 16-byte kernel gives for that prefix;
    the all-element route of an unaligned base gives the same bits; every output is 0 or x times the float 1 / (1 - p); the backward
    of ops.dropout reproduces the mask.  n = 8 stays on the 16-byte kernel."""
    from meant_amd import ops
    from meant_amd.ops import _dt, _p, _stream, check
    L_ = _lib()
    lib = L_.lib
    p, seed = 0.25, 1234
    rs = np.random.RandomState(n)
    x = torch.from_numpy(rs.standard_normal(n).astype("float32"))
    x[x.abs() < 0.1] = 0.5                                           # no zeros: a zero output is a dropped element
    x_d = x.to(dtype).to(dev)
    y = torch.full_like(x_d, 9.0)
    hits = L_.route_count("rows_elem")
    check(lib.meant_dropout(_p(x_d), _p(y), n, p, seed, _dt(x_d), _stream()), "dropout")
    torch.cuda.synchronize()
    assert L_.route_count("rows_elem") == hits + (1 if n % 8 else 0)
    n8 = 8 * (n // 8)
    if n8:
        y8 = torch.empty(n8, device=dev, dtype=dtype)
        check(lib.meant_dropout(_p(x_d), _p(y8), n8, p, seed, _dt(x_d), _stream()), "dropout")   # n8 % 8 == 0: the existing kernel
        assert torch.equal(y[:n8].cpu(), y8.cpu()), f"n={n}: prefix"
    x_o = _offset_by_one(x_d)
    y_o = _offset_by_one(torch.full_like(x_d, 9.0))
    if n % 8:                                                        # an unaligned base: every group element by element
        check(lib.meant_dropout(_p(x_o), _p(y_o), n, p, seed, _dt(x_d), _stream()), "dropout")
        assert torch.equal(y_o.cpu(), y.cpu()), f"n={n}: unaligned base"
    sc = torch.tensor(65536.0 / (65536.0 - 16384.0), dtype=torch.float32)      # keep_scale8's multiplier at p = 0.25
    kept = (x_d.cpu().float() * sc).to(dtype)
    y_c = y.cpu()
    assert torch.all((y_c == 0) | (y_c == kept)), f"n={n}: an output that is neither 0 nor x / (1 - p)"
    if n > 1000:
        rate = (y_c != 0).float().mean().item()
        assert abs(rate - 0.75) < 0.03, rate
    xg = x_d.clone().requires_grad_(True)
    yg = ops.dropout(xg, p, seed)
    yg.backward(torch.ones_like(yg))
    assert torch.equal(yg.detach().cpu(), y_c)
    assert torch.equal(xg.grad.cpu(), torch.where(y_c != 0, sc.to(dtype), torch.zeros((), dtype=dtype)).expand(n)), f"n={n}: backward mask"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("w", [2, 198, 396, 1001])
def test_geglu_any_width(dev, dtype, w):
    """ops.geglu at w % 8 != 0 (w = 4 dim for dim = 99; 2 and 1001 for a single partial chunk and an odd one), forward and backward
    against float64 at test_geglu_parity's gates"""
    from meant_amd import ops
    L_ = _lib()
    rs = np.random.RandomState(w)
    rows = 131
    h = torch.from_numpy(rs.standard_normal((rows, 2 * w)).astype("float32")).to(dtype)
    dy = torch.from_numpy(rs.standard_normal((rows, w)).astype("float32")).to(dtype)
    hr = h.double().requires_grad_(True)
    a, g = hr.chunk(2, dim=-1)
    yr = a * torch.nn.functional.gelu(g)
    yr.backward(dy.double())
    hd = h.to(dev).requires_grad_(True)
    hits = L_.route_count("rows_elem")
    y = ops.geglu(hd)
    y.backward(dy.to(dev))
    torch.cuda.synchronize()
    assert L_.route_count("rows_elem") == hits + 2
    tol_o, tol_g = (2e-5, 2e-5) if dtype == torch.float32 else (8e-3, 1e-2)
    assert _rel(y, yr) <= tol_o, f"geglu fwd {_rel(y, yr):.2e}"
    assert _rel(hd.grad, hr.grad) <= tol_g, f"geglu bwd {_rel(hd.grad, hr.grad):.2e}"


# ------------------------------------------------------------------------------------------------------------------------------
# 4. / 5. meant_amd.TimeSformer against oracle.TimeSformer in float64
# ------------------------------------------------------------------------------------------------------------------------------
_SMALL = dict(num_frames=3, image_size=32, patch_size=16, depth=2)
_LONG = dict(dim=16, heads=2, dim_head=8, image_size=80, patch_size=2, depth=1)
MODEL_CASES = {
    "dim100": dict(kw=dict(_SMALL, dim=100, heads=2, dim_head=16), b=2, hw=(32, 32)),
    "dim99": dict(kw=dict(_SMALL, dim=99, heads=3, dim_head=20), b=2, hw=(32, 32)),
    "dim99_mask": dict(kw=dict(_SMALL, dim=99, heads=3, dim_head=20), b=2, hw=(32, 32), mask=True),
    "dim99_shift": dict(kw=dict(_SMALL, dim=99, heads=3, dim_head=20, shift_tokens=True), b=2, hw=(32, 32)),
    "dim50_posemb": dict(kw=dict(_SMALL, dim=50, heads=2, dim_head=8, rotary_emb=False), b=2, hw=(32, 32)),
    "frames13": dict(kw=dict(_LONG, num_frames=13), b=1, hw=(80, 80), routes=dict(attn_cls=2, attn_cls_split=2)),     # 20 801 tokens
    "frames25": dict(kw=dict(_LONG, num_frames=25), b=1, hw=(80, 80), routes=dict(attn_cls=0, attn_cls_split=4)),     # 40 001 tokens
}
_ORACLE_RUNS = {}


def _model_case(name):
    cfg = MODEL_CASES[name]
    f = cfg["kw"]["num_frames"]
    rs = np.random.RandomState(len(name) * 17 + f)
    b, (hh, ww) = cfg["b"], cfg["hw"]
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


def _maxerr_scaled(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / max(1.0, b.abs().max().item())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_timesformer_any_vs_oracle(dev, dtype, case):
    """the procedure and gates of test_gpu_divided.test_timesformer_vs_oracle at widths off the 8-grid (dim 100 and 99, head dims 16,
    20 and 8, frame mask, token shift, learned positions) and at 20 801 / 40 001 tokens: 13 frames run the cls backward over key
    segments and its forward on the one-workgroup kernel, 25 frames run both over segments"""
    import meant_amd as M
    from oracle import meant_oracle as O
    L_ = _lib()
    cfg = MODEL_CASES[case]
    kw = dict(cfg["kw"], num_classes=3, channels=3)
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
    L_.route_reset()
    x = hip.meant_forward(video.to(dev), mask=mask.to(dev) if mask is not None else None)
    logits = hip.to_out(x[:, 0])
    loss = _loss(x.float(), logits.float(), target.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    for route, hits in cfg.get("routes", {}).items():
        assert L_.route_count(route) == hits, f"{case}: route {route} took {L_.route_count(route)} calls, expected {hits}"
    if "routes" not in cfg:
        assert L_.route_count("rows_elem") > 0, f"{case}: no element-form launch"
    tol = 2e-4 if dtype == torch.float32 else 4e-2                          # the golden test's gates, relative to the largest value
    print(f"{case}: tokens {_rel(x, x_r):.2e} logits {_maxerr_scaled(logits, logits_r):.2e} loss {loss.item()} vs {loss_r}")
    assert _rel(x, x_r) <= tol, f"{case}: tokens {_rel(x, x_r):.2e}"
    assert _maxerr_scaled(logits, logits_r) <= tol, f"{case}: logits"
    assert abs(loss.item() - loss_r) <= (1e-4 if dtype == torch.float32 else 2e-2) * abs(loss_r), f"{case}: loss {loss.item()} vs {loss_r}"
    compare_param_grads(ref, hip, dtype, case)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_timesformer_odd_width_trains_with_dropout(dev, dtype):
    """train mode at dim = 99 with both dropouts (the oracle has none): the odd-length dropout calls run, outputs and gradients finite"""
    import meant_amd as M
    L_ = _lib()
    torch.manual_seed(5)
    m = M.TimeSformer(dim=99, heads=3, dim_head=20, num_classes=3, channels=3, attn_dropout=0.1, ff_dropout=0.1, **_SMALL).to(dev).train()
    m.compute_dtype = dtype
    L_.route_reset()
    out = m(torch.randn(2, 3, 3, 32, 32, device=dev))
    out.float().sum().backward()
    torch.cuda.synchronize()
    assert L_.route_count("rows_elem") > 0
    assert out.shape == (2, 3) and torch.isfinite(out.float()).all()
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
