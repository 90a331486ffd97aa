"""meant_qkv_embed_bwd_by_id without a GPU: the header binding, the option and the route name, the workspace arithmetic, the argument
checks that come before any launch, and a float64 emulation (with the kernels' bf16 roundings) of the per-token and the by-id route,
which says what the 2x error margin of tests/test_gpu_qkv_by_id.py asks of each."""
import pytest
import torch

from meant_amd import _lib

lib = _lib.lib


def test_binding_comes_from_the_header():
    res, args = _lib.SIGNATURES["meant_qkv_embed_bwd_by_id"]
    assert len(args) == 23 and res is not None
    assert len(_lib.SIGNATURES["meant_qkv_embed_bwd_by_id_ws"][1]) == 4
    assert (_lib.BY_ID_SHARED, _lib.BY_ID_TABLE) == (1, 2)
    assert _lib.get_option("qkv_by_id") in (0, 1, 2)
    assert _lib.route_count("qkv_by_id") >= 0


def test_option_round_trip():
    saved = _lib.get_option("qkv_by_id")
    try:
        for v in (0, 2, 1):
            _lib.set_option("qkv_by_id", v)
            assert _lib.get_option("qkv_by_id") == v
    finally:
        _lib.set_option("qkv_by_id", saved)


def test_automatic_rule_is_a_comparison_of_shapes():
    from meant_amd import ops
    saved = _lib.get_option("qkv_by_id")
    try:
        _lib.set_option("qkv_by_id", 1)
        assert ops.qkv_by_id_wanted(128 * 12 * 512, 64001)               # the headline step: T / V = 12.3
        assert ops.qkv_by_id_wanted(6 * 64001, 64001) and not ops.qkv_by_id_wanted(6 * 64001 - 1, 64001)
        assert not ops.qkv_by_id_wanted(128 * 512, 64001)                # meant_vqa at 128 samples: T = V
        assert not ops.qkv_by_id_wanted(4096, 50)                        # a small table, however often its rows repeat
        _lib.set_option("qkv_by_id", 0)
        assert not ops.qkv_by_id_wanted(128 * 12 * 512, 64001)
        _lib.set_option("qkv_by_id", 2)
        assert ops.qkv_by_id_wanted(768, 300)
    finally:
        _lib.set_option("qkv_by_id", saved)
    bf = torch.bfloat16
    assert ops.qkv_by_id_shape_ok(768, 768, 64, 64001, bf) and ops.qkv_by_id_shape_ok(256, 256, 64, 300, bf)
    assert not ops.qkv_by_id_shape_ok(768, 768, 64, 64001, torch.float32)
    assert not ops.qkv_by_id_shape_ok(128, 128, 64, 100, bf)             # H Dh % 256 != 0
    assert not ops.qkv_by_id_shape_ok(772, 768, 64, 64001, bf)           # d % 8 != 0


def _ws(n, d, N3, V):
    return lib.meant_qkv_embed_bwd_by_id_ws(n, d, N3, V)


def test_workspace_arithmetic():
    n, d, N3, V = 786432, 768, 2304, 64001
    Vp = (V + 255) // 256 * 256
    nst = (n + 255) // 256
    # hi | lo images of D; the normalised table and three dN buffers (bf16); the fp32 dN, table image and per-id dx rows; the norm's
    # 1 / rms and the epilogue's ones; the crossing runs' partial sums and the column sums; the run lengths; the live flags
    floor = 2 * Vp * N3 * 2 + 4 * Vp * d * 2 + 3 * V * d * 4 + V * 4 + Vp * 4 + nst * 3 * N3 * 4 + nst * 4 + n // 64
    ws = _ws(n, d, N3, V)
    assert floor <= ws <= floor + 16 * 256 + max(lib.meant_rmsnorm_bwd_ws(V, d), lib.meant_embedding_bwd_seg_ws(n, d),
                                                lib.meant_linear_bwd_dw_ws(Vp, N3, d, _lib.BF16)) + 256
    saved = _lib.get_option("deterministic")
    try:
        _lib.set_option("deterministic", 1)
        assert _ws(n, d, N3, V) >= ws                        # the ordered dW partials share the launchers' region
        assert _ws(n, d, N3, V) >= lib.meant_linear_bwd_dw_ws(Vp, N3, d, _lib.BF16)
    finally:
        _lib.set_option("deterministic", saved)
    assert _ws(768, 256, 768, 300) > 0 and _ws(1, 8, 192, 1) > 0
    assert _ws(768, 256, 768, 300) < _ws(768, 256, 768, 301 + 256)
    for bad in ((0, 256, 768, 300), (768, 252, 768, 300), (768, 256, 770, 300), (768, 256, 768, 0), (1 << 31, 256, 768, 300),
                (768, 256, 768, 1 << 31), (768, 256, 3 * 32, 300)):
        assert _ws(*bad) == 0, bad


def test_argument_checks_come_before_any_launch():
    """no device pointer is touched: the calls fail on their arguments (ids missing, unknown stage bits, a shape outside the route)"""
    z = None
    one = 4096                                               # stands for a non-null, 16-byte aligned address; never dereferenced
    def call(sorted_ids=one, stage=3, d=256, lo=0, hi=300, ws=one, wsb=1 << 40):
        return lib.meant_qkv_embed_bwd_by_id(one, z, sorted_ids, one, one, one, 1e-8, one, z, one, one, one, one, 768, d, 768, 300, lo, hi, stage,
                                             ws, wsb, z)
    assert call(sorted_ids=z) == _lib.ERR_ARG
    assert call(stage=0) == _lib.ERR_ARG and call(stage=4) == _lib.ERR_ARG
    assert call(d=252) == _lib.ERR_UNSUPPORTED
    assert call(lo=5, hi=4) == _lib.ERR_ARG and call(hi=301) == _lib.ERR_ARG
    assert call(wsb=16) == _lib.ERR_WORKSPACE
    assert call(ws=one + 4) == _lib.ERR_ARG


# ---- what the rounding points of the two routes do to the gradients -------------------------------------------------------------------
def _bf(x):
    return x.to(torch.bfloat16).double()


def _f32(x):
    return x.float().double()


def _emulate(hot_share, lo_image=True, seed=0):
    """worst errors, relative to the largest fp64 element, of (per-token, by-id) for dW', dgain and dtable"""
    V, d, N3, T, eps = 48, 64, 192, 1024, 1e-8
    g_ = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V, (T,), generator=g_)
    ids[torch.rand(T, generator=g_) < hot_share] = 7
    tab = _bf(torch.randn(V, d, generator=g_, dtype=torch.float64))
    gain = _f32(1 + 0.2 * torch.randn(d, generator=g_, dtype=torch.float64))
    W = _bf(torch.randn(N3, d, generator=g_, dtype=torch.float64) / d ** 0.5)
    dqkv = torch.randn(T, N3, generator=g_, dtype=torch.float64)
    dqkv[ids == 7] += 0.5
    dqkv = _bf(dqkv)
    dres = _bf(torch.randn(T, d, generator=g_, dtype=torch.float64))

    def norm_fwd(x):
        rinv = 1.0 / (x.norm(dim=-1, keepdim=True) * d ** -0.5 + eps)
        return x * rinv, rinv

    def norm_bwd(dn, x):                                     # of n = gain * x * rinv, rinv = 1 / (|x| / sqrt(d) + eps)
        xh, rinv = norm_fwd(x)
        gdn = gain * dn
        rms = x.norm(dim=-1, keepdim=True) * d ** -0.5
        return gdn * rinv - x * ((gdn * x).sum(-1, keepdim=True) * rinv * rinv / (d * rms)), (dn * xh).sum(0)

    onehot = torch.zeros(T, V, dtype=torch.float64)
    onehot[torch.arange(T), ids] = 1
    # fp64 from the same operands
    x = tab[ids]
    xh, _ = norm_fwd(x)
    n = gain * xh
    ref_dW = dqkv.t() @ n
    dx, ref_dg = norm_bwd(dqkv @ W, x)
    ref_dt = onehot.t() @ (dx + dres)
    # per token: n, dn and dx are bf16 tensors
    n_b = _bf(n)
    tok_dW = dqkv.t() @ n_b
    dn_b = _bf(dqkv @ W)
    dx_b, tok_dg = norm_bwd(dn_b, x)
    tok_dt = onehot.t() @ _bf(dx_b + dres)
    # by id: D and dNtab are two bf16 images each (hi + lo), Ntab one, the norm backward runs in fp32 on V rows
    D = _f32(onehot.t() @ dqkv)
    hi = _bf(D)
    lo = _bf(D - hi) if lo_image else torch.zeros_like(D)
    ntab = _bf(gain * norm_fwd(tab)[0])
    id_dW = hi.t() @ ntab + lo.t() @ ntab
    dNlo = _bf(lo @ W)
    dN = _bf(hi @ W + dNlo)
    dN = _f32(dN + _bf(_f32(hi @ W + dNlo) - dN))            # the second image: what the first rounding dropped
    dxt, id_dg = norm_bwd(dN, tab)
    id_dt = _f32(dxt) + onehot.t() @ dres
    err = lambda a, r: ((a - r).abs().max() / r.abs().max()).item()
    return ({"dw": err(tok_dW, ref_dW), "dgain": err(tok_dg, ref_dg), "dtable": err(tok_dt, ref_dt)},
            {"dw": err(id_dW, ref_dW), "dgain": err(id_dg, ref_dg), "dtable": err(id_dt, ref_dt)})


def test_norm_backward_of_the_emulation_is_the_derivative():
    """the closed form used above against autograd, so that the emulation says something about the kernels' formula"""
    d, eps = 16, 1e-8
    x = torch.randn(5, d, dtype=torch.float64, requires_grad=True)
    gain = torch.randn(d, dtype=torch.float64)
    dn = torch.randn(5, d, dtype=torch.float64)
    n = gain * x / (x.norm(dim=-1, keepdim=True) * d ** -0.5 + eps)
    (ref,) = torch.autograd.grad((n * dn).sum(), x)
    rms = x.detach().norm(dim=-1, keepdim=True) * d ** -0.5
    rinv = 1.0 / (rms + eps)
    gdn = gain * dn
    got = gdn * rinv - x.detach() * ((gdn * x.detach()).sum(-1, keepdim=True) * rinv * rinv / (d * rms))
    assert (got - ref).abs().max().item() < 1e-12


@pytest.mark.parametrize("hot_share", [0.0, 0.3, 0.9])
def test_emulated_by_id_error_within_twice_the_per_token_error(hot_share):
    """with the hi + lo images the by-id route's roundings (V rows, once each) stay inside twice the per-token route's (every token);
    the per-token figures themselves are the bf16 roundings of n, dn and dx: a few 1e-3 of the largest element"""
    tok, by_id = _emulate(hot_share)
    for k in tok:
        assert tok[k] < 2e-2, (k, tok[k])
        assert by_id[k] <= 2 * tok[k], (k, by_id[k], tok[k])
