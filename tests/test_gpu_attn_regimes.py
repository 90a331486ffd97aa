"""The attention cores under peaked and shifted softmaxes, through the C ABI against float64 on the host.

Every other attention test feeds the kernels randn activations at scale 1/sqrt(H*Dh) or 0.7/sqrt(Dh): scores of standard deviation
below 1, every probability close to 1/S, a running maximum that barely moves.  Here the inputs come from
attn_ref.regime_inputs: `sharp` (score deviation 6, a median largest probability above 0.5), `rising` / `falling` (the row maximum
moves up in every 64-key tile / is set by the first tile, while the other tiles keep a sizeable share of the mass) and `offset+` /
`offset-` (every score near +-100, +-144 in the log2 domain: exp2 without the maximum subtracted overflows or gives 0 / 0).  Each
test runs forward then backward on NaN-prefilled outputs, asserts the route counters so that the shape provably reaches the kernel
it is meant for, and compares with float64 on the same bf16-exact inputs within tests.util.TOL and attn_ref._check's bounds.
tests/test_attn_regimes_host.py shows on the host that these checks reject a flash kernel with a missing rescale, no maximum
subtraction, a tile maximum in the wrong units, a missing delta term or a wrong stored maximum.

  bf16 flash kernels   Dh 64 ... 256, (S, causal, mask) of CASES; at Dh = 64 the single-pass and the two-pass backward
  one-wave kernels     S = 16, Dh 64 / 128
  f32 tier, fp32 detour   f32 at Dh 64 / 40, bf16 at Dh 40
  cls query            meant_attn_cls_fwd / _bwd and the split pair with three segments, both tiers
  temporal core        meant_temporal_attn_fwd / _bwd at L = 64 (short-lag kernels) and 200 (long-lag), both tiers

In the four regimes that put the score on a carrier (lane 0 of q and k), lane 0 of dq is left out of the comparison (it must be
finite): see attn_ref.carrier_columns.  Masks are `none`, `suffix` and `holes`, which keep key 0 live, so that every query row has a
live visible key.  Fully padded rows are left out on purpose: at |score| > 32 the reference's fp32 sum s - 1e9 no longer absorbs the
score (it rounds to multiples of 64), and the contract of include/meant_hip.h ("the score itself absorbed") stops matching the
reference there.

The worst error every route reached in every regime on an MI355X is in profiles/attn_regimes_errors.txt."""
import functools

import numpy as np
import pytest
import torch

from tests.attn_ref import (REGIMES, _check, _cls_grad_given_out, _cls_reference, _mask, _reference, _rel, _run, carrier_columns, is_carrier,
                            regime_inputs)
from tests.util import DTYPES, IDS, TOL

pytestmark = pytest.mark.gpu

G, H = 2, 2
SEED = 11
ATTN_ROUTES = ("attn_fwd", "attn_fwd_d96", "attn_fwd_d128", "attn_fwd_d160", "attn_fwd_d192", "attn_fwd_d256", "attn_bwd", "attn_bwd_d96",
               "attn_bwd_d128", "attn_bwd_d160", "attn_bwd_d192", "attn_bwd_d256", "attn_bwd1", "attn_generic", "attn_short", "attn_cls")
CASES = [(196, 0, "none"), (512, 1, "suffix"), (300, 1, "holes"), (1100, 0, "suffix")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=2)
def _case(S, Dh, regime, causal, mask_kind, natural):
    """inputs, mask and float64 reference of one case, shared by the tests that run it on more than one route (they follow each other)"""
    qkv, do, scale = regime_inputs(G, S, H, Dh, regime, SEED, causal=causal)
    mask = _mask(mask_kind, G, S, np.random.RandomState(SEED + S))
    return qkv, do, scale, mask, _reference(qkv, do, mask, G, S, H, Dh, scale, causal, natural=natural)


def _skip(regime, Dh):
    return carrier_columns(H, Dh) if is_carrier(regime) else None


def _report(route, regime, fig):
    print(f"regime-errors route={route} regime={regime} " + " ".join(f"{k}={v:.2e}" for k, v in fig.items()))


def _core_case(dev, dtype, S, Dh, regime, causal, mask_kind, expected, route, option=None):
    """one forward + backward of meant_attn_fwd / _bwd: the whole route table, then _check against float64"""
    from meant_amd import _lib
    natural = dtype == torch.float32 or bool(expected.get("attn_generic"))       # the f32 tier and the fp32 detour keep natural-log units
    qkv, do, scale, mask, ref = _case(S, Dh, regime, causal, mask_kind, natural)
    old = _lib.get_option(option[0]) if option else None
    try:
        if option:
            _lib.set_option(*option)
        o, lse, dqkv, counts = _run(qkv.to(dev).to(dtype), do.to(dev).to(dtype), mask, G, S, H, Dh, scale, causal, route_names=ATTN_ROUTES, dtype=dtype)
    finally:
        if option:
            _lib.set_option(option[0], old)
    what = f"{route} {regime} S={S} causal={causal} mask={mask_kind}"
    assert counts == {r: expected.get(r, 0) for r in ATTN_ROUTES}, f"{what}: {counts}"
    tier = torch.float32 if dtype == torch.float32 else torch.bfloat16
    fig = _check(o, lse, dqkv, ref, H, Dh, what, tol=TOL[tier], skip_dq=_skip(regime, Dh))
    _report(route, regime, fig)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the bf16 flash kernels; at Dh = 64 the backward in its single-pass form (S <= 256, causal S <= 512) and as two passes
def _flash_params():
    out = []
    for Dh in (64, 96, 128, 160, 192, 256):
        for S, causal, mask_kind in CASES:
            cid = f"Dh{Dh}-S{S}-c{causal}-{mask_kind}"
            if Dh != 64:
                out.append(pytest.param(Dh, S, causal, mask_kind, None, {f"attn_fwd_d{Dh}": 1, "attn_bwd": 1, f"attn_bwd_d{Dh}": 1}, id=cid))
                continue
            one_pass = S <= 256 or (causal and S <= 512)
            out.append(pytest.param(Dh, S, causal, mask_kind, None, {"attn_fwd": 1, "attn_bwd1" if one_pass else "attn_bwd": 1}, id=cid))
            if (S, causal, mask_kind) in CASES[:2]:
                out.append(pytest.param(Dh, S, causal, mask_kind, ("attn_bwd1", 0), {"attn_fwd": 1, "attn_bwd": 1}, id=cid + "-two_pass"))
    return out


@pytest.mark.parametrize("Dh,S,causal,mask_kind,option,expected", _flash_params())
@pytest.mark.parametrize("regime", REGIMES)
def test_flash_regimes(dev, regime, Dh, S, causal, mask_kind, option, expected):
    route = f"flash_d{Dh}" + ("" if Dh != 64 else "_bwd1" if expected.get("attn_bwd1") else "_two_pass")
    _core_case(dev, torch.bfloat16, S, Dh, regime, causal, mask_kind, expected, route, option)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the one-wave kernels (attn_short.hip): S = 16
@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("Dh", [64, 128])
@pytest.mark.parametrize("regime", REGIMES)
def test_one_wave_regimes(dev, regime, Dh, causal):
    _core_case(dev, torch.bfloat16, 16, Dh, regime, causal, "suffix", {"attn_short": 2}, f"short_d{Dh}")


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the f32 tier (materialised scores, no attn_* counter moves) and the bf16 detour through it at a head dim that is not native
@pytest.mark.parametrize("tier", ["f32_d64", "f32_d40", "generic_d40"])
@pytest.mark.parametrize("S,causal,mask_kind", [CASES[0], CASES[2]])
@pytest.mark.parametrize("regime", REGIMES)
def test_f32_and_detour_regimes(dev, regime, S, causal, mask_kind, tier):
    dtype, Dh, expected = {"f32_d64": (torch.float32, 64, {}), "f32_d40": (torch.float32, 40, {}),
                           "generic_d40": (torch.bfloat16, 40, {"attn_generic": 2})}[tier]
    _core_case(dev, dtype, S, Dh, regime, causal, mask_kind, expected, tier)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the cls query's attention, whole and over three key segments
def _run_cls_pair(dev, qkv_d, dout_d, km, B, L, Dh, scale, nseg):
    """forward, then the backward accumulated on zeros; nseg = 0: meant_attn_cls_fwd / _bwd, otherwise the split pair"""
    from meant_amd import _lib
    from meant_amd.ops import _dt, _p, _stream, check
    lib = _lib.lib
    D = H * Dh
    out = torch.full((B, D), float("nan"), device=dev, dtype=qkv_d.dtype)
    stats = torch.full((B, H, 2), float("nan"), device=dev, dtype=torch.float32)
    dqkv = torch.zeros_like(qkv_d)
    _lib.route_reset()
    if nseg == 0:
        check(lib.meant_attn_cls_fwd(_p(qkv_d), _p(out), D, _p(stats), _p(km), B, L, H, Dh, scale, _dt(qkv_d), _stream()), "attn_cls_fwd")
        check(lib.meant_attn_cls_bwd(_p(qkv_d), _p(out), D, _p(dout_d), D, _p(stats), _p(km), _p(dqkv), B, L, H, Dh, scale, _dt(qkv_d), _stream()),
              "attn_cls_bwd")
    else:
        wsb = lib.meant_attn_cls_split_ws(B, L, H, Dh, nseg)
        assert wsb > 0
        ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
        check(lib.meant_attn_cls_split_fwd(_p(qkv_d), _p(out), D, _p(stats), _p(km), B, L, H, Dh, scale, nseg, _dt(qkv_d), _p(ws), wsb, _stream()),
              "attn_cls_split_fwd")
        check(lib.meant_attn_cls_split_bwd(_p(qkv_d), _p(out), D, _p(dout_d), D, _p(stats), _p(km), _p(dqkv), B, L, H, Dh, scale, nseg, _dt(qkv_d),
                                           _p(ws), wsb, _stream()), "attn_cls_split_bwd")
    torch.cuda.synchronize()
    counts = {r: _lib.route_count(r) for r in ("attn_cls", "attn_cls_split")}
    return out.cpu(), stats.cpu().double(), dqkv.cpu(), counts


def _stats_close(a, b):
    return bool(((a - b).abs() <= 1e-4 * (1 + b.abs())).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("regime", REGIMES)
def test_cls_query_regimes(dev, dtype, regime):
    """B = 2, L = 300, Dh = 64, a random suffix of padding; the carrier sits on the row-0 query.  Output, the (max, log-sum) pair within
    1e-4 (1 + |ref|), and dq of row 0 / dk / dv against the float64 gradient with delta from the stored output; the split pair against
    float64 and against the unsplit pair"""
    B, L, Dh = 2, 300, 64
    D = H * Dh
    x, do, scale = regime_inputs(B, L, H, Dh, regime, SEED)
    qkv, dout = x.view(B, L, 3 * D), do.view(B, L, D)[:, 0].contiguous()
    mask = torch.from_numpy(_mask("suffix", B, L, np.random.RandomState(SEED)))
    o_ref, g_ref, mx_ref, lse_ref = _cls_reference(qkv, mask, H, Dh, scale, dout)
    g_exact = _cls_grad_given_out(qkv, mask, H, Dh, scale, dout, o_ref)
    assert torch.allclose(g_exact, g_ref.view(B, L, 3, D), rtol=1e-9, atol=1e-9 * g_ref.abs().max().item()), "reference"
    st_ref = torch.stack([mx_ref, lse_ref], dim=-1)
    qkv_d, dout_d, km = qkv.to(dev).to(dtype), dout.to(dev).to(dtype), mask.to(dev)
    tol = TOL[dtype]
    keep = ~carrier_columns(H, Dh) if is_carrier(regime) else torch.ones(D, dtype=torch.bool)
    results = {}
    for nseg, want in ((0, {"attn_cls": 1, "attn_cls_split": 0}), (3, {"attn_cls": 0, "attn_cls_split": 2})):
        route = ("cls_split_" if nseg else "cls_") + IDS[DTYPES.index(dtype)]
        what = f"{route} {regime}"
        out, stats, dqkv, counts = _run_cls_pair(dev, qkv_d, dout_d, km, B, L, Dh, scale, nseg)
        assert counts == want, f"{what}: {counts}"
        assert not torch.isnan(out.float()).any() and not torch.isnan(stats).any() and torch.isfinite(dqkv.float()).all(), f"{what}: unwritten output"
        fig = {"o": _rel(out, o_ref), "m": (stats[..., 0] - mx_ref).abs().max().item(), "l": (stats[..., 1] - lse_ref).abs().max().item()}
        g3 = _cls_grad_given_out(qkv, mask, H, Dh, scale, dout, out)
        got = dqkv.double().view(B, L, 3, D)
        assert torch.equal(got[:, 1:, 0], torch.zeros_like(got[:, 1:, 0])), f"{what}: q block of a row >= 1 touched"
        gmax = g3.abs().max().item()
        for i, blk in enumerate(("dq", "dk", "dv")):
            a, b = (got[:, :1, 0][..., keep], g3[:, :1, 0][..., keep]) if i == 0 else (got[:, :, i], g3[:, :, i])
            fig[blk] = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-3 * gmax)
            fig[blk + "_norm"] = abs(a.norm().item() - b.norm().item()) / max(b.norm().item(), 1e-3 * g3.norm().item())
        _report(route, regime, fig)
        assert fig["o"] <= tol["out"], f"{what}: o {fig['o']:.2e}"
        assert _stats_close(stats, st_ref), f"{what}: stats off by {fig['m']:.2e} (max), {fig['l']:.2e} (log-sum)"
        for blk in ("dq", "dk", "dv"):
            assert fig[blk] <= tol["gelem"], f"{what}: {blk} {fig[blk]:.2e}"
            assert fig[blk + "_norm"] <= tol["gnorm"], f"{what}: {blk} norm off by {fig[blk + '_norm']:.2e}"
        results[nseg] = (out, stats)
    assert _rel(results[3][0], results[0][0]) <= tol["out"], f"{regime}: split output against the unsplit one"
    assert _stats_close(results[3][1], results[0][1]), f"{regime}: split stats against the unsplit ones"


# ------------------------------------------------------------------------------------------------------------------------------
# 5. the temporal core: the last lag step's query over L keys, key l in the role of j
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("L", [64, 200])
@pytest.mark.parametrize("regime", REGIMES)
def test_temporal_regimes(dev, dtype, regime, L):
    """the stored p, o, dq and dkv of meant_temporal_attn_fwd / _bwd against float64: L = 64 on the one-wave kernels, L = 200 on the
    long-lag ones (route temporal_long), whose waves merge their running maxima through LDS"""
    from meant_amd import _lib
    from meant_amd.ops import _dt, _p, _stream, check
    lib = _lib.lib
    B, Dh = 2, 64
    D = H * Dh
    x, do, scale = regime_inputs(B, L, H, Dh, regime, SEED)
    x = x.view(B, L, 3, D)
    q, kv, dout = x[:, -1, 0].contiguous(), x[:, :, 1:].reshape(B * L, 2 * D), do.view(B, L, D)[:, -1].contiguous()

    qd, kvd = q.double().requires_grad_(), kv.double().requires_grad_()
    k64, v64 = kvd[:, :D].view(B, L, H, Dh), kvd[:, D:].view(B, L, H, Dh)
    p_ref = torch.softmax(torch.einsum("bhd,blhd->bhl", qd.view(B, H, Dh), k64) * scale, dim=-1)
    o_ref = torch.einsum("bhl,blhd->bhd", p_ref, v64).reshape(B, D)
    o_ref.backward(dout.double())

    q_d, kv_d, do_d = (a.to(dev).to(dtype) for a in (q, kv, dout))
    o = torch.full_like(q_d, float("nan"))
    p = torch.full((B, H, L), float("nan"), device=dev, dtype=torch.float32)
    dq, dkv = torch.full_like(q_d, float("nan")), torch.full_like(kv_d, float("nan"))
    _lib.route_reset()
    check(lib.meant_temporal_attn_fwd(_p(q_d), _p(kv_d), _p(o), _p(p), B, L, H, Dh, scale, _dt(q_d), _stream()), "temporal_attn_fwd")
    check(lib.meant_temporal_attn_bwd(_p(q_d), _p(kv_d), _p(p), _p(do_d), _p(dq), _p(dkv), B, L, H, Dh, scale, _dt(q_d), _stream()), "temporal_attn_bwd")
    torch.cuda.synchronize()
    route = ("temporal_long_" if L > 64 else "temporal_short_") + IDS[DTYPES.index(dtype)]
    what = f"{route} {regime} L={L}"
    assert _lib.route_count("temporal_long") == (2 if L > 64 else 0), f"{what}: temporal_long {_lib.route_count('temporal_long')}"
    o, p, dq, dkv = (a.double().cpu() for a in (o, p, dq, dkv))
    assert not any(torch.isnan(a).any() for a in (o, p, dq, dkv)), f"{what}: unwritten output"
    assert torch.isfinite(dq).all(), f"{what}: dq not finite"
    tol = TOL[dtype]
    keep = ~carrier_columns(H, Dh) if is_carrier(regime) else torch.ones(D, dtype=torch.bool)
    grads = {"dq": (dq[:, keep], qd.grad[:, keep]), "dk": (dkv[:, :D], kvd.grad[:, :D]), "dv": (dkv[:, D:], kvd.grad[:, D:])}
    gmax = max(qd.grad[:, keep].abs().max().item(), kvd.grad.abs().max().item())
    gnorm = (qd.grad[:, keep].norm() ** 2 + kvd.grad.norm() ** 2).sqrt().item()
    fig = {"o": _rel(o, o_ref.detach()), "p": (p - p_ref.detach()).abs().max().item()}
    for name, (a, b) in grads.items():
        fig[name] = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-3 * gmax)
        fig[name + "_norm"] = abs(a.norm().item() - b.norm().item()) / max(b.norm().item(), 1e-3 * gnorm)
    _report(route, regime, fig)
    assert fig["o"] <= tol["out"], f"{what}: o {fig['o']:.2e}"
    assert fig["p"] <= tol["out"], f"{what}: p {fig['p']:.2e}"
    for name in grads:
        assert fig[name] <= tol["gelem"], f"{what}: {name} {fig[name]:.2e}"
        assert fig[name + "_norm"] <= tol["gnorm"], f"{what}: {name} norm off by {fig[name + '_norm']:.2e}"
