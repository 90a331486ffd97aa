"""Shared helpers of the attention tests at the C ABI: key masks, the float64 references of the attention core and of the cls
query's attention, one forward + backward through meant_attn_fwd / _bwd on NaN-prefilled outputs, the comparison against the
reference, and the input regimes (peaked and shifted softmaxes) of test_gpu_attn_regimes.py / test_attn_regimes_host.py."""
import math

import numpy as np
import torch

from tests.util import TOL

F32, BF16 = 0, 1
LOG2E = 1.0 / math.log(2.0)
KV_TILE = 64                                         # keys per tile of the flash kernels


def _mask(kind, G, S, rs):
    m = np.ones((G, S), dtype=np.float32)
    if kind == "suffix":                             # trailing padding of random length per group
        for g in range(G):
            p = rs.randint(0, max(1, (3 * S) // 4))
            if p:
                m[g, S - p:] = 0
    elif kind == "holes":                            # padding in the middle: dead tiles between live ones at the longer S
        for g in range(G):
            a = rs.randint(1, max(2, S // 2)) if S > 1 else 0
            b = rs.randint(a, S) if a < S else S
            m[g, a:b] = 0
    elif kind == "dead_group":                       # group 0 has no live key at all, the others a random suffix
        m[0, :] = 0
        for g in range(1, G):
            p = rs.randint(0, max(1, S // 2))
            if p:
                m[g, S - p:] = 0
    return None if kind == "none" else m


def _rotate(x, a, b):
    """x [G, S, H, Dh] float64, tables [S, R] float64: the rotation in pairs y[2j] = a[2j] x[2j] - b[2j] x[2j+1],
    y[2j+1] = a[2j+1] x[2j+1] + b[2j+1] x[2j] on the first R lanes of every head"""
    R = a.shape[1]
    xr = x[..., :R]
    sw = torch.stack([-xr[..., 1::2], xr[..., 0::2]], dim=-1).reshape(xr.shape)      # (-x[2j+1], x[2j])
    y = xr * a[None, :, None, :] + sw * b[None, :, None, :]
    return torch.cat([y, x[..., R:]], dim=-1)


def _reference(qkv, do, mask, G, S, H, Dh, scale, causal, tables=None, natural=False):
    """float64 on the host: o, the pair (m, log l) per (g, h, query) -- in the log2 domain as the bf16 tier keeps it, in natural-log
    units (natural=True) as the f32 tier and the fp32 detour do --, and dqkv.  Masked keys get the additive -1e9
    with the score itself absorbed (as the fp32 sum s - 1e9 does in the reference); the score's gradient passes through unchanged.
    With tables, qkv holds the rotated q / k and the gradient is taken through the rotation back to the unrotated inputs."""
    D = H * Dh
    x = qkv.double().cpu().view(G, S, 3, H, Dh)
    if tables is not None:
        qa, qb, ka, kb = (a.double() for a in tables)
        # unrotated inputs whose rotation equals the bf16 inputs exactly in value: rotate -> attention -> adjoint
        x0 = x.clone().requires_grad_()
        q = _rotate(x0[:, :, 0], qa, qb)
        k = _rotate(x0[:, :, 1], ka, kb)
        q = q + (x[:, :, 0] - q).detach()
        k = k + (x[:, :, 1] - k).detach()
        v = x0[:, :, 2]
        leaf = x0
    else:
        leaf = x.clone().requires_grad_()
        q, k, v = leaf[:, :, 0], leaf[:, :, 1], leaf[:, :, 2]
    q, k, v = (a.transpose(1, 2) for a in (q, k, v))                                   # [G, H, S, Dh]
    s = (q @ k.transpose(-1, -2)) * scale
    if mask is not None:
        dead = torch.from_numpy(mask == 0)[:, None, None, :].expand_as(s)
        s = torch.where(dead, s - s.detach() - 1e9, s)
    if causal:
        s = s.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
    if natural:
        m = s.detach().amax(dim=-1)
        logl = torch.log(torch.exp(s.detach() - m[..., None]).sum(-1))
    else:
        t2 = s.detach() * LOG2E
        m = t2.amax(dim=-1)
        logl = torch.log2(torch.exp2(t2 - m[..., None]).sum(-1))
    o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(G * S, D)
    o.backward(do.double().cpu())
    return o.detach(), torch.stack([m, logl], dim=-1), leaf.grad.reshape(G * S, 3 * D)


def _run(qkv, do, mask, G, S, H, Dh, scale, causal, tables=None, route_names=None, dtype=torch.bfloat16):
    """one meant_attn_fwd and one meant_attn_bwd on qkv / do (device tensors of `dtype`), the route counters reset before the pair.
    Every output starts as NaN.  lse comes back as the tier keeps it: log2 units in bf16, natural-log units in f32."""
    from meant_amd import _lib
    from meant_amd._lib import lib, check
    assert qkv.dtype == dtype and do.dtype == dtype
    code = BF16 if dtype == torch.bfloat16 else F32
    D, st = H * Dh, torch.cuda.current_stream().cuda_stream
    o = torch.full((G * S, D), float("nan"), device=qkv.device, dtype=dtype)
    lse = torch.full((G, H, S, 2), float("nan"), device=qkv.device)
    wsb = lib.meant_attn_ws(G, S, H, Dh, code)
    ws = torch.empty(max(wsb, 16), device=qkv.device, dtype=torch.uint8)
    km = torch.from_numpy(mask).to(qkv.device) if mask is not None else None
    mp = km.data_ptr() if km is not None else None
    tp = [a.to(qkv.device) for a in tables] if tables is not None else None
    pp = [a.data_ptr() for a in tp] if tp is not None else [None] * 4
    R = tables[0].shape[1] if tables is not None else 0
    _lib.route_reset()
    check(lib.meant_attn_fwd(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), mp, G, S, H, Dh, scale, causal, code, ws.data_ptr(), wsb, st), "attn_fwd")
    dqkv = torch.full_like(qkv, float("nan"))
    check(lib.meant_attn_bwd(qkv.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), mp, dqkv.data_ptr(), G, S, H, Dh, scale, causal,
                             pp[0], pp[1], pp[2], pp[3], R, code, ws.data_ptr(), wsb, st), "attn_bwd")
    torch.cuda.synchronize()
    routes = {r: _lib.route_count(r) for r in route_names or (f"attn_fwd_d{Dh}", f"attn_bwd_d{Dh}", "attn_generic", "attn_short", "attn_bwd1")}
    return o, lse, dqkv, routes


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-12)


def _errors(o, lse, dqkv, ref, H, Dh, skip_dq=None):
    """the figures _check holds against its bounds: o relative to the reference's largest value, both halves of the statistics
    pair, and per gradient block the element error and the norm difference (each relative, over the floors of _check)"""
    o_r, st_r, g_r = ref
    D = H * Dh
    st = lse.double().cpu()
    fig = {"o": _rel(o, o_r),
           "m": ((st[..., 0] - st_r[..., 0]).abs() - 1e-6 * st_r[..., 0].abs()).max().item(),   # m ~ -1.4e9 on fully padded rows: fp32 resolution
           "l": (st[..., 1] - st_r[..., 1]).abs().max().item()}
    # dQ and dK are structurally zero at S = 1 (one key: the softmax is constant): errors are taken against a floor of 1e-3 of the
    # whole gradient's scale, where both sides hold rounding noise
    gmax, gnorm = g_r.abs().max().item(), g_r.norm().item()
    for name, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D))):
        a, b = dqkv[:, sl].double().cpu(), g_r[:, sl]
        if name == "dq" and skip_dq is not None:
            a, b = a[:, ~skip_dq], b[:, ~skip_dq]
        fig[name] = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-3 * gmax)
        nb = b.norm().item()
        fig[name + "_norm"] = abs(a.norm().item() - nb) / max(nb, 1e-3 * gnorm)
    return fig


def _check(o, lse, dqkv, ref, H, Dh, what, tol=None, skip_dq=None):
    """tol: a tier's dict of tests.util.TOL (bf16 when not given).  skip_dq: bool [H * Dh], the dq columns left out of the element
    and norm comparisons; they must still be finite.  Returns the figures of _errors."""
    tol = TOL[torch.bfloat16] if tol is None else tol
    assert not torch.isnan(o).any() and not torch.isnan(lse).any() and not torch.isnan(dqkv).any(), f"{what}: unwritten output"
    if skip_dq is not None:
        assert torch.isfinite(dqkv[:, :H * Dh].float()).all(), f"{what}: dq not finite"
    fig = _errors(o, lse, dqkv, ref, H, Dh, skip_dq)
    assert fig["o"] <= tol["out"], f"{what}: o {fig['o']:.2e}"
    assert fig["m"] <= 1e-3, f"{what}: m off by {fig['m']:.2e}"
    assert fig["l"] <= 1e-3, f"{what}: log l off by {fig['l']:.2e}"
    for name in ("dq", "dk", "dv"):
        assert fig[name] <= tol["gelem"], f"{what}: {name} {fig[name]:.2e}"
        assert fig[name + "_norm"] <= tol["gnorm"], f"{what}: {name} norm off by {fig[name + '_norm']:.2e} of the reference's"
    return fig


# ------------------------------------------------------------------------------------------------------------------------------
# the cls query's attention (meant_attn_cls_fwd / _bwd and the split pair)
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
    contract, as in every flash backward): ds = p (dout . v - delta), dq0 = scale ds K, dK = scale ds q0, dV = p dout; a masked
    key has no score gradient.  With the exact output this is the autograd gradient (checked by the caller)."""
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


# ------------------------------------------------------------------------------------------------------------------------------
# input regimes: softmaxes that are peaked, whose maximum moves from key tile to key tile, or whose scores sit far from zero
REGIMES = ("sharp", "rising", "falling", "offset+", "offset-")
CARRIER = 8.0                                        # lane 0 of every query head in the carrier regimes


def is_carrier(regime):
    return regime != "sharp"


def carrier_columns(H, Dh):
    """bool [H * Dh]: lane 0 of every head, the dq columns the carrier regimes leave out of the comparison.  Lane 0 of dq is
    scale * sum_j dS_j k_j0 with k_j0 the carrier, up to ~140: exactly 0 where the carrier is constant over j (sum_j dS_j = 0), and a
    sum of cancelling terms times a large factor in any case, so the bf16 rounding of dS makes it noise in a correct kernel."""
    c = torch.zeros(H, Dh, dtype=torch.bool)
    c[:, 0] = True
    return c.view(-1)


def _slope(S):
    return max(2.0 / KV_TILE, 6.0 / S)


def regime_inputs(G, S, H, Dh, regime, seed, causal=0):
    """bf16-exact float32 qkv [G*S, 3*H*Dh] and do [G*S, H*Dh] on the host, and scale = 1/sqrt(H*Dh).
      sharp    q and k of randn scaled so that the scores have a standard deviation of 6
      rising   score(i, j) = slope * j + unit noise, slope = max(2/64, 6/S): the row maximum moves up in every 64-key tile while the
               earlier tiles keep a sizeable share of the mass
      falling  score(i, j) = -slope * j + unit noise: the first tile sets the maximum, the later ones still carry mass
      offset+  score = +100 + unit noise, offset- score = -100 + unit noise (+-144 in log2 units)
    The last four put the score on a carrier: lane 0 of every q head is CARRIER, lane 0 of key j is target(j) / (scale * CARRIER),
    the other lanes are scaled to give noise of standard deviation 1.  The regime is asserted on the float64 scores of group 0
    without a key mask (under the causal mask where the case that uses the inputs has one: `causal` changes nothing else), so that
    another seed or shape cannot quietly give a flat softmax."""
    assert regime in REGIMES, regime
    scale = 1.0 / math.sqrt(H * Dh)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(G, S, 3, H, Dh, generator=gen)
    do = torch.randn(G * S, H * Dh, generator=gen).bfloat16().float()
    if regime == "sharp":
        x[:, :, :2] *= math.sqrt(6.0 / (scale * math.sqrt(Dh)))
    else:
        j = torch.arange(S, dtype=torch.float32)
        target = {"rising": _slope(S) * j, "falling": -_slope(S) * j, "offset+": torch.full((S,), 100.0), "offset-": torch.full((S,), -100.0)}[regime]
        x[:, :, :2, :, 1:] *= math.sqrt(1.0 / (scale * math.sqrt(Dh - 1)))
        x[:, :, 0, :, 0] = CARRIER
        x[:, :, 1, :, 0] = (target / (scale * CARRIER))[None, :, None]
    x = x.bfloat16().float()
    _assert_regime(x[0].double(), S, scale, regime, causal)
    return x.view(G * S, 3 * H * Dh), do, scale


def _assert_regime(x, S, scale, regime, causal):
    """x [S, 3, H, Dh] float64: one group's inputs"""
    s = torch.einsum("ihd,jhd->hij", x[:, 0], x[:, 1]) * scale          # [H, S, S]
    if causal:
        s = s.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
    p = torch.softmax(s, dim=-1)
    tile = torch.arange(S) // KV_TILE
    arg = s.argmax(dim=-1)                                                # [H, S]
    outside = (p * (tile[None, None, :] != tile[arg][..., None])).sum(-1)  # mass outside the 64-key tile of the row's largest score
    if regime == "sharp":
        top = p.amax(dim=-1).median().item()
        assert top >= 0.5, f"sharp: median largest probability {top:.2f}"
    elif regime == "rising":
        if S >= 128:                                 # the last row's largest score among the last 64 keys
            assert (arg[:, -1] >= S - KV_TILE).all(), f"rising: last row's argmax {arg[:, -1].tolist()} of {S}"
            assert outside.median().item() >= 0.15, f"rising: median mass outside the argmax's tile {outside.median().item():.2f}"
    elif regime == "falling":
        # unit noise on a slope of 2 per tile puts the largest score of a row into tile 1 about once in 200 rows: nearly all, not all
        first = (arg < KV_TILE).double().mean().item()
        assert first >= 0.95, f"falling: the largest score lies in tile 0 in {first:.3f} of the rows"
        if S >= 128:
            assert outside.median().item() >= 0.05, f"falling: median mass outside tile 0 {outside.median().item():.2f}"
    else:
        fin = s[torch.isfinite(s)]
        lo, hi = fin.abs().min().item(), fin.abs().max().item()
        assert 90.0 <= lo and hi <= 110.0 and (fin > 0).all().item() == (regime == "offset+"), f"{regime}: |score| in [{lo:.1f}, {hi:.1f}]"
