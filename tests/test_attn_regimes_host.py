"""Do the checks of test_gpu_attn_regimes.py bite?  A pure-torch emulation of the bf16 flash forward and backward (64-key tiles with
a running maximum, P rounded to bf16 before P V, o rounded to bf16, delta from the rounded o, dS rounded to bf16) goes through
attn_ref._check against the float64 reference in the five input regimes of attn_ref.regime_inputs.  The emulation as it stands
must pass everywhere; with each of five defects a flash kernel can have, it must fail in the regime named next to the defect.
No GPU."""
import numpy as np
import pytest
import torch

from tests.attn_ref import KV_TILE, LOG2E, REGIMES, _check, _mask, _reference, carrier_columns, is_carrier, regime_inputs

G, S, H, DH = 2, 320, 2, 64
SEED = 11

# defect -> the regime in which _check must reject it
MUTATIONS = {
    "no_rescale": "rising",         # (a) O and l are not rescaled when the running maximum moves
    "no_max": "offset+",            # (b) P = exp2(t) instead of exp2(t - m): overflow at +144, 0 / 0 at -144
    "raw_tile_max": "offset-",      # (c) the tile maximum of a tile without masked keys is taken from the scores before c1 = scale log2(e)
    "no_delta": "sharp",            # (d) dS = P dP instead of P (dP - delta)
    "last_tile_max": "falling",     # (e) the stored m is the last tile's maximum instead of the row's
}


def _bf(x):
    return x.bfloat16().float()


def flash_emulation(qkv, do, mask, G, S, H, Dh, scale, causal, mutation=None):
    """o bf16 [G*S, H*Dh], the pair (m, log2 l) float [G, H, S, 2] and dqkv bf16 [G*S, 3*H*Dh], in float32 arithmetic"""
    assert mutation is None or mutation in MUTATIONS
    D = H * Dh
    x = qkv.float().view(G, S, 3, H, Dh)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))                  # [G, H, S, Dh]
    dout = do.float().view(G, S, H, Dh).transpose(1, 2)
    c1 = scale * LOG2E
    dead = torch.from_numpy(mask == 0) if mask is not None else torch.zeros(G, S, dtype=torch.bool)
    rows = torch.arange(S)

    def scores(t0, t1):
        """raw q k^T of a tile, its log2-domain scores with the padding and causal terms, and per (group, row) whether the tile is
        free of both"""
        raw = q @ k[:, :, t0:t1].transpose(-1, -2)
        t = raw * c1
        t = torch.where(dead[:, None, None, t0:t1], torch.full_like(t, -1e9 * LOG2E), t)
        hidden = rows[t0:t1][None, :] > rows[:, None] if causal else torch.zeros(S, t1 - t0, dtype=torch.bool)
        t = t.masked_fill(hidden, float("-inf"))
        plain = ~dead[:, t0:t1].any(dim=1)[:, None, None] & ~hidden.any(dim=1)[None, None, :]        # [G, 1, S]
        return raw, t, plain

    m = torch.full((G, H, S), float("-inf"))
    l = torch.zeros(G, H, S)
    acc = torch.zeros(G, H, S, Dh)
    m_tile = m
    for t0 in range(0, S, KV_TILE):
        t1 = min(S, t0 + KV_TILE)
        raw, t, plain = scores(t0, t1)
        m_tile = t.amax(dim=-1)
        if mutation == "raw_tile_max":
            m_tile = torch.where(plain, raw.amax(dim=-1), m_tile)
        m_new = torch.maximum(m, m_tile)
        alpha = torch.ones_like(m) if mutation in ("no_rescale", "no_max") else torch.exp2(m - m_new)
        p = torch.exp2(t) if mutation == "no_max" else torch.exp2(t - m_new[..., None])
        l = l * alpha + p.sum(-1)
        acc = acc * alpha[..., None] + _bf(p) @ v[:, :, t0:t1]
        m = m_new
    o = _bf(acc / l[..., None])
    logl = torch.log2(l) - m if mutation == "no_max" else torch.log2(l)        # no_max: l holds sum exp2(t), the same pair while nothing overflows
    m_st = m_tile if mutation == "last_tile_max" else m
    lse = torch.stack([m_st, logl], dim=-1)

    delta = (dout * o).sum(-1)                                                   # from the rounded o, as the kernels take it
    dq = torch.zeros(G, H, S, Dh)
    dk = torch.zeros(G, H, S, Dh)
    dv = torch.zeros(G, H, S, Dh)
    for t0 in range(0, S, KV_TILE):
        t1 = min(S, t0 + KV_TILE)
        _, t, _ = scores(t0, t1)
        p = torch.exp2(t - (m_st + logl)[..., None])
        dp = dout @ v[:, :, t0:t1].transpose(-1, -2)
        ds = _bf(p * dp if mutation == "no_delta" else p * (dp - delta[..., None]))
        dq += scale * (ds @ k[:, :, t0:t1])
        dk[:, :, t0:t1] = scale * (ds.transpose(-1, -2) @ q)
        dv[:, :, t0:t1] = _bf(p).transpose(-1, -2) @ dout
    dqkv = torch.stack([g.transpose(1, 2) for g in (dq, dk, dv)], dim=2).reshape(G * S, 3 * D).bfloat16()
    return o.transpose(1, 2).reshape(G * S, D).bfloat16(), lse, dqkv


_CASES = {}


def _case(regime, causal):
    """inputs, mask and the float64 reference of one (regime, causal), computed once"""
    key = (regime, causal)
    if key not in _CASES:
        # one set of inputs for both values of causal, its regime asserted in the causal view: S = 320 is five full tiles, where
        # the non-causal `rising` mass outside the last tile is e^-2 + e^-4 + ... = 0.14 of the row, a hair under the 0.15 the helper
        # asks for (the causal rows, which end inside a tile, keep 0.3 - 0.4 outside it)
        qkv, do, scale = regime_inputs(G, S, H, DH, regime, SEED, causal=1)
        mask = _mask("suffix", G, S, np.random.RandomState(SEED))
        _CASES[key] = (qkv, do, scale, mask, _reference(qkv, do, mask, G, S, H, DH, scale, causal))
    return _CASES[key]


def _emulate_and_check(regime, causal, mutation):
    qkv, do, scale, mask, ref = _case(regime, causal)
    o, lse, dqkv = flash_emulation(qkv, do, mask, G, S, H, DH, scale, causal, mutation)
    skip = carrier_columns(H, DH) if is_carrier(regime) else None
    return _check(o, lse, dqkv, ref, H, DH, f"{regime} causal={causal} {mutation}", skip_dq=skip)


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("regime", REGIMES)
def test_emulation_passes(regime, causal):
    fig = _emulate_and_check(regime, causal, None)
    print(f"{regime} causal={causal}: " + " ".join(f"{k}={v:.1e}" for k, v in fig.items()))


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_mutation_is_rejected(mutation, causal):
    with pytest.raises(AssertionError):
        _emulate_and_check(MUTATIONS[mutation], causal, mutation)
