"""Do the checks of test_gpu_norm_regimes.py bite?  The float32 host emulation of the norm kernels' arithmetic (norm_ref.emulate_*:
the chunked sum of squares, r = 1 / (sqrt(ss) / sqrt(d) + eps), the backward with nsd = (1 / r - eps) d and its guard, the two-pass
LayerNorm, the fold's kcoef) goes through norm_ref.check against the float64 references in every input regime of
norm_ref.regime_inputs, in both tiers (the bf16 tier rounds y and dx to bf16).  The emulation as it stands must pass everywhere.
With each defect a norm kernel can have it must be rejected in the regime named next to the defect, by an error of at least
4 x the bound, so that no rejection hangs on a rounding.  And the eps and lost-chunk defects PASS on `unit` / randn rows, the
inputs of every other norm test: the reason the regimes exist.  No GPU."""
import functools

import pytest
import torch

from tests import norm_ref as N
from tests.util import DTYPES, IDS

D, ROWS = 768, 96                                    # rows = d / 8: every chunk position carries a spike once
D_PARTIAL, D_PART = 520, 260
D_FOLD = 128
SEED = 5
FACTOR = 4.0

# defect -> (family, the regimes in which check must reject it, the tiers)
DEFECTS = {
    "no_eps": ("rms", ("eps_heavy", "tiny"), IDS),
    "eps_in_sqrt": ("rms", ("eps_heavy", "tiny"), IDS),
    "bwd_no_eps": ("rms", ("eps_heavy", "tiny"), IDS),
    "fold_no_eps": ("fold", ("eps_heavy",), ["bf16"]),
    "lost_chunk": ("rms", ("spike",), IDS),
    "ln_one_pass": ("ln", ("shifted",), ["f32"]),
    "ln_eps_outside": ("ln", ("eps_heavy",), IDS),
    "no_guard": ("rms", ("zero",), IDS),
    "partial_all_columns": ("partial", ("tail",), IDS),
}
assert set(DEFECTS) == set(N.DEFECTS)
FAMILIES = {"rms": N.RMS_REGIMES, "ln": N.LN_REGIMES, "partial": N.PARTIAL_REGIMES, "fold": N.FOLD_REGIMES}


def _dtype(tier):
    return DTYPES[IDS.index(tier)]


@functools.lru_cache(maxsize=None)
def _case(family, regime, tier):
    """inputs and float64 reference of one (family, regime); the tier changes the inputs of `shifted` alone"""
    if family == "rms":
        t = N.regime_inputs(regime, ROWS, D, SEED, tier)
        return t, N.ref_rmsnorm(t), N.RMS_SPEC
    if family == "partial":
        t = N.regime_inputs(regime, ROWS, D_PARTIAL, SEED, tier, d_part=D_PART)
        return t, N.ref_rmsnorm(t, D_PART, with_offset=True), dict(N.RMS_SPEC, doffset=("tensor", "gelem"))
    if family == "ln":
        t = N.regime_inputs(regime, ROWS, D, SEED, tier, norm="ln")
        return t, N.ref_layernorm(t), N.LN_CONSTANT_SPEC if regime == "constant" else N.LN_SPEC
    t = N.regime_inputs(regime, ROWS, D_FOLD, SEED, tier)
    t["fold"] = N.fold_weights(D_FOLD, SEED)
    W, b, g3 = t["fold"]
    ref = N.evaluate(lambda x: {"y": N.fold64(x, t["gain"].double(), W.double(), b.double(), g3.double(), t["eps"], t["eps"])},
                     {"x": t["x"]}, {"y": t["dy"]})
    return t, ref, N.FOLD_SPEC


def _emulate(family, regime, tier, defect):
    t, ref, spec = _case(family, regime, tier)
    if family == "rms":
        got = N.emulate_rmsnorm(t, tier, defect=defect)
    elif family == "partial":
        got = N.emulate_rmsnorm(t, tier, D_PART, with_offset=True, defect=defect)
    elif family == "ln":
        got = N.emulate_layernorm(t, tier, defect)
    else:
        got = N.emulate_fold(t, *t["fold"], defect=defect)
    return got, ref, spec


def _cases():
    return [(f, r, tier) for f, regs in FAMILIES.items() for r in regs for tier in (IDS if f != "fold" else ["bf16"])]


@pytest.mark.parametrize("family,regime,tier", _cases())
def test_emulation_passes(family, regime, tier):
    got, ref, spec = _emulate(family, regime, tier, None)
    fig = N.check(got, ref, spec, _dtype(tier), f"{family} {regime} {tier}")
    print(f"{family} {regime} {tier}: " + " ".join(f"{k}={v:.1e}" for k, v in fig.items()))


def _rejections():
    return [(d, r, tier) for d, (_, regs, tiers) in DEFECTS.items() for r in regs for tier in tiers]


@pytest.mark.parametrize("defect,regime,tier", _rejections())
def test_defect_is_rejected(defect, regime, tier):
    """by at least FACTOR x the bound in one compared tensor (a non-finite one counts as infinite), and so by check itself"""
    family = DEFECTS[defect][0]
    got, ref, spec = _emulate(family, regime, tier, defect)
    fig = N.errors(got, ref, spec)
    worst = max(fig[name] / N.bound(key, _dtype(tier)) for name, (_, key, *_f) in spec.items())
    print(f"{defect} {regime} {tier}: worst error / bound {worst:.1f}  " + " ".join(f"{k}={v:.1e}" for k, v in fig.items()))
    assert worst >= FACTOR, f"{defect} in {regime} ({tier}): only {worst:.2f} x the bound"
    with pytest.raises(AssertionError):
        N.check(got, ref, spec, _dtype(tier), f"{defect} {regime} {tier}")


@pytest.mark.parametrize("tier", IDS)
@pytest.mark.parametrize("defect", ["no_eps", "eps_in_sqrt", "bwd_no_eps"])
def test_eps_defects_pass_on_unit_rows(defect, tier):
    """eps = 1e-8 next to rms = 1 is below one float ulp: the inputs of every other norm test cannot see where eps sits"""
    got, ref, spec = _emulate("rms", "unit", tier, defect)
    N.check(got, ref, spec, _dtype(tier), f"{defect} unit {tier}")


def test_fold_defect_passes_on_unit_rows():
    got, ref, spec = _emulate("fold", "unit", "bf16", "fold_no_eps")
    N.check(got, ref, spec, torch.bfloat16, "fold_no_eps unit")


def test_lost_chunk_passes_the_bf16_output_bound_on_randn_rows():
    """a sum of squares that leaves out one 8-column chunk moves y by about 8 / (2 d) of a randn row: inside 4e-2"""
    got, ref, spec = _emulate("rms", "unit", "bf16", "lost_chunk")
    fig = N.errors(got, ref, spec)
    assert fig["y"] <= N.bound("out", torch.bfloat16), fig
    assert fig["y"] >= 1e-3, "the defect has to be there"
