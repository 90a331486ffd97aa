"""Do the checks of test_gpu_loss_regimes.py bite?  The float32 host emulation of the hard-label softmax cross-entropy kernels
(loss_ref.emulate: 256 threads over 8-column chunks and the ragged tail, each with an online (max, sum) pair that a -inf column
leaves alone, the pair merge over lanes and waves, row_loss = log S + (M - x_t), softmax = exp((x - M) - log S)) goes through
loss_ref.check against float64 in every regime of loss_ref.regime_inputs and both tiers, and must pass.  With each defect such a
kernel can have it must be rejected in the regime named next to the defect, by at least 4 x the gate (a value that is not finite, or
a structural zero that is not zero, counts as infinitely far).  The two defects the kernels had -- logsumexp handed to the backward
in ONE float, and no -inf guard in a thread's online update -- PASS on `plain` rows, the inputs of the older test: the reason the
regimes exist.  The gates themselves are recomputed from the emulation here.  No GPU."""
import functools
import math

import pytest
import torch

from tests import loss_ref as L

TIERS = ("f32", "bf16")
T, SEED, FACTOR = 5, 5, 4.0
VS = (12, 2059)                                      # a tail column in a thread with no chunk / thread 0's second chunk and a tail
POISON = float("nan")
HOSTS = 1.25                                         # two hosts differed by 11 % in a worst figure: their exp and log round differently

# defect -> the (regime, tier) in which check must reject it
DEFECTS = {
    "lse_one_float": [("shifted+30000", "f32"), ("shifted+1000", "f32"), ("shifted-1000", "f32")],
    "no_inf_guard": [("masked", "f32"), ("masked", "bf16")],
    "lost_chunk": [("peaked", "f32"), ("peaked", "bf16")],
    "lost_tail": [("peaked", "f32"), ("peaked", "bf16")],
    "lost_wave": [("peaked", "f32"), ("peaked", "bf16")],
    "reads_padding": [("plain", "f32"), ("wide", "bf16")],
    "target_off_by_one": [(r, tier) for tier in TIERS for r in L.regimes(tier) if r != "uniform"],
    "ignored_not_zero": [("garbage_ignored", "f32"), ("garbage_ignored", "bf16")],
    "gscale_dropped": [("plain", "f32"), ("peaked", "bf16"), ("masked", "f32")],
    "padding_not_zeroed": [("plain", "f32"), ("uniform", "bf16"), ("garbage_ignored", "f32")],
}
assert set(DEFECTS) == set(L.DEFECTS)


@functools.lru_cache(maxsize=None)
def _case(regime, V, tier, pad=POISON, gscale=None):
    """inputs and float64 reference of one case, shared and never written to; `peaked` has one row per peak position"""
    rows = len(L.peak_positions(V)) if regime == "peaked" else T
    t = L.regime_inputs(regime, rows, V, L.ceil8(V) + 256, SEED, tier, gscale=gscale, pad=pad)
    return t, L.reference(t)


def _worst_over_gate(fig, tier):
    return max((float("inf") if v > 0 else 0.0) if L.GATES[tier][k] == 0 else v / L.GATES[tier][k] for k, v in fig.items())


@pytest.mark.parametrize("tier", TIERS)
def test_reference_is_finite_and_targets_are_never_masked(tier):
    for regime in L.regimes(tier):
        for V in L.GATE_VS:
            t, ref = _case(regime, V, tier)
            for name in ("row_loss", "lse", "mean", "dlogits"):
                assert bool(torch.isfinite(ref[name]).all()), (regime, V, name)
            cnt = ref["counted"]
            xt = t["logits"][cnt].gather(1, t["targets"][cnt][:, None])
            assert bool((xt > -1e8).all()), (regime, V)
            assert bool((ref["dlogits"][~cnt] == 0).all()) and bool((ref["dlogits"][:, V:] == 0).all())
            assert bool((ref["row_loss"][~cnt] == 0).all())


@pytest.mark.parametrize("tier", TIERS)
def test_regimes_hold_what_they_promise(tier):
    V = 2059
    t, ref = _case("uniform", V, tier)
    cnt = ref["counted"]
    assert torch.allclose(ref["row_loss"][cnt], torch.full((int(cnt.sum()),), math.log(V), dtype=torch.float64), rtol=1e-12, atol=0)
    t, ref = _case("peaked", V, tier)
    assert t["logits"].shape[0] == V // 8 + 7 + V % 8
    cols = set(t["logits"][:, :V].argmax(1).tolist())
    assert cols == set(L.peak_positions(V))                            # every chunk start, lane and tail column carries the peak once
    on = ref["row_loss"][ref["counted"]]
    assert bool(((on < 1e-3) | (on > 35)).all()) and bool((on < 1e-3).any()) and bool((on > 35).any())
    t, _ = _case("masked", V, tier)
    x = t["logits"][:, :V]
    assert bool(torch.isinf(x[:, :8]).all(1).any()) and bool(torch.isinf(x[:, 8 * (V >> 3):]).all(1).any())
    assert bool((torch.isfinite(x).sum(1) == 2).any())
    t, ref = _case("garbage_ignored", V, tier)
    assert bool(torch.isnan(t["logits"][~ref["counted"]]).any()) and int(ref["counted"].sum()) >= 2
    # the bad targets of the last rows walk through every kind over the V of the GPU tests
    kinds = set()
    for v in L.GATE_VS:
        last = int(_case("plain", v, tier)[0]["targets"][-1])
        kinds.add({v: "V", L.ceil8(v) + 255: "ld - 1"}.get(last, last))
    assert kinds == {-100, "V", "ld - 1", -1, 2 ** 31 + 3}, kinds


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("V", L.GATE_VS)
def test_emulation_passes(V, tier):
    for regime in L.regimes(tier):
        for pad in (POISON, 1e30):
            t, ref = _case(regime, V, tier, pad)
            fig = L.check(L.emulate(t), ref, t, f"{regime} V={V} {tier}")
        print(f"{regime} V={V} {tier}: " + " ".join(f"{k}={v:.1e}" for k, v in fig.items()))


@pytest.mark.parametrize("tier", TIERS)
def test_gates_are_four_times_the_emulations_worst(tier):
    """GATES holds 4 x the worst figure rounded up; a host whose exp / log round differently may move the worst a little, so the
    gate has to lie within [4 x / HOSTS, 8 x] of what is measured here"""
    worst = L.emulation_worst(tier)
    print(tier, {k: f"{v:.3e}" for k, v in worst.items()})
    for k, gate in L.GATES[tier].items():
        if k == "zeros":
            assert gate == 0.0 and worst[k] == 0.0
        else:
            assert 4 * worst[k] <= gate * HOSTS and gate <= 8 * worst[k], (k, worst[k], gate)


def test_ce_probs_gates_are_four_times_the_emulations_worst():
    worst = {}
    for kind in L.CE_PROBS_KINDS:
        for B, C in L.CE_PROBS_SHAPES:
            for seed in range(5):
                p, tg = L.ce_probs_inputs(kind, B, C, seed)
                fig = L.ce_probs_errors(*L.emulate_ce_probs(p, tg), *L.ce_probs_reference(p, tg))
                for k, v in fig.items():
                    worst[k] = max(worst.get(k, 0.0), v)
    print({k: f"{v:.3e}" for k, v in worst.items()})
    for k, gate in L.CE_PROBS_GATES.items():
        assert 4 * worst[k] <= gate * HOSTS and gate <= 8 * worst[k], (k, worst[k], gate)


def test_ce_probs_one_float_form():
    """max + log sum in one float, the form ce_probs_kernel keeps: inside the gates on probabilities; on rand + 1000 outside them
    (why that kind is not held to them) and inside gate + 2^-15, half an ulp of the float near 1008"""
    shifted = {}
    for kind in L.CE_PROBS_KINDS:
        for B, C in L.CE_PROBS_SHAPES:
            p, tg = L.ce_probs_inputs(kind, B, C, SEED)
            got, ref = L.emulate_ce_probs(p, tg, one_float=True), L.ce_probs_reference(p, tg)
            if kind != "shifted":
                L.ce_probs_check(*got, *ref, f"one float, {kind} [{B}, {C}]")
                continue
            fig = L.ce_probs_check(*got, *ref, f"one float, {kind} [{B}, {C}]", {k: v + 2.0 ** -15 for k, v in L.CE_PROBS_GATES.items()})
            for k, v in fig.items():
                shifted[k] = max(shifted.get(k, 0.0), v)
    print({k: f"{v:.3e}" for k, v in shifted.items()})
    assert all(shifted[k] > 3 * L.CE_PROBS_GATES[k] for k in shifted), shifted


def _rejections():
    return [(d, r, tier, V) for d, where in DEFECTS.items() for r, tier in where for V in VS]


@pytest.mark.parametrize("defect,regime,tier,V", _rejections())
def test_defect_is_rejected(defect, regime, tier, V):
    if defect == "lost_wave" and V < 8 * 129:
        V = 2049                                     # wave 2 has to hold something
    gscale = {"gscale_dropped": -3.0 if regime != "peaked" else 1.0 / 7.0}.get(defect)
    t, ref = _case(regime, V, tier, POISON, gscale)
    fig = L.errors(L.emulate(t, defect), ref, t)
    worst = _worst_over_gate(fig, tier)
    print(f"{defect} {regime} {tier} V={V}: worst figure / gate {worst:.3g}  " + " ".join(f"{k}={v:.1e}" for k, v in fig.items()))
    assert worst >= FACTOR, f"{defect} in {regime} ({tier}, V={V}): only {worst:.2f} x the gate"
    with pytest.raises(AssertionError):
        L.check(L.emulate(t, defect), ref, t, f"{defect} {regime} {tier}")


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("defect", ["lse_one_float", "no_inf_guard"])
def test_the_kernels_two_defects_pass_on_plain_rows(defect, tier):
    """randn * 3: the row maximum is about 12, so M + log S in one float costs 1e-6 at the most, and nothing is -inf"""
    for V in L.GATE_VS:
        t, ref = _case("plain", V, tier)
        L.check(L.emulate(t, defect), ref, t, f"{defect} plain V={V} {tier}")


def test_where_the_unguarded_update_turns_a_row_into_nan():
    """a thread whose first 8-column chunk is all -inf keeps s = NaN from (-inf) - (-inf); the merge over lanes drops the pair of a
    thread whose maximum stayed -inf, so the NaN reaches the row exactly where that thread goes on to a finite column: a second chunk
    (V >= 2056 for thread 0), or a tail column behind its chunk (V = 12: column 8).  A thread with nothing but the masked chunk
    (V = 2048), or with one masked tail column and no chunk (x[0] at V = 5, x[9] at V = 12), is dropped whole and the row is right.
    The guarded form is right in all of them."""
    for V, cols, nan in ((4101, range(8), True), (2056, range(8), True), (12, range(8), True), (2048, range(8), False), (5, [0], False),
                         (12, [9], False)):
        t = L.regime_inputs("plain", 1, V, L.ceil8(V), 0, "f32")
        t["logits"][0, list(cols)] = L.NEG_INF
        t["targets"][0] = V - 1
        ref = L.reference(t)
        assert bool(torch.isnan(L.emulate(t, "no_inf_guard")["row_loss"]).any()) == nan, (V, list(cols))
        L.check(L.emulate(t), ref, t, f"V={V}")
