"""The norm kernels under eps-visible, scaled, spiked and shifted inputs, through meant_amd.ops (autograd drives forward and backward)
against float64 on the same inputs.

Every other norm test feeds randn rows (rms = 1) at eps = 1e-8, where the eps term is below one float ulp, and the exact tests
(test_gpu_norm_exact.py) SUPPLY the statistics to the backward.  Here the inputs come from norm_ref.regime_inputs: `eps_heavy` and
`tiny` make the place of eps visible, forward and backward; `vanishing`, `large` and `zero` put the statistics at the ends of the
float range and on the `nsd > 0` / `den > 0` guards; `spike` lets every 8-column chunk position carry a whole row's energy once, so a
reduction over lanes, chunks, waves or slices that loses one is off by a factor of 1000; `shifted` and `constant` ask LayerNorm for a
variance about the mean; `tail` asks the partial RMSNorm to ignore the columns past d_part.  tests/test_norm_regimes_host.py shows on
the host that the comparison used here (norm_ref.check: row-normalised errors within tests.util.TOL, everything finite) rejects a
kernel with eps dropped, inside the square root or missing from the backward's norm or the fold's kcoef, a lost chunk, a one-pass
variance, eps outside LayerNorm's square root, a missing guard and statistics over the wrong columns -- and that the randn rows of
the other tests accept most of them.

Shapes are the smallest at which each kernel family exists: the tables of test_gpu_norm_exact.py, whose mirror of the launch rule
(norm_route) is asserted, so that each case provably sits on the family it names.  Dropout stays at p = 0 and the ops allocate
their outputs as usual.  The reference runs in torch float64 on the device (the Linear in front of a d = 8200 norm is 8200 x 8200).

  one row per wave   ops.rmsnorm, rmsnorm_fork (dres), linear_gelu_rmsnorm (gelu_pre): d = 8, 520, 2048, and 768 at an odd row count
  packed             the same at (d, R) = (128, 4), (512, 1), (1024, 1), (768, 2)
  wide / odd         the same with any_width=True at d = 100, 2056, 8200 (two slices), 3
  partial + bias     ops.rmsnorm_partial at (d, d_part) = (520, 260), (100, 50)
  pooled             linear_gelu_rmsnorm_pooled, rmsnorm_fork_pooled at d = 128, 768, groups of 8 rows
  folded (bf16)      norm_linear_gelu_norm and its pooled form at d = 128, eps0 and eps3 both the regime's
  LayerNorm          ops.layernorm at d = 768 (one row per wave), 100 and 4100 (wide)

The Linear in front of a norm is the identity with a zero bias (both still parameters with compared gradients), so that the norm's
input is gelu of the regime's rows: zero rows stay zero, the spike stays sqrt(d), a positive element of `large` stays 2^50 z.
The worst error every route reached in every regime on an MI355X is in profiles/norm_regimes_errors.txt.

Rows beyond `large` (a sum of squares that overflows float32) are undefined by include/meant_hip.h and not tested."""
import functools

import pytest
import torch

from tests import norm_ref as N
from tests.test_gpu_norm_exact import PACKED, norm_route
from tests.util import DTYPES, IDS

pytestmark = pytest.mark.gpu
SEED = 5
ROWS = 12
ROW_SHAPES = [(8, ROWS), (520, ROWS), (2048, ROWS), (768, 7)]          # (d, rows): 768 at an odd row count cannot pack
WIDE_SHAPES = [(100, ROWS), (2056, ROWS), (8200, ROWS), (3, ROWS)]
PARTIAL_SHAPES = [(520, 260), (100, 50)]
PARTIAL_ROWS = 13
POOLED_D, GROUP_ROWS, NGROUPS = [128, 768], 8, 3
FOLD_D, FOLD_S = 128, 24
LN_SHAPES = [(768, "row"), (100, "wide"), (4100, "wide")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rows_for(regime, d, rows, multiple=1, odd=False):
    """`spike` needs ceil(d / 8) rows, rounded up to the family's row multiple (and kept odd where the case is about an odd count)"""
    if regime == "spike":
        rows = max(rows, -(-d // 8))
        rows = -(-rows // multiple) * multiple
        if odd and rows % 2 == 0:
            rows += 1
    return rows


@functools.lru_cache(maxsize=4)
def _inputs(regime, rows, d, tier, norm="rms", d_part=None):
    """the regime's tensors plus the cotangents of the second outputs: dres [rows, d] on the scale of the row's dx (r, so that it
    is visible next to the norm's own gradient in every regime) and one bf16-exact vector per GROUP_ROWS / FOLD_S rows"""
    t = N.regime_inputs(regime, rows, d, SEED, tier, norm, d_part)
    gen = torch.Generator().manual_seed(SEED + 1)
    r = N.rinv64(t["x"], t["eps"]).float()
    t["dres"] = (0.5 * torch.randn(rows, d, generator=gen) * r[:, None]).bfloat16().float()
    return t


def _report(route, regime, tier, fig):
    print(f"norm-regime-errors route={route} regime={regime} tier={tier} " + " ".join(f"{k}={v:.2e}" for k, v in fig.items()))


def _compare(dev, dtype, route, regime, fwd_gpu, fwd_ref, leaves, cots, spec, act=("x",)):
    """one forward + backward through the ops on the device, the same through float64, norm_ref.check"""
    tier = IDS[DTYPES.index(dtype)]
    got = N.evaluate(fwd_gpu, leaves, cots, prep=lambda name, v: v.to(dev).to(dtype) if name in act else v.to(dev).float())
    torch.cuda.synchronize()
    ref = N.evaluate(fwd_ref, leaves, cots, device=dev)
    fig = N.check(got, ref, spec, dtype, f"{route} {regime} {tier}")
    _report(route, regime, tier, fig)


def _saved(y, i):
    """the i-th tensor the op saved for its backward (the statistics the kernel computed)"""
    return y.grad_fn.saved_tensors[i]


# ------------------------------------------------------------------------------------------------------------------------------
# 1. ops.rmsnorm, rmsnorm_fork, linear_gelu_rmsnorm on the three kernel families
GAIN_SPEC = {"dgain": ("tensor", "gelem")}
PLAIN_SPEC = dict({"y": ("rows", "out"), "rinv": ("rel", "stat"), "dx": ("rows", "gelem")}, **GAIN_SPEC)
GELU_SPEC = dict({"y": ("rows", "out"), "dx": ("rows", "gelem"), "dW": ("tensor", "gelem"), "db": ("tensor", "gelem")}, **GAIN_SPEC)


def _entry_case(dev, dtype, entry, regime, rows, d, any_width, route):
    from meant_amd import ops
    tier = IDS[DTYPES.index(dtype)]
    t = _inputs(regime, rows, d, tier)
    eps = t["eps"]
    if entry == "rmsnorm":
        def gpu(x, gain):
            y = ops.rmsnorm(x, gain, eps, any_width=any_width)
            return {"y": y, "rinv": _saved(y, 2)}
        ref = lambda x, gain: {"y": N.rms64(x, gain, eps), "rinv": N.rinv64(x, eps)}
        _compare(dev, dtype, route, regime, gpu, ref, {"x": t["x"], "gain": t["gain"]}, {"y": t["dy"]}, PLAIN_SPEC)
    elif entry == "fork":
        def gpu(x, gain):
            y, res = ops.rmsnorm_fork(x, gain, eps, any_width=any_width)
            return {"y": y, "res": res, "rinv": _saved(y, 2)}
        ref = lambda x, gain: {"y": N.rms64(x, gain, eps), "res": x * 1.0, "rinv": N.rinv64(x, eps)}
        _compare(dev, dtype, route, regime, gpu, ref, {"x": t["x"], "gain": t["gain"]}, {"y": t["dy"], "res": t["dres"]}, PLAIN_SPEC)
    else:
        x = t["x"]
        if regime == "large" and d > 1:
            # gelu(-2^50 z) = 0: at d = 3 a row can keep ONE live element, whose normalised value is the constant sqrt(d) g and whose
            # gradient is a structural zero -- rounding noise against an exact 0 in float64.  Two live elements per row rule that out.
            x = x.clone()
            x[:, :2] = x[:, :2].abs()
        leaves = {"x": x, "gain": t["gain"], "W": torch.eye(d), "b": torch.zeros(d)}
        gpu = lambda x, gain, W, b: {"y": ops.linear_gelu_rmsnorm(x, W, b, gain, eps, any_width=any_width)}
        ref = lambda x, gain, W, b: {"y": N.rms64(N.gelu_linear64(x, W, b), gain, eps)}
        _compare(dev, dtype, route, regime, gpu, ref, leaves, {"y": t["dy"]}, GELU_SPEC)


ENTRIES = ["rmsnorm", "fork", "gelu_pre"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("regime", N.RMS_REGIMES)
@pytest.mark.parametrize("d,rows", ROW_SHAPES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_one_row_per_wave(dev, dtype, entry, d, rows, regime):
    rows = _rows_for(regime, d, rows, odd=rows % 2 == 1)
    assert norm_route(rows, d)[0] == "row"
    _entry_case(dev, dtype, entry, regime, rows, d, False, f"row_{entry}_d{d}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("regime", N.RMS_REGIMES)
@pytest.mark.parametrize("d,R,C", PACKED)
@pytest.mark.parametrize("entry", ENTRIES)
def test_packed(dev, dtype, entry, d, R, C, regime):
    rows = _rows_for(regime, d, ROWS, multiple=4)
    assert norm_route(rows, d) == ("packed", R, C, 8)
    _entry_case(dev, dtype, entry, regime, rows, d, False, f"packed_{entry}_d{d}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("regime", N.RMS_REGIMES)
@pytest.mark.parametrize("d,rows", WIDE_SHAPES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_wide_and_odd_widths(dev, dtype, entry, d, rows, regime):
    rows = _rows_for(regime, d, rows)
    assert norm_route(rows, d) == ("wide", 0, 0, 8 if d % 8 == 0 else 1)
    _entry_case(dev, dtype, entry, regime, rows, d, True, f"wide_{entry}_d{d}")


# ------------------------------------------------------------------------------------------------------------------------------
# 2. ops.rmsnorm_partial with the offset
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("regime", N.PARTIAL_REGIMES)
@pytest.mark.parametrize("d,d_part", PARTIAL_SHAPES)
def test_partial_with_bias(dev, dtype, d, d_part, regime):
    from meant_amd import ops
    assert norm_route(PARTIAL_ROWS, d, may_pack=False)[0] == ("row" if d % 8 == 0 else "wide")
    t = _inputs(regime, PARTIAL_ROWS, d, IDS[DTYPES.index(dtype)], "rms", d_part)
    eps = t["eps"]

    def gpu(x, gain, offset):
        y = ops.rmsnorm_partial(x, gain, offset, d_part, eps, any_width=True)
        return {"y": y, "rinv": _saved(y, 2)}

    ref = lambda x, gain, offset: {"y": N.rms64(x, gain, eps, d_part, offset), "rinv": N.rinv64(x, eps, d_part)}
    _compare(dev, dtype, f"partial_d{d}_p{d_part}", regime, gpu, ref, {"x": t["x"], "gain": t["gain"], "offset": t["offset"]}, {"y": t["dy"]},
             dict(PLAIN_SPEC, doffset=("tensor", "gelem")))


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the pooled forms: the sequence mean behind the norm (and of the norm's input)
def _group_cot(t, groups, d, key="dy"):
    """bf16-exact [groups, d]: the group means of the aligned dy (of dres)"""
    return t[key].view(groups, -1, d).mean(1).bfloat16().float()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("regime", N.RMS_REGIMES)
@pytest.mark.parametrize("d", POOLED_D)
@pytest.mark.parametrize("entry", ["gelu_pre_pooled", "fork_pooled"])
def test_pooled(dev, dtype, entry, d, regime):
    from meant_amd import ops
    rows = _rows_for(regime, d, NGROUPS * GROUP_ROWS, multiple=GROUP_ROWS)
    G = rows // GROUP_ROWS
    t = _inputs(regime, rows, d, IDS[DTYPES.index(dtype)])
    eps = t["eps"]
    x3 = t["x"].view(G, GROUP_ROWS, d)
    assert norm_route(rows, d)[0] == "packed" and ops.pooled_norm_ok(x3, GROUP_ROWS)
    route = f"{entry}_d{d}"
    if entry == "fork_pooled":
        def gpu(x, gain):
            y, xm = ops.rmsnorm_fork_pooled(x, gain, eps)
            return {"y": y, "xm": xm, "rinv": _saved(y, 2)}
        ref = lambda x, gain: {"y": N.rms64(x, gain, eps), "xm": x.mean(1), "rinv": N.rinv64(x, eps).reshape(-1)}
        spec = dict(PLAIN_SPEC, xm=("tensor", "out"))
        _compare(dev, dtype, route, regime, gpu, ref, {"x": x3, "gain": t["gain"]},
                 {"y": t["dy"].view(G, GROUP_ROWS, d), "xm": _group_cot(t, G, d, "dres")}, spec)
    else:
        leaves = {"x": x3, "gain": t["gain"], "W": torch.eye(d), "b": torch.zeros(d)}
        gpu = lambda x, gain, W, b: {"hm": ops.linear_gelu_rmsnorm_pooled(x, W, b, gain, eps)}
        ref = lambda x, gain, W, b: {"hm": N.rms64(N.gelu_linear64(x, W, b), gain, eps).mean(1)}
        spec = dict({"hm": ("tensor", "out"), "dx": ("rows", "gelem"), "dW": ("tensor", "gelem"), "db": ("tensor", "gelem")}, **GAIN_SPEC)
        _compare(dev, dtype, route, regime, gpu, ref, leaves, {"hm": _group_cot(t, G, d)}, spec)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. RMSNorm folded into the Linear that consumes it (bf16 tier): eps0 and eps3 both the regime's
FOLD_GRADS = {"dx": ("rows", "gelem"), "dgain": ("tensor", "gelem"), "dW": ("tensor", "gelem"), "db": ("tensor", "gelem"), "dgain3": ("tensor", "gelem")}


@pytest.mark.parametrize("regime", N.FOLD_REGIMES)
@pytest.mark.parametrize("pooled", [False, True], ids=["tokens", "pooled"])
def test_folded(dev, pooled, regime):
    from meant_amd import ops
    d, S = FOLD_D, FOLD_S
    G = 5 if pooled else 4
    rows = G * S
    t = _inputs(regime, rows, d, "bf16")
    eps = t["eps"]
    W, b, g3 = N.fold_weights(d, SEED)
    x3 = t["x"].view(G, S, d)
    assert ops.pooled_norm_ok(x3, rows) and d % 64 == 0               # the shapes norm_linear_ok admits
    leaves = {"x": x3, "gain": t["gain"], "W": W, "b": b, "gain3": g3}
    if pooled:
        def gpu(x, gain, W, b, gain3):
            hm, xm = ops.norm_linear_gelu_norm_pooled(x, gain, eps, W, b, gain3, eps)
            return {"hm": hm, "xm": xm}
        ref = lambda x, gain, W, b, gain3: {"hm": N.fold64(x, gain, W, b, gain3, eps, eps).mean(1), "xm": x.mean(1)}
        spec = dict({"hm": ("tensor", "out"), "xm": ("tensor", "out")}, **FOLD_GRADS)
        cots = {"hm": _group_cot(t, G, d), "xm": _group_cot(t, G, d, "dres")}
    else:
        def gpu(x, gain, W, b, gain3):
            y, res = ops.norm_linear_gelu_norm(x, gain, eps, W, b, gain3, eps)
            return {"y": y, "res": res}
        ref = lambda x, gain, W, b, gain3: {"y": N.fold64(x, gain, W, b, gain3, eps, eps), "res": x * 1.0}
        spec = dict({"y": ("rows", "out")}, **FOLD_GRADS)
        cots = {"y": t["dy"].view(G, S, d), "res": t["dres"].view(G, S, d)}
    _compare(dev, torch.bfloat16, "folded_pooled" if pooled else "folded", regime, gpu, ref, leaves, cots, spec)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. ops.layernorm
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("regime", N.LN_REGIMES)
@pytest.mark.parametrize("d,kind", LN_SHAPES)
def test_layernorm(dev, dtype, d, kind, regime):
    from meant_amd import ops
    rows = _rows_for(regime, d, ROWS)
    assert norm_route(rows, d, may_pack=False)[0] == kind
    t = _inputs(regime, rows, d, IDS[DTYPES.index(dtype)], "ln")
    eps = t["eps"]
    x_host = t["x"].to(dtype)                                          # `shifted` in the f32 tier is not bf16-exact; it is float-exact

    def gpu(x, gamma, beta):
        y = ops.layernorm(x, gamma, beta, eps, any_width=True)
        stats = _saved(y, 2)
        return {"y": y, "mean": N.ln_mean_in_row_units(stats[:, 0], x_host, eps), "rstd": stats[:, 1]}

    def ref(x, gamma, beta):
        xd = x.detach()
        return {"y": N.ln64(x, gamma, beta, eps), "mean": N.ln_mean_in_row_units(xd.mean(-1), x_host, eps),
                "rstd": 1.0 / (xd.var(dim=-1, unbiased=False) + eps).sqrt()}

    _compare(dev, dtype, f"layernorm_{kind}_d{d}", regime, gpu, ref, {"x": t["x"], "gamma": t["gamma"], "beta": t["beta"]}, {"y": t["dy"]},
             N.LN_CONSTANT_SPEC if regime == "constant" else N.LN_SPEC)
