"""Shared helpers of the norm regime tests (test_norm_regimes_host.py, test_gpu_norm_regimes.py): the input regimes that make the
statistics of the norm kernels and their eps term visible, the float64 references, the row-normalised comparison, and a float32
host emulation of the kernels' arithmetic with switchable defects.

Regimes (regime_inputs): `unit` (sigma = 1, eps = 1e-8: the inputs of every other norm test, where eps is below one float ulp),
`eps_heavy` (eps = 0.5), `tiny` (sigma = 2^-27: eps r = 0.57 at the reference's own eps), `vanishing` (sigma = 1e-20: x^2 is
denormal in float32, r -> 1 / eps), `large` (sigma = 2^50), `zero` (every third row all zeros), `spike` (2^-10 randn plus one
element sqrt(d) per row, walking over every chunk position), and for LayerNorm `shifted` (mean 4096, std 1 in the f32 tier; mean 64,
std 4 in the bf16 tier) and `constant`; for the partial RMSNorm `tail` (the columns the statistics must not see scaled by 2^10).
`large` does not go beyond 2^50: above that the sum of squares overflows float32 in the kernels and in the reference's own x.norm
(utils/rms_norm.py:42) alike, and include/meant_hip.h defines nothing there.  Every x and dy is exactly representable in bf16 (but
for `shifted` in the f32 tier), so both tiers see the same numbers, and dy is ALIGNED with x (dy = bf16(x / sigma + 0.25 randn)): with
an independent dy the x k term of the backward is 1 / sqrt(d) of the other term and a wrong k hides inside the bf16 bound.

No regime had to change to separate its defect by 4 x the bound (REGIME_NOTES); the folded chain needed a choice of its Linear that
keeps the gradient aligned (fold_weights).

References: the literal formulas of utils/rms_norm.py:40-57 (partial and bias forms included), nn.LayerNorm, gelu(Linear(.)) in
front of the norm, the sequence mean behind it and Linear(RMSNorm(x)), in torch float64 with autograd on whatever device the
inputs live on.  A row of zeros follows torch's convention: the subgradient of the norm at 0 is 0.

Comparison (check): y and dx row by row, max_j |got - ref| / max_j |ref| over the row, maximised over the rows (a reference row of
zeros must be matched exactly); parameter gradients and pooled features per tensor; rinv and rstd element by element, relatively;
the LayerNorm mean in units of the row's sqrt(var + eps).  Nothing is compared absolutely: y ~ 1e-12 in `vanishing`.  The bounds
are tests.util.TOL: `out` (times 4 in bf16, as the other norm tests use it) for forward values, `gelem` for gradients, the f32
tier's `out` for the float statistics of either tier.  Every compared tensor must be finite."""
import math

import torch
import torch.nn.functional as F

from tests.util import TOL

RMS_REGIMES = ("unit", "eps_heavy", "tiny", "vanishing", "large", "zero", "spike")
LN_REGIMES = ("unit", "eps_heavy", "shifted", "constant", "large", "spike")
PARTIAL_REGIMES = ("unit", "eps_heavy", "tail")
FOLD_REGIMES = ("unit", "eps_heavy", "tiny", "zero")
SIGMA = {"tiny": 2.0 ** -27, "vanishing": 1e-20, "large": 2.0 ** 50}
EPS = {"eps_heavy": 0.5, "shifted": 1e-5, "constant": 1e-5}
REGIME_NOTES = ()                                    # (regime, what changed, why): nothing had to change


def _bf(t):
    return t.bfloat16().float()


def spike_column(i, d):
    """column of row i's spike: chunk i mod ceil(d / 8), element i mod 8 of it (folded back into the row where d % 8 != 0)"""
    return (8 * (i % -(-d // 8)) + i % 8) % d


def regime_inputs(regime, rows, d, seed, tier="bf16", norm="rms", d_part=None):
    """float32 host tensors: x, dy [rows, d], gain (gamma), beta, offset [d], eps, and sigma, the scale of a live row.
    norm = "ln": eps defaults to nn.LayerNorm's 1e-5."""
    assert regime in RMS_REGIMES + LN_REGIMES + PARTIAL_REGIMES, regime
    gen = torch.Generator().manual_seed(seed)
    z = _bf(torch.randn(rows, d, generator=gen))
    noise = 0.25 * torch.randn(rows, d, generator=gen)
    gain = 1 + 0.1 * torch.randn(d, generator=gen)
    beta = 0.1 * torch.randn(d, generator=gen)
    eps = EPS.get(regime, 1e-5 if norm == "ln" else 1e-8)
    sigma, xhat = 1.0, z
    if regime in ("unit", "eps_heavy"):
        x = z
    elif regime in ("tiny", "large"):
        sigma = SIGMA[regime]
        x = z * sigma                                # a power of two: exact
    elif regime == "vanishing":
        sigma = SIGMA[regime]
        x = _bf(z * sigma)
        xhat = x / sigma
    elif regime == "zero":
        x = z.clone()
        x[0::3] = 0
        xhat = x
    elif regime == "spike":
        assert rows >= -(-d // 8), "every chunk position has to carry a spike once"
        x = _bf(z * 2.0 ** -10)
        for i in range(rows):
            x[i, spike_column(i, d)] = _bf(torch.tensor(math.sqrt(d))).item()
        xhat = x
    elif regime == "shifted":
        mean, sigma = (4096.0, 1.0) if tier == "f32" else (64.0, 4.0)
        x = mean + sigma * z
        x = x if tier == "f32" else _bf(x)
        xhat = (x - mean) / sigma
    elif regime == "constant":
        x = _bf(3 * torch.randn(rows, 1, generator=gen)).expand(rows, d).contiguous()
        assert bool((x != 0).all())
    elif regime == "tail":
        assert d_part is not None and 0 < d_part < d
        x = z.clone()
        x[:, d_part:] *= 2.0 ** 10
    dy = _bf(xhat + noise)
    return dict(x=x, dy=dy, gain=gain, gamma=gain, beta=beta, offset=beta, eps=eps, sigma=sigma)


# ------------------------------------------------------------------------------------------------------------------------------
# float64 references
def rms64(x, gain, eps, d_part=None, offset=None):
    """utils/rms_norm.py:40-57"""
    d = x.shape[-1]
    part, d_x = (x, d) if d_part is None else (x[..., :d_part], d_part)
    rms_x = part.norm(2, dim=-1, keepdim=True) * d_x ** (-1. / 2)
    y = gain * (x / (rms_x + eps))
    return y if offset is None else y + offset


def rinv64(x, eps, d_part=None):
    part, d_x = (x, x.shape[-1]) if d_part is None else (x[..., :d_part], d_part)
    return 1.0 / (part.detach().double().norm(2, dim=-1) * d_x ** (-1. / 2) + eps)


def ln64(x, gamma, beta, eps):
    return F.layer_norm(x, (x.shape[-1],), gamma, beta, eps)


def gelu_linear64(x, weight, bias):
    return F.gelu(F.linear(x, weight, bias))


def evaluate(forward, leaves, cots, prep=None, device=None):
    """forward(**leaves) -> dict of outputs; the gradient of sum_k <outputs[k], cots[k]> w.r.t. every leaf, as "d" + its name.
    prep(name, tensor): the leaf as the evaluation takes it (float64, on `device` if given, by default)"""
    prep = prep or (lambda name, t: t.to(device).double() if device is not None else t.double())
    ls = {k: prep(k, v).detach().clone().requires_grad_() for k, v in leaves.items()}
    outs = forward(**ls)
    loss = sum((outs[k].double() * cots[k].to(outs[k].device).double()).sum() for k in cots)
    loss.backward()
    res = {k: v.detach() for k, v in outs.items()}
    res.update({"d" + k: v.grad.detach() for k, v in ls.items() if v.grad is not None})
    return res


# ------------------------------------------------------------------------------------------------------------------------------
# comparison
def _f64(t):
    return t.detach().double().cpu()


def _ratio(diff, den):
    bad = torch.full_like(diff, float("inf"))
    e = torch.where(den > 0, diff / den.clamp_min(1e-300), torch.where(diff > 0, bad, torch.zeros_like(diff)))
    return e.max().item()


def row_error(got, ref):
    g, r = _f64(got), _f64(ref)
    g, r = g.reshape(-1, g.shape[-1]), r.reshape(-1, r.shape[-1])
    return _ratio((g - r).abs().amax(1), r.abs().amax(1))


def tensor_error(got, ref, floor=0.0):
    g, r = _f64(got), _f64(ref)
    return _ratio((g - r).abs().max().reshape(1), r.abs().max().clamp_min(floor).reshape(1))


def rel_error(got, ref):
    g, r = _f64(got).reshape(-1), _f64(ref).reshape(-1)
    return _ratio((g - r).abs(), r.abs())


def unit_error(got, ref):
    """both sides already divided by their natural unit (ln_mean_in_row_units)"""
    return (_f64(got) - _f64(ref)).abs().max().item()


MODES = {"rows": row_error, "tensor": tensor_error, "rel": rel_error, "units": unit_error}


def bound(key, dtype):
    """key: "out", "gelem" (the tier's) or "stat" (float statistics: the f32 tier's `out` in either tier)"""
    if key == "stat":
        return TOL[torch.float32]["out"]
    return TOL[dtype][key] * (4 if key == "out" and dtype == torch.bfloat16 else 1)


def errors(got, ref, spec):
    """spec: name -> (mode, bound key) or (mode, bound key, name of the reference tensor whose largest magnitude is the floor of the
    denominator: for a gradient that is structurally zero).  Every named tensor must be present on both sides."""
    fig = {}
    for name, (mode, _, *floor) in spec.items():
        g = _f64(got[name])
        kw = {"floor": _f64(ref[floor[0]]).abs().max().item()} if floor else {}
        fig[name] = MODES[mode](g, ref[name], **kw) if bool(torch.isfinite(g).all()) else float("inf")
    return fig


def check(got, ref, spec, dtype, what):
    """asserts every compared tensor finite, then every figure within its bound; returns the figures"""
    for name in spec:
        assert bool(torch.isfinite(_f64(got[name])).all()), f"{what}: {name} is not finite"
        assert bool(torch.isfinite(_f64(ref[name])).all()), f"{what}: the reference's {name} is not finite"
    fig = errors(got, ref, spec)
    for name, (_, key, *_f) in spec.items():
        assert fig[name] <= bound(key, dtype), f"{what}: {name} {fig[name]:.2e} > {bound(key, dtype):.1e}"
    return fig


RMS_SPEC = {"y": ("rows", "out"), "rinv": ("rel", "stat"), "dx": ("rows", "gelem"), "dgain": ("tensor", "gelem")}
LN_SPEC = {"y": ("rows", "out"), "mean": ("units", "stat"), "rstd": ("rel", "stat"), "dx": ("rows", "gelem"), "dgamma": ("tensor", "gelem"),
           "dbeta": ("tensor", "gelem")}
# rows of one constant: xhat = 0 and dgamma = sum dy xhat is structurally zero (rounding noise in the float64 reference): it is held
# against the scale of dbeta = sum dy, the same sum without the factor |xhat| <= O(1)
LN_CONSTANT_SPEC = dict(LN_SPEC, dgamma=("tensor", "gelem", "dbeta"))
FOLD_SPEC = {"y": ("rows", "out"), "dx": ("rows", "gelem")}


def ref_rmsnorm(t, d_part=None, with_offset=False):
    leaves = {"x": t["x"], "gain": t["gain"]}
    if with_offset:
        leaves["offset"] = t["offset"]
    ref = evaluate(lambda x, gain, offset=None: {"y": rms64(x, gain, t["eps"], d_part, offset)}, leaves, {"y": t["dy"]})
    ref["rinv"] = rinv64(t["x"], t["eps"], d_part)
    return ref


def ln_mean_in_row_units(mean, x, eps):
    """the mean [rows] divided by the row's float64 sqrt(var + eps): the unit in which an error of the mean reaches y"""
    x = x.detach().double().cpu()
    return _f64(mean) / (x.var(dim=-1, unbiased=False) + eps).sqrt()


def ref_layernorm(t):
    ref = evaluate(lambda x, gamma, beta: {"y": ln64(x, gamma, beta, t["eps"])}, {k: t[k] for k in ("x", "gamma", "beta")}, {"y": t["dy"]})
    x = t["x"].double()
    ref["mean"] = ln_mean_in_row_units(x.mean(-1), x, t["eps"])
    ref["rstd"] = 1.0 / (x.var(dim=-1, unbiased=False) + t["eps"]).sqrt()
    return ref


def fold_weights(d, seed):
    """the Linear of the folded chain: close to the identity, so that the gradient that reaches the folded norm's output stays
    aligned with x (a random W would scatter it, and the kcoef x term would be 1 / sqrt(d) of the rest), a bias of 2 + 0.1 randn, and
    the second gain.  The bias puts the pre-activation where gelu is close to linear and makes the direction of the activation
    mostly a constant, so that RMSNorm_3's backward, which removes the component of dy along its input, leaves the part aligned
    with x alone: with a bias around 0 a kcoef without its (1 - eps_up r_up) factor moved dx by 0.24 of a row in `eps_heavy`, 3.99 x
    the bf16 gradient bound; with it by 0.55."""
    gen = torch.Generator().manual_seed(seed + 1000)
    W = torch.eye(d) + 0.1 * torch.randn(d, d, generator=gen) / math.sqrt(d)
    return W, 2 + 0.1 * torch.randn(d, generator=gen), 1 + 0.1 * torch.randn(d, generator=gen)


def fold64(x, gain0, W, b, gain3, eps0, eps3):
    """RMSNorm_3(gelu(Linear(RMSNorm_0(x)))): meant/meant.py:61-64"""
    return rms64(gelu_linear64(rms64(x, gain0, eps0), W, b), gain3, eps3)


# ------------------------------------------------------------------------------------------------------------------------------
# float32 host emulation of the kernels' arithmetic (csrc/norm.hip), with switchable defects
DEFECTS = ("no_eps", "eps_in_sqrt", "bwd_no_eps", "fold_no_eps", "lost_chunk", "ln_one_pass", "ln_eps_outside", "no_guard", "partial_all_columns")
LOST_CHUNK = 5                                       # the chunk index `lost_chunk` leaves out of the sum of squares


def _store(t, tier):
    return _bf(t) if tier == "bf16" else t


def _chunks(t):
    """[rows, d] -> [rows, ceil(d / 8), 8], zero-padded: a lane's 8 columns at a time, then the sum over the lanes"""
    rows, d = t.shape
    return F.pad(t, (0, -d % 8)).view(rows, -1, 8)


def _chunked_sum(t, lost=None):
    per = _chunks(t).sum(-1)
    if lost is not None:
        per = per.clone()
        per[:, lost % per.shape[1]] = 0
    return per.sum(-1)


def emulate_rinv(x, eps, d_part=None, defect=None):
    d = x.shape[1]
    d_stat = d if d_part is None or defect == "partial_all_columns" else d_part
    xs = x.clone()
    xs[:, d_stat:] = 0
    ss = _chunked_sum(xs * xs, LOST_CHUNK if defect == "lost_chunk" else None)
    inv_sqrt_d = 1.0 / math.sqrt(d_stat)
    if defect == "no_eps":
        return 1.0 / (ss.sqrt() * inv_sqrt_d)
    if defect == "eps_in_sqrt":
        return 1.0 / (ss * (inv_sqrt_d * inv_sqrt_d) + eps).sqrt()
    return 1.0 / (ss.sqrt() * inv_sqrt_d + eps)


def emulate_rms_bwd(dy, x, gain, r, eps, tier, d_part=None, defect=None, gelu_grad=None):
    """(dx as the tier stores it, dgain): norm.hip's rmsnorm_bwd_wide_kernel / rmsnorm_bwd_packed_kernel"""
    d = x.shape[1]
    d_stat = d if d_part is None or defect == "partial_all_columns" else d_part
    gd = gain * dy
    xs = x.clone()
    xs[:, d_stat:] = 0
    cdot = _chunked_sum(gd * x)                     # over the whole row: every column of y carries the factor r
    nsd = (1.0 / r if defect == "bwd_no_eps" else 1.0 / r - eps) * d_stat
    k = cdot * r * r / nsd
    if defect != "no_guard":
        k = torch.where(nsd > 0, k, torch.zeros_like(k))
    dx = r[:, None] * gd - k[:, None] * xs
    if gelu_grad is not None:
        dx = dx * gelu_grad
    return _store(dx, tier), (dy * x * r[:, None]).sum(0), dx


def emulate_rmsnorm(t, tier, d_part=None, with_offset=False, defect=None):
    x, dy, gain, eps = t["x"].float(), t["dy"].float(), t["gain"].float(), torch.tensor(t["eps"], dtype=torch.float32)
    r = emulate_rinv(x, eps, d_part, defect)
    y = gain * (x * r[:, None])
    if with_offset:
        y = y + t["offset"]
    dx, dgain, _ = emulate_rms_bwd(dy, x, gain, r, eps, tier, d_part, defect)
    out = {"y": _store(y, tier), "rinv": r, "dx": dx, "dgain": dgain}
    if with_offset:
        out["doffset"] = dy.sum(0)
    return out


def emulate_layernorm(t, tier, defect=None):
    """the two-pass statistics of layernorm_fwd_wide_kernel, rstd = rsqrt(var + eps), and layernorm_bwd_wide_kernel"""
    x, dy, gamma, beta, eps = t["x"].float(), t["dy"].float(), t["gamma"].float(), t["beta"].float(), torch.tensor(t["eps"], dtype=torch.float32)
    d = x.shape[1]
    mean = _chunked_sum(x) / d
    if defect == "ln_one_pass":
        var = _chunked_sum(x * x) / d - mean * mean
    else:
        c = x - mean[:, None]
        var = _chunked_sum(c * c) / d
    rstd = 1.0 / (var.sqrt() + eps) if defect == "ln_eps_outside" else 1.0 / (var + eps).sqrt()
    xh = (x - mean[:, None]) * rstd[:, None]
    y = xh * gamma + beta
    gd = dy * gamma
    s1, s2 = _chunked_sum(gd) / d, _chunked_sum(gd * xh) / d
    dx = rstd[:, None] * (gd - s1[:, None] - xh * s2[:, None])
    return {"y": _store(y, tier), "mean": ln_mean_in_row_units(mean, x, t["eps"]), "rstd": rstd, "dx": _store(dx, tier),
            "dgamma": (dy * xh).sum(0), "dbeta": dy.sum(0)}


def _gelu_grad32(p):
    return 0.5 * (1 + torch.erf(p / math.sqrt(2.0))) + p * torch.exp(-0.5 * p * p) / math.sqrt(2.0 * math.pi)


def emulate_fold(t, W, b, gain3, defect=None):
    """the folded chain of the bf16 tier: statistics of x, pre = r0 (x W'^T) + b with W' = bf16(W diag(g0)), a = gelu(pre), RMSNorm_3;
    backward: the chained norm backward (dpre, the scaled gradient r0 dpre, kcoef), then dx = (r0 dpre) W' - kcoef x"""
    x, dy, g0, eps = t["x"].float(), t["dy"].float(), t["gain"].float(), torch.tensor(t["eps"], dtype=torch.float32)
    d = x.shape[1]
    r0 = emulate_rinv(x, eps, None, defect)
    wp = _bf(W * g0)
    pre = _bf(r0[:, None] * (x @ wp.t()) + b)
    a = _bf(F.gelu(pre))
    r3 = emulate_rinv(a, eps, None, defect)
    y = _bf(gain3 * (a * r3[:, None]))
    _, _, dpre = emulate_rms_bwd(dy, a, gain3, r3, eps, "bf16", None, defect, gelu_grad=_gelu_grad32(pre))
    s = _chunked_sum(dpre * (pre - b))
    den = (torch.ones_like(r0) if defect == "fold_no_eps" else 1.0 - eps * r0) * d
    kcoef = s * r0 * r0 / den
    if defect != "no_guard":
        kcoef = torch.where(den > 0, kcoef, torch.zeros_like(kcoef))
    dx = _bf(dpre * r0[:, None]) @ wp - kcoef[:, None] * x
    return {"y": y, "dx": _bf(dx)}
