"""Shared helpers of the loss regime tests (test_loss_regimes_host.py, test_gpu_loss_regimes.py): the input regimes under which a
hard-label softmax cross-entropy can be wrong without randn rows noticing, the float64 references, a float32 host emulation of the
kernels' arithmetic (csrc/optim.hip: softmax_ce_fwd_kernel / _bwd_kernel, ce_probs_kernel) with switchable defects, and the
comparison with its gates.

Regimes (regime_inputs; the logits are rounded to the tier's storage type, so the reference sees what the kernel reads):
  plain            randn * 3: the inputs of the older test, the control
  peaked           randn with one column 40 above it.  The peak walks the row (peak_positions): every chunk start, every lane of one
                   chunk, every ragged-tail column.  Even rows have the target on the peak (loss near 0), odd rows off it (near 40):
                   a lost chunk, lane, tail column or wave is off by e^40
  wide             randn * 30: most exponentials underflow
  shifted+1000, shifted-1000 (both tiers), shifted+30000 (f32 tier): plain plus a bf16-exact constant
  masked           -inf on whole aligned chunks (the first one included), on scattered single columns, on everything but two columns,
                   on the whole ragged tail (the last chunk where V % 8 == 0); the row's slot decides which
  masked_additive  the same layouts with the attention masks' additive -1e9 in place of -inf
  uniform          one value per row: loss log V, gradient 1 / V - onehot
  garbage_ignored  plain, but every second row does not count and holds NaN, +-inf and 3e38: its row_loss and gradient row are zeros
The target of a row that counts is never masked.  Row r of a case sits in slot (r + seed) % 4; the slot picks the row's target among
column 8 * (V >> 3) - 1, the first tail column 8 * (V >> 3), V - 1 and 0, and its mask layout.  With T >= 5 the last row does not
count in any regime: its target is the ignore value, V, ld - 1 (both addresses inside the buffer), -1 or 2^31 + 3, by (seed + V).

References, float64, all from the shift-invariant form log S + (M - x_t) with M the row maximum and S = sum_j exp(x_j - M):
row_loss, lse = M + log S, the mean over the rows that count (0 when none does: what ops.softmax_cross_entropy returns) and dlogits
of the whole [T, ld] buffer, exact zeros on the rows that do not count and on the columns >= V.

Comparison (check) and gates.  Everything compared must be finite.  Error measures:
  row_loss, mean, lse   |err| / max(1, |ref|), lse through its meaning M + log S (added in float64 from the kernel's pair)
  dlogits               max |err| / |gscale|; in the bf16 tier less one bf16 rounding of the reference element, 2^-8 |ref|
  rowsum (f32 tier)     |sum_j dlogits[t, j]| / |gscale| of a row that counts: 0 in exact arithmetic, the figure that exposes a
                        logsumexp kept in one float (0.00045 at a shift of 30000)
  zeros                 the largest magnitude where the reference is a structural zero: must be 0
Every gate is 4 x the worst figure of the emulation as it stands (emulate: float32, shift-invariant, -inf-guarded, the kernel's 256
threads x 8-column chunks, ragged tail, pair merge over lanes and waves) against float64 over every regime, the V of GATE_VS,
T = 5 (`peaked` also with one row per peak position at V = 2059) and seeds 0..4 (test_loss_regimes_host.py recomputes this and holds
GATES within [3.2 x, 8 x] of it).  The factor 4 allows for the device's __expf / logf against the host's exp / log and for another
merge order.  The bf16 tier's dlogits gate is taken from the emulation's gradient BEFORE its rounding to bf16, since the
measure already forgives that rounding.  Worst figures measured (f32 tier / bf16 tier):
  row_loss 1.33e-7 / 1.13e-7, mean 1.11e-7 / 9.5e-8, lse 1.41e-7 / 1.41e-7, dlogits 1.92e-7 / 2.03e-7, rowsum 3.23e-7
meant_ce_probs (emulate_ce_probs: max, sum of exp(x - max) term after term, log, per row in float32) over rand rows, rows of exact 0 and
1 and rand + 1000 at the shapes of CE_PROBS_SHAPES, seeds 0..4: loss 1.63e-6 (|err| / max(1, |ref|)), dprobs 1.05e-7 (max |err| * B,
the gradient carrying the factor 1 / B of the mean; 9.5e-8 on a host whose vectorised exp rounds differently: the larger of the two
is taken).  The loss figure is that of the 0 / 1 rows at C = 3129: some 1500 equal terms e^-1 added one after the other to a sum
near 2000 round the same way, 1e-5 of the sum; rand rows stay at 1.8e-7, and a pairwise sum of the same terms at 1.2e-7.
The kernel itself keeps max + log sum in ONE float (emulate_ce_probs(one_float=True)): on probabilities that costs at most half an
ulp of 8.7, inside these gates; on rand + 1000, outside the entry's contract, half an ulp of 1008, 2^-15, which that kind is allowed
on top of the gates (test_gpu_loss_regimes.test_ce_probs_against_float64).  That is what one thread per row costs at this width (DESIGN, "Not built": the row-parallel form)."""
import functools
import math

import torch

NEG_INF = float("-inf")
REGIMES = ("plain", "peaked", "wide", "shifted+1000", "shifted-1000", "shifted+30000", "masked", "masked_additive", "uniform",
           "garbage_ignored")
GSCALES = (1.0, 1.0 / 7.0, -3.0)
GATE_VS = (1, 5, 8, 12, 2047, 2048, 2049, 2056, 2059, 4101)
# 4 x the emulation's worst, rounded up to two digits (module docstring)
GATES = {"f32": {"row_loss": 5.3e-7, "mean": 4.5e-7, "lse": 5.7e-7, "dlogits": 7.7e-7, "rowsum": 1.3e-6, "zeros": 0.0},
         "bf16": {"row_loss": 4.5e-7, "mean": 3.8e-7, "lse": 5.7e-7, "dlogits": 8.2e-7, "zeros": 0.0}}
CE_PROBS_SHAPES = [(B, C) for B in (1, 63, 64, 65, 257) for C in (1, 2, 7, 3129)]
CE_PROBS_KINDS = ("rand", "zero_one", "shifted")
CE_PROBS_GATES = {"loss": 6.6e-6, "dprobs": 4.2e-7}


def regimes(tier):
    return tuple(r for r in REGIMES if tier == "f32" or r != "shifted+30000")


def _store(t, tier):
    return t.bfloat16().float() if tier == "bf16" else t.float()


def ceil8(v):
    return (v + 7) // 8 * 8


def peak_positions(V):
    """every chunk start, the other lanes of one chunk (the second where there is one), every ragged-tail column"""
    nchunk = V >> 3
    pos = [8 * c for c in range(nchunk)]
    if nchunk:
        pos += [8 * min(1, nchunk - 1) + i for i in range(1, 8)]
    return pos + list(range(8 * nchunk, V))


def counted(targets, V, ignore_index):
    return (targets != ignore_index) & (targets >= 0) & (targets < V)


def _valid_targets(V, ignore_index):
    return [c for c in (8 * (V >> 3) - 1, 8 * (V >> 3), V - 1, 0) if 0 <= c < V and c != ignore_index]


def bad_targets(V, ld, ignore_index):
    return [b for b in (ignore_index, V, ld - 1, -1, 2 ** 31 + 3) if not (0 <= b < V) or b == ignore_index]


def _mask_layout(slot, V, target, gen):
    """bool [V], True = masked; the target stays"""
    nchunk = V >> 3
    mask = torch.zeros(V, dtype=torch.bool)
    if slot == 0:                                        # whole aligned chunks, the first included
        for c in range(0, nchunk, 3):
            mask[8 * c:8 * c + 8] = True
    elif slot == 1:                                      # scattered single columns
        mask = torch.rand(V, generator=gen) < 0.3
    elif slot == 2:                                      # everything but two columns
        mask[:] = True
        mask[(target + 1 + V // 2) % V] = False
    else:                                                # the whole ragged tail (the last chunk where there is none)
        mask[8 * nchunk if V % 8 else max(0, V - 8):] = True
    mask[target] = False
    return mask


def regime_inputs(regime, T, V, ld, seed, tier, ignore_index=-100, gscale=None, pad=0.0):
    """dict: logits float32 [T, ld] (columns >= V hold `pad`), targets int64 [T], ignore_index, gscale (a float32 value, as the
    device scalar holds it), and V, ld, tier, regime"""
    assert regime in regimes(tier) and 0 < V <= ld and ld % 8 == 0
    gen = torch.Generator().manual_seed(seed * 1000003 + V)
    z = torch.randn(T, V, generator=gen)
    valid, bad = _valid_targets(V, ignore_index), bad_targets(V, ld, ignore_index)
    slots = [(r + seed) % 4 for r in range(T)]
    targets = torch.tensor([valid[s % len(valid)] if valid else ignore_index for s in slots], dtype=torch.int64)
    if regime == "peaked":
        pos = peak_positions(V)
        x = z.clone()
        for r in range(T):
            p = pos[(r + seed) % len(pos)]
            x[r, p] += 40.0
            targets[r] = p if r % 2 == 0 or V == 1 else (p + 1 + (r // 2) % (V - 1)) % V
            if targets[r] == ignore_index:
                targets[r] = p
    elif regime == "wide":
        x = z * 30
    elif regime.startswith("shifted"):
        x = z * 3 + float(regime[len("shifted"):])
    elif regime == "uniform":
        x = (z[:, :1] * 3).expand(T, V).clone()
    else:
        x = z * 3
    x = _store(x, tier)
    if regime in ("masked", "masked_additive"):
        for r in range(T):
            # keep the target out of what the layout masks whole where the row is wide enough: the last column under masked
            # chunks, the last chunk's last column under a masked tail
            want = {0: V - 1, 3: 8 * (V >> 3) - 1 if V % 8 and V > 8 else 0}.get(slots[r])
            if want is not None and want != ignore_index:
                targets[r] = want
            m = _mask_layout(slots[r], V, int(targets[r]), gen)
            x[r] = torch.where(m, torch.full_like(x[r], NEG_INF), x[r]) if regime == "masked" else _store(x[r] - 1e9 * m.float(), tier)
    # the rows that do not count
    off = [T - 1] if T >= 5 else []
    if regime == "garbage_ignored":
        off = sorted(set(off) | set(range(1, T, 2)) | ({0} if T == 1 else set()))
        junk = torch.tensor([float("nan"), float("inf"), 3e38, NEG_INF, -3e38])
        for k, r in enumerate(off):
            x[r] = _store(junk[(torch.arange(V) + k) % 5], tier)
    for k, r in enumerate(off):
        targets[r] = bad[(k + seed + V) % len(bad)]
    logits = torch.full((T, ld), float(pad))
    logits[:, :V] = x
    g = GSCALES[(seed + T + V) % 3] if gscale is None else gscale
    return dict(logits=logits, targets=targets, ignore_index=ignore_index, gscale=torch.tensor(g, dtype=torch.float32).item(), V=V, ld=ld,
                tier=tier, regime=regime)


# ------------------------------------------------------------------------------------------------------------------------------
# float64 references
def reference(t):
    """row_loss [T], lse [T], mean, dlogits [T, ld], counted [T]; rows that do not count: row_loss 0, lse 0 (not compared), gradient 0"""
    V, ld, tg = t["V"], t["ld"], t["targets"]
    x = t["logits"][:, :V].double()
    cnt = counted(tg, V, t["ignore_index"])
    x = torch.where(cnt[:, None], x, torch.zeros_like(x))          # a row that does not count may hold anything
    M = x.amax(1)
    logS = (x - M[:, None]).exp().sum(1).log()
    tc = torch.where(cnt, tg, torch.zeros_like(tg))
    xt = x.gather(1, tc[:, None])[:, 0]
    zero = torch.zeros_like(M)
    row_loss = torch.where(cnt, logS + (M - xt), zero)
    onehot = torch.zeros_like(x).scatter_(1, tc[:, None], 1.0)
    d = torch.zeros(x.shape[0], ld, dtype=torch.float64)
    d[:, :V] = torch.where(cnt[:, None], (((x - M[:, None]) - logS[:, None]).exp() - onehot) * t["gscale"], torch.zeros_like(x))
    n = int(cnt.sum())
    return dict(row_loss=row_loss, lse=torch.where(cnt, M + logS, zero), mean=row_loss.sum() / max(1, n), dlogits=d, counted=cnt)


# ------------------------------------------------------------------------------------------------------------------------------
# float32 host emulation of softmax_ce_fwd_kernel / softmax_ce_bwd_kernel, with switchable defects
DEFECTS = ("lse_one_float", "no_inf_guard", "lost_chunk", "lost_tail", "lost_wave", "reads_padding", "target_off_by_one", "ignored_not_zero",
           "gscale_dropped", "padding_not_zeroed")
LOST_WAVE = 2


def _online(m, s, vals, real, guard):
    """one step of a thread's online (max, sum) update over the columns vals [..., k]; real: the thread has such a step"""
    mn = torch.maximum(m, vals.amax(-1))
    s_new = s * (m - mn).exp() + (vals - mn[..., None]).exp().sum(-1)
    take = real & (mn != NEG_INF) if guard else real
    return torch.where(take, mn, m), torch.where(take, s_new, s)


def _merge(m, s, mo, so):
    mn = torch.maximum(m, mo)
    zero = torch.zeros_like(s)
    return mn, torch.where(m == NEG_INF, zero, s * (m - mn).exp()) + torch.where(mo == NEG_INF, zero, so * (mo - mn).exp())


def emulate_fwd(t, defect=None):
    """(M, logS) float32 [T] as the forward kernel leaves them, row_loss float32 [T]; with `lse_one_float` logS is 0 and M the one
    float M + log S of the older handoff"""
    V, tg = t["V"], t["targets"]
    Vs = t["ld"] if defect == "reads_padding" else V
    x = t["logits"][:, :Vs].float()
    T = x.shape[0]
    guard = defect != "no_inf_guard"
    nchunk, ntail = Vs >> 3, Vs & 7
    npass = -(-nchunk // 256)
    ch = torch.full((T, npass * 256, 8), NEG_INF)
    ch[:, :nchunk] = x[:, :8 * nchunk].reshape(T, nchunk, 8)
    real = torch.arange(npass * 256) < nchunk
    if defect == "lost_chunk":
        real[nchunk // 2] = False
    ch, real = ch.view(T, npass, 256, 8), real.view(npass, 256)
    m, s = torch.full((T, 256), NEG_INF), torch.zeros(T, 256)
    for p in range(npass):
        m, s = _online(m, s, ch[:, p], real[p].expand(T, 256), guard)
    tail = torch.full((T, 256, 1), NEG_INF)
    tail[:, :ntail, 0] = x[:, 8 * nchunk:]
    treal = torch.arange(256) < (ntail - 1 if defect == "lost_tail" else ntail)
    m, s = _online(m, s, tail, treal.expand(T, 256), guard)
    m, s = m.view(T, 4, 64), s.view(T, 4, 64)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        m, s = _merge(m, s, m[..., lane ^ o], s[..., lane ^ o])
    wm, ws = m[..., 0].clone(), s[..., 0]
    if defect == "lost_wave":
        wm[:, LOST_WAVE] = NEG_INF
    M = wm.amax(1)
    S = torch.zeros(T)
    for w in range(4):
        S = S + torch.where(wm[:, w] == NEG_INF, torch.zeros(T), ws[:, w] * (wm[:, w] - M).exp())
    logS = S.log()
    cnt = counted(tg, V, t["ignore_index"])
    tc = torch.where(cnt, tg, torch.zeros_like(tg))
    if defect == "target_off_by_one":
        tc = (tc + 1) % V
    xt = x.gather(1, tc[:, None])[:, 0]
    if defect == "lse_one_float":
        M, logS = M + logS, torch.zeros(T)
        loss = M - xt
    else:
        loss = logS + (M - xt)
    row_loss = loss if defect == "ignored_not_zero" else torch.where(cnt, loss, torch.zeros(T))
    return M, logS, row_loss


def emulate_bwd(t, M, logS, defect=None):
    """dlogits float32 [T, ld] before the rounding to the tier's storage type"""
    V, ld, tg = t["V"], t["ld"], t["targets"]
    x = t["logits"].float()
    T = x.shape[0]
    cnt = counted(tg, V, t["ignore_index"])
    tc = torch.where(cnt, tg, torch.zeros_like(tg))
    if defect == "target_off_by_one":
        tc = (tc + 1) % V
    g = torch.tensor(1.0 if defect == "gscale_dropped" else t["gscale"], dtype=torch.float32)
    d = ((x - M[:, None]) - logS[:, None]).exp() - torch.zeros_like(x).scatter_(1, tc[:, None], 1.0)
    d = d * g
    if defect != "ignored_not_zero":
        d = torch.where(cnt[:, None], d, torch.zeros_like(d))
    if defect != "padding_not_zeroed":
        d[:, V:] = 0
    return d


def emulate(t, defect=None):
    """what the two entries and the wrapper's mean give, as check takes it (plus dlogits_f32, the gradient before its rounding)"""
    M, logS, row_loss = emulate_fwd(t, defect)
    d = emulate_bwd(t, M, logS, defect)
    n = int(counted(t["targets"], t["V"], t["ignore_index"]).sum())
    return dict(row_loss=row_loss, lse=M.double() + logS.double(), mean=row_loss.sum() / max(1, n), dlogits=_store(d, t["tier"]), dlogits_f32=d)


# ------------------------------------------------------------------------------------------------------------------------------
# comparison
def _f64(v):
    return (v.detach() if isinstance(v, torch.Tensor) else torch.tensor(v)).double().cpu()


def _worst(e):
    """the largest entry; inf if any is not finite"""
    if e.numel() == 0:
        return 0.0
    return float(e.max()) if bool(torch.isfinite(e).all()) else float("inf")


def errors(got, ref, t, names=("row_loss", "mean", "lse", "dlogits", "rowsum", "zeros"), grad="dlogits"):
    """the figures of the module docstring; a value that is not finite where it is compared counts as infinite"""
    cnt, V, tier, g = ref["counted"], t["V"], t["tier"], abs(t["gscale"])
    fig = {}
    for name in ("row_loss", "mean", "lse"):
        if name in names and name in got:
            a, b = _f64(got[name]).reshape(-1), _f64(ref[name]).reshape(-1)
            if name == "lse":
                a, b = a[cnt], b[cnt]
            fig[name] = _worst((a - b).abs() / b.abs().clamp(min=1.0))
    if grad in got and ("dlogits" in names or "zeros" in names or "rowsum" in names):
        a, b = _f64(got[grad]), _f64(ref["dlogits"])
        live = a[cnt][:, :V]
        if "dlogits" in names:
            err = (live - b[cnt][:, :V]).abs()
            if tier == "bf16" and grad == "dlogits":
                err = (err - 2.0 ** -8 * b[cnt][:, :V].abs()).clamp(min=0.0)
            fig["dlogits"] = _worst(err / g)
        if "rowsum" in names and tier == "f32":
            fig["rowsum"] = _worst(live.sum(1).abs() / g)
        if "zeros" in names:
            dead = torch.cat([a[~cnt].reshape(-1), a[:, V:].reshape(-1), _f64(got["row_loss"])[~cnt]] if "row_loss" in got else
                             [a[~cnt].reshape(-1), a[:, V:].reshape(-1)])
            fig["zeros"] = _worst(dead.abs())
    return fig


def check(got, ref, t, what, gates=None):
    """asserts the reference finite, every compared value finite and every figure within its gate; returns the figures"""
    gates = gates or GATES[t["tier"]]
    for name in ("row_loss", "lse", "mean", "dlogits"):
        assert bool(torch.isfinite(_f64(ref[name])).all()), f"{what}: the reference's {name} is not finite"
    fig = errors(got, ref, t)
    for name, v in fig.items():
        assert math.isfinite(v), f"{what}: {name} is not finite"
        assert v <= gates[name], f"{what}: {name} {v:.3e} > {gates[name]:.2e}"
    return fig


def gate_cases(tier):
    """(regime, T, V, seed) of the gates' derivation"""
    cases = [(regime, 5, V, seed) for regime in regimes(tier) for V in GATE_VS for seed in range(5)]
    return cases + [("peaked", len(peak_positions(2059)), 2059, seed) for seed in range(5)]


@functools.lru_cache(maxsize=None)
def emulation_worst(tier):
    """the emulation's worst figure per measure against float64 over gate_cases; dlogits from the gradient before its rounding"""
    worst = {}
    for regime, T, V, seed in gate_cases(tier):
        t = regime_inputs(regime, T, V, ceil8(V) + 256, seed, tier)
        got, ref = emulate(t), reference(t)
        fig = errors(got, ref, t, names=("row_loss", "mean", "lse", "rowsum", "zeros"))
        fig.update(errors(got, ref, t, names=("dlogits",), grad="dlogits_f32"))
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


def report(entry, t, fig, **extra):
    kv = dict(entry=entry, regime=t["regime"], tier=t["tier"], V=t["V"], **extra)
    print("loss-regime-errors " + " ".join(f"{k}={v}" for k, v in kv.items()) + " " + " ".join(f"{k}={v:.2e}" for k, v in fig.items()))


# ------------------------------------------------------------------------------------------------------------------------------
# meant_ce_probs: CrossEntropyLoss (mean) on rows of probabilities, one thread per row
@functools.lru_cache(maxsize=None)
def ce_probs_inputs(kind, B, C, seed):
    """probs float32 [B, C], target int64 [B]"""
    assert kind in CE_PROBS_KINDS
    gen = torch.Generator().manual_seed(seed * 7919 + B * 131 + C)
    p = torch.rand(B, C, generator=gen)
    if kind == "zero_one":
        p = (p < 0.5).float()
        p[0] = 0.0
        p[-1] = 1.0
    elif kind == "shifted":
        p = p + 1000.0
    return p, torch.randint(0, C, (B,), generator=gen)


def ce_probs_reference(p, target):
    """float64: loss, dprobs [B, C]"""
    x = p.double()
    M = x.amax(1)
    logS = (x - M[:, None]).exp().sum(1).log()
    xt = x.gather(1, target[:, None])[:, 0]
    onehot = torch.zeros_like(x).scatter_(1, target[:, None], 1.0)
    return (logS + (M - xt)).mean(), (((x - M[:, None]) - logS[:, None]).exp() - onehot) / x.shape[0]


def emulate_ce_probs(p, target, one_float=False):
    """float32, the shift-invariant form: per row max, sum of exp(x - max), its log; the rows' terms added 64 at a time.
    one_float: logsumexp = max + log sum in one float, as ce_probs_kernel keeps it (its inputs are probabilities)"""
    x = p.float()
    B = x.shape[0]
    M = x.amax(1)
    e, S = (x - M[:, None]).exp(), torch.zeros(B)
    for c in range(x.shape[1]):                                        # one thread adds a row's terms one after the other
        S = S + e[:, c]
    logS = S.log()
    xt = x.gather(1, target[:, None])[:, 0]
    rows = ((M + logS) - xt if one_float else logS + (M - xt)) / B
    loss = torch.zeros(())
    for w in range(0, B, 64):
        loss = loss + rows[w:w + 64].sum()
    onehot = torch.zeros_like(x).scatter_(1, target[:, None], 1.0)
    soft = (x - (M + logS)[:, None]).exp() if one_float else ((x - M[:, None]) - logS[:, None]).exp()
    return loss, (soft - onehot) / B


def ce_probs_errors(loss, dprobs, ref_loss, ref_dprobs):
    fig = {"loss": _worst(((_f64(loss) - _f64(ref_loss)).abs() / _f64(ref_loss).abs().clamp(min=1.0)).reshape(1))}
    if dprobs is not None:
        fig["dprobs"] = _worst((_f64(dprobs) - _f64(ref_dprobs)).abs().reshape(-1) * dprobs.shape[0])
    return fig


def ce_probs_check(loss, dprobs, ref_loss, ref_dprobs, what, gates=None):
    gates = gates or CE_PROBS_GATES
    fig = ce_probs_errors(loss, dprobs, ref_loss, ref_dprobs)
    for name, v in fig.items():
        assert math.isfinite(v), f"{what}: {name} is not finite"
        assert v <= gates[name], f"{what}: {name} {v:.3e} > {gates[name]:.2e}"
    return fig
