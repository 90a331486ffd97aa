"""Shared helpers of the hard-label cross-entropy tests (test_ce_hard_host.py, test_gpu_ce_hard.py): the float64 reference of
F.cross_entropy(x, y, weight=, label_smoothing=, ignore_index=) with this project's conventions, a float32 host emulation of the
kernels' arithmetic (csrc/ce_hard.hip), the cases and the gates.

Reference (reference), float64, per row of logits x[0..C), target y, class weights w (ones without), W = sum w, smoothing eps:
  a row counts iff y != ignore_index and 0 <= y < C;  M = max x, S = sum exp(x - M), -logp_c = log S + (M - x_c)
  row_loss = (1 - eps) w_y (-logp_y) + (eps / C) (W log S + sum_c w_c (M - x_c)),  row_w = w_y
  grad_rows = d row_loss / d x = ((1 - eps) w_y + eps W / C) softmax - ((1 - eps) w_y onehot_y + (eps / C) w)
  loss = sum row_loss / sum row_w, and where that denominator is 0 (no row counts, or only rows of weight 0) loss = 0 with a
  zero gradient: the convention of ops.softmax_cross_entropy, not torch's NaN.  Rows that do not count: exact zeros, whatever
  they hold.  At eps == 0 the smoothing term is left out altogether, so a -inf logit is a masked column.
test_ce_hard_host.py holds this against F.cross_entropy in float64 ('none', 'sum', 'mean' and the autograd gradient).

Emulation (emulate), float32, of the three kernel shapes:
  "reg"     the class head up to C = 4096: lane i of a group of G = 64 (C <= 1024) or 256 takes columns i, i + G, ...; maximum, then
            per-lane sums of exp(x - M), w and w (M - x) in column order, butterflies over the 64 lanes, the four waves' sums as
            (0 + 1) + (2 + 3)
  "stream"  the class head above: 256 threads with a running (m, s, W, D) each, four columns 256 apart per step, single columns
            behind; all raised to the common maximum, then the same sums
  "vocab"   the large-vocabulary pair: the same running quadruple over 8-column chunks, 256 chunks apart, the ragged tail one
            column per thread; the gradient as exp((x - M) - log S)
and of the reduction (the rows' float32 values added in float64).

Error measures (errors):
  row_loss, loss   |err| / max(1, |ref|)
  grad             max |err| of the unnormalised gradient d row_loss / d x (the class head's dprobs as the entry leaves it; the
                   vocabulary backward's dlogits divided by |gscale|; in the bf16 tier less one bf16 rounding of the reference
                   element, 2^-8 |ref|).  The weights of the cases lie in [0, 2], so the scale of a gradient row is O(1)
  zeros            the largest magnitude where the reference has a structural zero (rows that do not count, padding columns): must be 0
  row_w            the number of rows whose row_w is not bit-equal to w_y (0 for the others): must be 0
Every gate is 4 x the emulation's worst figure against float64 over the gate cases, the margin tests/loss_ref.py takes for the
device's __expf / logf against the host's and for another merge order; test_ce_hard_host.py recomputes the figures and holds GATES
within [3.2 x, 8 x] of them.  Gate cases: "probs", every shape of PROBS_SHAPES x every kind of PROBS_KINDS x every option of
PROBS_OPTS; "f32" / "bf16", T = 5, every V of loss_ref.GATE_VS with ld = ceil8(V) + 256, every regime of loss_ref.regimes(tier),
every option of vocab_opts(regime) (eps = 0 alone on the two masked regimes), seed 0.  The bf16 tier's gradient figure is taken
before the gradient's rounding to bf16, which the measure already forgives.  Worst figures measured:
  probs  row_loss 2.17e-7, loss 1.29e-7, grad 2.78e-7
  f32    row_loss 1.97e-7, loss 1.35e-7, grad 3.62e-7
  bf16   row_loss 1.55e-7, loss 1.19e-7, grad 2.95e-7
"""
import functools
import math

import torch

from tests import loss_ref

NEG_INF = float("-inf")
IGNORE = -100
CUT_WAVE, CUT_REG = 1024, 4096                         # C <= 1024: "ce_hard_wave"; above: "ce_hard_block", the row in registers up to 4096
PROBS_SHAPES = [(1, 1), (3, 2), (5, 7), (4, 64), (4, 65), (7, 257), (4, 1024), (4, 1025), (130, 3129), (3, 4096), (2, 4097), (9, 64001)]
PROBS_KINDS = ("probs", "randn8", "shifted")
PROBS_OPTS = ((0.0, "rand"), (0.1, None), (0.1, "zeros"), (1.0, "rand"))          # (label_smoothing, weight kind)
VOCAB_T = 5
# 4 x the emulation's worst, rounded up to two digits (module docstring)
GATES = {"probs": {"row_loss": 8.7e-7, "loss": 5.2e-7, "grad": 1.2e-6, "zeros": 0.0, "row_w": 0.0},
         "f32": {"row_loss": 7.9e-7, "loss": 5.5e-7, "grad": 1.5e-6, "zeros": 0.0, "row_w": 0.0},
         "bf16": {"row_loss": 6.3e-7, "loss": 4.8e-7, "grad": 1.2e-6, "zeros": 0.0, "row_w": 0.0}}


def vocab_opts(regime):
    """(label_smoothing, weight kind) of a large-vocabulary case: a -inf column is outside the contract at eps > 0"""
    eps = (0.0,) if regime.startswith("masked") else (0.0, 0.1)
    return tuple((e, w) for e in eps for w in (None, "rand", "zeros"))


def counted(y, C, ignore_index):
    return (y != ignore_index) & (y >= 0) & (y < C) if ignore_index is not None else (y >= 0) & (y < C)


def make_weight(kind, C, seed):
    """None | "rand": 0.25 + 1.75 * rand | "zeros": the same with about a third of the classes at exactly 0 (class 0 always, where
    there is more than one class)"""
    if kind is None:
        return None
    g = torch.Generator().manual_seed(seed * 9176 + C)
    w = 0.25 + 1.75 * torch.rand(C, generator=g)
    if kind == "zeros":
        w = torch.where(torch.rand(C, generator=g) < 0.33, torch.zeros(C), w)
        if C > 1:
            w[0] = 0.0
    return w


@functools.lru_cache(maxsize=None)
def probs_inputs(B, C, kind):
    """probs float32 [B, C] and target int64 [B] of a class-head case: with three rows or more the last is ignored, with four or
    more the one before it holds a class index outside [0, C) -- C, -1 or 2^31 + 3 by (B + C)"""
    assert kind in PROBS_KINDS
    g = torch.Generator().manual_seed(B * 131 + C)
    p = torch.randn(B, C, generator=g) * 8 if kind == "randn8" else torch.rand(B, C, generator=g)
    if kind == "shifted":
        p = p + 1000.0
    y = torch.randint(0, C, (B,), generator=g)
    if B >= 3:
        y[B - 1] = IGNORE
    if B >= 4:
        y[B - 2] = (C, -1, 2 ** 31 + 3)[(B + C) % 3]
    return p, y


# ------------------------------------------------------------------------------------------------------------------------------
# float64 reference
def reference(x, y, w=None, eps=0.0, ignore_index=IGNORE):
    """dict of float64: row_loss [T], row_w [T], grad_rows [T, C] (d row_loss / d x), num, den, loss, grad [T, C] (d loss / d x),
    counted [T] and the three counts"""
    T, C = x.shape
    cnt = counted(y, C, ignore_index)
    x = torch.where(cnt[:, None], x.double(), torch.zeros(T, C, dtype=torch.float64))   # a row that does not count may hold anything
    wd = torch.ones(C, dtype=torch.float64) if w is None else w.double()
    yc = torch.where(cnt, y, torch.zeros_like(y))
    M = x.amax(1)
    logS = (x - M[:, None]).exp().sum(1).log()
    wy = wd[yc]
    a = (1.0 - eps) * wy
    nlp_y = logS + (M - x.gather(1, yc[:, None])[:, 0])
    soft = ((x - M[:, None]) - logS[:, None]).exp()
    onehot = torch.zeros_like(x).scatter_(1, yc[:, None], 1.0)
    row_loss, A, sub = a * nlp_y, a, a[:, None] * onehot
    if eps > 0:                                          # left out at eps == 0: 0 * inf under a masked column otherwise
        W = wd.sum()
        row_loss = row_loss + (eps / C) * (W * logS + (wd[None, :] * (M[:, None] - x)).sum(1))
        A = a + (eps / C) * W
        sub = sub + (eps / C) * wd[None, :]
    zero = torch.zeros(T, dtype=torch.float64)
    row_loss, row_w = torch.where(cnt, row_loss, zero), torch.where(cnt, wy, zero)
    grad_rows = torch.where(cnt[:, None], A[:, None] * soft - sub, torch.zeros_like(x))
    num, den = row_loss.sum(), row_w.sum()
    ok = bool(den != 0)
    ign = (y == ignore_index) if ignore_index is not None else torch.zeros_like(cnt)
    return dict(row_loss=row_loss, row_w=row_w, grad_rows=grad_rows, num=num, den=den, loss=num / den if ok else torch.zeros((), dtype=torch.float64),
                grad=grad_rows / den if ok else torch.zeros_like(grad_rows), counted=cnt, n_counted=int(cnt.sum()), n_ignored=int(ign.sum()),
                n_invalid=int((~cnt & ~ign).sum()))


# ------------------------------------------------------------------------------------------------------------------------------
# float32 host emulation
_LANE = torch.arange(64)


def _group_sum(v):
    """v float32 [..., G] with G = 64 or 256: the butterflies of a wave, then the four waves as (0 + 1) + (2 + 3)"""
    v = v.reshape(*v.shape[:-1], -1, 64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANE ^ o]
    v = v[..., 0]
    return v[..., 0] if v.shape[-1] == 1 else (v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])


def _emulate_reg(x, wcol, smooth):
    """(M, s, W, D) float32 [T] of the register forms"""
    T, C = x.shape
    G = 64 if C <= CUT_WAVE else 256
    xp = torch.full((T, 16 * G), NEG_INF)
    xp[:, :C] = x
    wp = torch.zeros(16 * G)
    wp[:C] = wcol
    inside = (torch.arange(16 * G) < C).view(16, G)
    xp, wp = xp.view(T, 16, G), wp.view(16, G)
    M = x.amax(1)
    s, W, D = torch.zeros(T, G), torch.zeros(T, G), torch.zeros(T, G)
    for u in range(16):
        s = s + (xp[:, u] - M[:, None]).exp()
        if smooth:
            W = W + wp[u]
            D = D + torch.where(inside[u], wp[u] * (M[:, None] - xp[:, u]), torch.zeros(T, G))
    return M, _group_sum(s), _group_sum(W), _group_sum(D)


def _steps(C, form):
    """the columns a thread takes, step by step: a list of int64 [256, k], -1 where the thread has no such step"""
    tid = torch.arange(256)
    steps = []
    if form == "stream":
        nfull = torch.clamp((C - 1 - 768 - tid) // 1024 + 1, min=0)              # steps with tid + 768 + 1024 n < C
        for n in range(int(nfull.max()) if C > 0 else 0):
            cols = n * 1024 + tid[:, None] + 256 * torch.arange(4)[None, :]
            steps.append(torch.where((n < nfull)[:, None], cols, torch.full_like(cols, -1)))
        for k in range(4):
            cols = nfull * 1024 + tid + 256 * k
            steps.append(torch.where(cols < C, cols, torch.full_like(cols, -1))[:, None])
    else:
        nchunk = C >> 3
        for n in range(-(-nchunk // 256)):
            c = n * 256 + tid
            cols = 8 * c[:, None] + torch.arange(8)[None, :]
            steps.append(torch.where((c < nchunk)[:, None], cols, torch.full_like(cols, -1)))
        cols = 8 * nchunk + tid
        steps.append(torch.where(cols < C, cols, torch.full_like(cols, -1))[:, None])
    return [s for s in steps if bool((s >= 0).any())]


def _emulate_online(x, wcol, smooth, form):
    """(M, s, W, D) float32 [T] of the running-quadruple forms"""
    T, C = x.shape
    m, s = torch.full((T, 256), NEG_INF), torch.zeros(T, 256)
    W, D = torch.zeros(T, 256), torch.zeros(T, 256)

    def raise_to(mn, real):
        nonlocal m, s, D
        up = real & (mn > m)
        scale = up & (m != NEG_INF)
        s = torch.where(scale, s * (m - mn).exp(), s)
        if smooth:
            D = torch.where(scale, D + W * (mn - m), D)
        m = torch.where(up, mn, m)

    for cols in _steps(C, form):
        real = cols[:, 0] >= 0
        safe = cols.clamp(min=0)
        v, wv = x[:, safe], wcol[safe]                                           # [T, 256, k], [256, k]
        raise_to(torch.where(real[None, :], v.amax(-1), torch.full((T, 256), NEG_INF)), real[None, :].expand(T, 256))
        for k in range(cols.shape[1]):
            mr = torch.where(m == NEG_INF, torch.zeros_like(m), m)
            s = torch.where(real, s + (v[..., k] - mr).exp(), s)
            if smooth:
                W = torch.where(real, W + wv[:, k], W)
                D = torch.where(real, D + wv[:, k] * (m - v[..., k]), D)
    M = m.amax(1)
    raise_to(M[:, None].expand(T, 256), torch.ones(T, 256, dtype=torch.bool))
    return M, _group_sum(s), _group_sum(W), _group_sum(D)


def emulate(x, y, w=None, eps=0.0, ignore_index=IGNORE, form=None):
    """what the kernels and the reduction give, in their float32 arithmetic: row_loss, row_w, grad_rows float32, loss float32, and M,
    logS of the rows; form: "reg" | "stream" (by C when None) | "vocab".  x is what the kernel reads, widened to float32"""
    T, C = x.shape
    form = form or ("reg" if C <= CUT_REG else "stream")
    cnt = counted(y, C, ignore_index)
    x = torch.where(cnt[:, None], x.float(), torch.zeros(T, C))
    smooth = eps > 0
    wcol = torch.ones(C) if w is None else w.float()
    e32 = torch.tensor(eps, dtype=torch.float32)
    M, s, W, D = _emulate_reg(x, wcol, smooth) if form == "reg" else _emulate_online(x, wcol, smooth, form)
    logS = s.log()
    yc = torch.where(cnt, y, torch.zeros_like(y))
    wy = wcol[yc]
    a = (1 - e32) * wy
    row_loss, A = a * (logS + (M - x.gather(1, yc[:, None])[:, 0])), a
    b = e32 / torch.tensor(float(C)) if smooth else torch.zeros(())
    if smooth:
        row_loss = row_loss + b * (W * logS + D)
        A = a + b * W
    sub = a[:, None] * torch.zeros(T, C).scatter_(1, yc[:, None], 1.0) + (b * wcol[None, :] if smooth else 0.0)
    if form == "vocab":
        grad = A[:, None] * ((x - M[:, None]) - logS[:, None]).exp() - sub
    else:
        grad = (A / s)[:, None] * (x - M[:, None]).exp() - sub
    zero = torch.zeros(T)
    row_loss, row_w = torch.where(cnt, row_loss, zero), torch.where(cnt, wy, zero)
    num, den = row_loss.double().sum(), row_w.double().sum()
    return dict(row_loss=row_loss, row_w=row_w, grad_rows=torch.where(cnt[:, None], grad, torch.zeros(T, C)),
                loss=(num / den).float() if bool(den != 0) else torch.zeros(()), M=M, logS=logS)


# ------------------------------------------------------------------------------------------------------------------------------
# comparison
def _f64(v):
    return (v.detach() if isinstance(v, torch.Tensor) else torch.tensor(v)).double().cpu()


def _worst(e):
    if e.numel() == 0:
        return 0.0
    return float(e.max()) if bool(torch.isfinite(e).all()) else float("inf")


def errors(got, ref, bf16_grad=False, w=None):
    """the figures of the module docstring for whatever of row_loss, loss, grad_rows [T, >= C], row_w `got` holds; a value that is
    not finite where it is compared counts as infinite"""
    cnt = ref["counted"]
    C = ref["grad_rows"].shape[1]
    fig, dead = {}, []
    for name in ("row_loss", "loss"):
        if name in got:
            a, b = _f64(got[name]).reshape(-1), _f64(ref[name]).reshape(-1)
            fig[name] = _worst((a - b).abs() / b.abs().clamp(min=1.0))
    if "row_loss" in got:
        dead.append(_f64(got["row_loss"])[~cnt])
    if "grad_rows" in got:
        a, b = _f64(got["grad_rows"]), ref["grad_rows"]
        err = (a[cnt][:, :C] - b[cnt]).abs()
        if bf16_grad:
            err = (err - 2.0 ** -8 * b[cnt].abs()).clamp(min=0.0)
        fig["grad"] = _worst(err)
        dead += [a[~cnt].reshape(-1), a[:, C:].reshape(-1)]
    if "row_w" in got:
        want = ref["row_w"].float()                      # w_y as the float32 weight holds it, 0 where the row does not count
        fig["row_w"] = float((got["row_w"].detach().cpu().float().view(torch.int32) != want.view(torch.int32)).sum())
    if dead:
        fig["zeros"] = _worst(torch.cat(dead).abs())
    return fig


def check(got, ref, tier, what, **kw):
    """asserts the reference finite, every compared value finite and every figure within its gate; returns the figures"""
    for name in ("row_loss", "loss", "grad_rows"):
        assert bool(torch.isfinite(ref[name]).all()), f"{what}: the reference's {name} is not finite"
    fig = errors(got, ref, **kw)
    for name, v in fig.items():
        assert math.isfinite(v), f"{what}: {name} is not finite"
        assert v <= GATES[tier][name], f"{what}: {name} {v:.3e} > {GATES[tier][name]:.2e}"
    return fig


def vocab_case(regime, V, tier, seed=0):
    """loss_ref.regime_inputs at T = 5, ld = ceil8(V) + 256, as it is"""
    return loss_ref.regime_inputs(regime, VOCAB_T, V, loss_ref.ceil8(V) + 256, seed, tier)


@functools.lru_cache(maxsize=None)
def emulation_worst(tier):
    """the emulation's worst figure per measure against float64 over the tier's gate cases"""
    worst = {}

    def take(got, ref):
        for k, v in errors(got, ref).items():
            worst[k] = max(worst.get(k, 0.0), v)

    if tier == "probs":
        for B, C in PROBS_SHAPES:
            for kind in PROBS_KINDS:
                p, y = probs_inputs(B, C, kind)
                for eps, wk in PROBS_OPTS:
                    w = make_weight(wk, C, B)
                    take(emulate(p, y, w, eps), reference(p, y, w, eps))
    else:
        for regime in loss_ref.regimes(tier):
            for V in loss_ref.GATE_VS:
                t = vocab_case(regime, V, tier)
                x = t["logits"][:, :V]
                for eps, wk in vocab_opts(regime):
                    w = make_weight(wk, V, V)
                    take(emulate(x, t["targets"], w, eps, t["ignore_index"], "vocab"), reference(x, t["targets"], w, eps, t["ignore_index"]))
    return worst
