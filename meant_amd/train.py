"""The train step around the hot path (reference: in_loop_train.py:202-239, 547-567).

Reference recipe: fp16 autocast + GradScaler, CrossEntropyLoss on the Sigmoid-ed output, clip_grad_norm_(1.0),
AdamW(lr 5e-5), CosineAnnealingWarmRestarts(T_0=7) stepped per epoch.  Here: bf16 compute needs no loss scaling,
and the tail of the step is three kinds of HIP launches over the flat fp32 buckets of the gradient reducer
(meant_amd/parallel.py) -- one sum-of-squares pass, one fused clip+AdamW pass per bucket -- instead of PyTorch's
per-tensor foreach chains.  Nothing in the step synchronises with the host.

The reference's own guard and its other driver choices are opt-in (GuardedAdam, through TrainStep(optimizer=, nonfinite=,
loss_scale=, clip_scaled=)): a step with an inf / NaN gradient is skipped, `-o Adam`, and the GradScaler recipe itself, with
the gradient statistics, the skip decision, the step count and the loss scale kept on the device; CosineAnnealing and LinearLR
are the driver's other two `-lrst` schedulers.
"""
from __future__ import annotations

import math
from typing import Iterable, Optional

import torch

from . import _lib, ops
from ._lib import lib, check
from .parallel import GradReducer


# ---------------------------------------------------------------------------------------------
class _CEOnProbs(torch.autograd.Function):
    """nn.CrossEntropyLoss()(probabilities, target), as in_loop_train.py:232 applies it to the Sigmoid output."""

    @staticmethod
    def forward(ctx, probs, target):
        ops._need_gpu(probs, target)
        p = ops._c(probs.float())
        t = ops._c(target.long())
        B, C = p.shape
        loss = torch.zeros(1, device=p.device, dtype=torch.float32)
        dp = torch.empty_like(p)
        check(lib.meant_ce_probs(ops._p(p), ops._p(t), ops._p(loss), ops._p(dp), B, C, ops._stream()), "ce_probs")
        ctx.save_for_backward(dp)
        return loss[0]

    @staticmethod
    def backward(ctx, dloss):
        (dp,) = ctx.saved_tensors
        return dp * dloss, None


class _CEOnProbsSoft(torch.autograd.Function):
    """nn.CrossEntropyLoss()(probabilities, class-probability target [B, C]), as vqa.py:173,209 applies it to the Sigmoid output
    with the answer weights of utils/custom_datasets.py:214-218: two launches (the rows, then their mean), no atomics."""

    @staticmethod
    def forward(ctx, probs, target):
        ops._need_gpu(probs, target)
        p = probs if probs.dtype == torch.float32 else probs.float()
        t = target if target.dtype in (torch.float32, torch.bfloat16) else target.float()
        B, C = p.shape
        (p, ldp), (t, ldt) = ops._rows(p), ops._rows(t)                     # column slices of wider blocks are read in place
        out = torch.empty(B + 1, device=p.device, dtype=torch.float32)      # row_loss [B], then the loss
        dp = torch.empty(B, C, device=p.device, dtype=torch.float32)
        check(lib.meant_ce_probs_soft(ops._p(p), ldp, ops._p(t), ldt, ops._dt(t), ops._p(out), out.data_ptr() + 4 * B, ops._p(dp), C, B, C,
                                      ops._stream()), "ce_probs_soft")
        ctx.save_for_backward(dp)
        return out[B]

    @staticmethod
    def backward(ctx, dloss):
        (dp,) = ctx.saved_tensors
        return dp * dloss, None


class _CEOnProbsHard(torch.autograd.Function):
    """F.cross_entropy(probabilities, target, weight=, label_smoothing=, ignore_index=) for class indices: the rows (loss, weight and
    the unnormalised gradient in one launch), then the ordered reduction into a device block.  No atomics, no host read."""

    @staticmethod
    def forward(ctx, probs, target, weight, eps, ignore_index):
        ops._need_gpu(probs, target, weight)
        p = probs if probs.dtype == torch.float32 else probs.float()
        t = ops._c(target.long())
        B, C = p.shape
        p, ldp = ops._rows(p)                                               # a column slice of a wider block is read in place
        n = ops.CE_STATS_FLOATS
        buf = torch.empty(n + 2 * B, device=p.device, dtype=torch.float32)  # the block, row_loss [B], row_w [B]
        dp = torch.empty(B, C, device=p.device, dtype=torch.float32)
        base = buf.data_ptr()
        check(lib.meant_ce_probs_hard(ops._p(p), ldp, ops._p(t), ops._p(weight), eps, ignore_index, base + 4 * n, base + 4 * (n + B),
                                      ops._p(dp), C, B, C, base, ops._stream()), "ce_probs_hard")
        ctx.save_for_backward(dp, buf)
        ctx.mark_non_differentiable(buf)
        return buf[0], buf

    @staticmethod
    def backward(ctx, dloss, _dbuf):
        dp, buf = ctx.saved_tensors
        return dp * (dloss * buf[1]), None, None, None, None               # buf[1]: 1 / sum of the counted rows' weights, or 0


def cross_entropy_on_probs(probs: torch.Tensor, target: torch.Tensor, *, weight=None, label_smoothing: float = 0.0,
                           ignore_index: Optional[int] = None) -> torch.Tensor:
    """nn.CrossEntropyLoss()(probs, target) of probabilities [B, C]: target [B] of class indices (any integer type), or a
    floating-point [B, C] of class probabilities / answer weights (rows need not sum to 1, may be all zero), read in place as
    float32 or bfloat16 with its row stride, any other float type widened to float32.
    weight ([C] class weights), label_smoothing (in [0, 1]) and ignore_index, for class indices: torch's
    CrossEntropyLoss(weight=, label_smoothing=, ignore_index=) -- sum(row_loss) / sum(w_target) over the rows whose target is not
    ignore_index and lies in [0, C).  Apart from torch: a target outside [0, C) is left out like an ignored one instead of raising,
    and where no row counts or the weights of those that do sum to 0 the loss is 0 with zero gradients, not NaN.  With all three
    at their defaults class indices take the plain kernel as before (a target outside [0, C) poisons its loss with NaN)."""
    plain = weight is None and label_smoothing == 0.0 and ignore_index is None
    if target.dtype.is_floating_point and target.dim() == 2:
        if not plain:
            raise ValueError("cross_entropy_on_probs: weight, label_smoothing and ignore_index go with class-index targets [B]; "
                             "class-probability targets [B, C] take none of them")
        if target.shape != probs.shape:
            raise ValueError(f"cross_entropy_on_probs: a class-probability target must have the shape of probs {tuple(probs.shape)}, "
                             f"got {tuple(target.shape)}")
        return _CEOnProbsSoft.apply(probs, target)
    if plain:
        return _CEOnProbs.apply(probs, target)
    if probs.dim() != 2 or target.dim() != 1 or target.shape[0] != probs.shape[0]:
        raise ValueError(f"cross_entropy_on_probs: probs [B, C] and target [B], got {tuple(probs.shape)} and {tuple(target.shape)}")
    w, eps = ops.ce_options(weight, label_smoothing, probs.shape[1], probs.device, "cross_entropy_on_probs")
    return _CEOnProbsHard.apply(probs, target, w, eps, ops.IGNORE_NONE if ignore_index is None else int(ignore_index))[0]


def balanced_class_weights(labels_or_counts: torch.Tensor, C: int, counts: bool = False) -> torch.Tensor:
    """float32 [C] of n / (C * count_c), sklearn's "balanced" class weights, 0 for a class without examples; on the device of the
    argument, with no host read.  labels_or_counts: integer labels of any shape (those outside [0, C) -- an ignore value -- are
    left out of the counts and of n), or, with counts=True, the [C] per-class counts themselves, e.g. the ntarget slice
    f1_metrics.state[2 * C:3 * C] of a first epoch, whose weights the next epoch's loss can take."""
    C = int(C)
    if C <= 0:
        raise ValueError(f"balanced_class_weights: C must be positive, got {C}")
    v = labels_or_counts if torch.is_tensor(labels_or_counts) else torch.as_tensor(labels_or_counts)
    if counts:
        if v.numel() != C:
            raise ValueError(f"balanced_class_weights: {C} class counts expected, got {tuple(v.shape)}")
        cnt = v.reshape(C).double()
    else:
        if v.dtype.is_floating_point or v.dtype == torch.bool:
            raise ValueError(f"balanced_class_weights: labels must be integers, got {v.dtype} (per-class counts go with counts=True)")
        lab = v.reshape(-1).long()
        ok = (lab >= 0) & (lab < C)
        cnt = torch.zeros(C, device=lab.device, dtype=torch.int64).scatter_add_(0, torch.where(ok, lab, torch.zeros_like(lab)),
                                                                                ok.long()).double()
    w = cnt.sum() / (C * cnt)
    return torch.where(cnt > 0, w, torch.zeros_like(w)).float()


# ---------------------------------------------------------------------------------------------
def flatten_parameters(reducer: GradReducer):
    """Make every parameter a view into a flat fp32 buffer laid out like its gradient bucket, so that one
    fused kernel can update a whole bucket.  Returns the list of flat parameter buffers (one per bucket)."""
    flats = []
    for b in reducer.buckets:
        flat = torch.zeros_like(b.flat)
        with torch.no_grad():
            for p, off in zip(b.params, b.offsets):
                n = p.numel()
                flat[off:off + n].copy_(p.detach().reshape(-1))
                p.data = flat[off:off + n].view_as(p)
        flats.append(flat)
    return flats


class FusedAdamW:
    """torch.optim.AdamW + torch.nn.utils.clip_grad_norm_ semantics on the reducer's flat buckets.

        red = GradReducer(model.parameters()); opt = FusedAdamW(red, lr=5e-5, max_grad_norm=1.0)
        red.prepare(); loss = f(model(x)); loss.backward(); red.wait(); opt.step()

    (`prepare()` comes BEFORE the forward pass: it also clears the per-step gradient-sink claims the forward's ops make.)
    `state_dict()` / `load_state_dict()` carry the step count, the learning rate and both moment buffers: a fresh optimizer over a
    model with the same parameter registration order continues exactly (checkpoint_train.py:217-219,333-336 of the reference
    saves and restores `optimizer.state_dict()` the same way)."""

    def __init__(self, reducer: GradReducer, lr: float = 5e-5, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, max_grad_norm: Optional[float] = None):
        self.reducer = reducer
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.max_grad_norm = max_grad_norm
        self.flat_params = flatten_parameters(reducer)
        self.exp_avg = [torch.zeros_like(f) for f in self.flat_params]
        self.exp_avg_sq = [torch.zeros_like(f) for f in self.flat_params]
        self.step_count = 0
        dev = self.flat_params[0].device if self.flat_params else torch.device("cuda")
        self._sumsq = torch.zeros(1, device=dev, dtype=torch.float32)

    @torch.no_grad()
    def step(self, grad_scale: float = 1.0):
        self.step_count += 1
        st = ops._stream()
        clip = self.max_grad_norm is not None and self.max_grad_norm > 0
        if clip:
            self._sumsq.zero_()
            for b in self.reducer.buckets:
                check(lib.meant_sumsq_f32(ops._p(b.flat), b.flat.numel(), ops._p(self._sumsq), st), "sumsq_f32")
        for b, p, m, v in zip(self.reducer.buckets, self.flat_params, self.exp_avg, self.exp_avg_sq):
            check(lib.meant_adamw_f32(ops._p(p), ops._p(b.flat), ops._p(m), ops._p(v), p.numel(), self.lr, self.betas[0],
                                      self.betas[1], self.eps, self.weight_decay, self.step_count,
                                      ops._p(self._sumsq) if clip else None, float(self.max_grad_norm or 0.0), float(grad_scale), st),
                  "adamw_f32")
        ops.weights.invalidate()        # parameters changed through raw pointers: drop the cached bf16 / transposed copies

    def grad_norm(self) -> torch.Tensor:
        """global L2 norm of the (already reduced) gradients, as a device scalar"""
        self._sumsq.zero_()
        for b in self.reducer.buckets:
            check(lib.meant_sumsq_f32(ops._p(b.flat), b.flat.numel(), ops._p(self._sumsq), ops._stream()), "sumsq_f32")
        return self._sumsq.sqrt()

    def state_dict(self):
        return {"step": self.step_count, "lr": self.lr, "exp_avg": [t.clone() for t in self.exp_avg],
                "exp_avg_sq": [t.clone() for t in self.exp_avg_sq]}

    def load_state_dict(self, sd):
        self.step_count, self.lr = sd["step"], sd["lr"]
        for d, s in zip(self.exp_avg, sd["exp_avg"]):
            d.copy_(s)
        for d, s in zip(self.exp_avg_sq, sd["exp_avg_sq"]):
            d.copy_(s)


class GuardedAdam:
    """The reference's guarded step on the reducer's flat buckets, with every decision taken on the device:
    `scaler.scale(loss).backward(); clip_grad_norm_; scaler.step(optimizer); scaler.update()` (in_loop_train.py:235-239) for
    `-o AdamW` and `-o Adam` (:548-550; Adam's weight_decay is L2 added to the gradient).

        red = GradReducer(model.parameters()); opt = GuardedAdam(red, kind="adam", loss_scale="dynamic", max_grad_norm=1.0)
        red.prepare(); loss = f(model(x)); opt.scale(loss).backward(); red.wait(); opt.step()

    A step whose reduced gradients hold an inf or a NaN changes no parameter and no moment and is counted as skipped; the step
    count (the bias corrections' t), the loss scale and its growth tracker live in a 64-byte state block on the device
    (include/meant_hip.h) that step() never reads back.  The statistics are taken after reducer.wait(), so every data-parallel
    rank takes the same decision.  loss_scale: None (no scaling, the guard alone), a float (a fixed scale) or "dynamic"
    (torch.amp.GradScaler's rule from init_scale).  clip_scaled=True clips the still-scaled gradients as the reference does
    (clip_grad_norm_ before scaler.step); False unscales first, the documented torch recipe."""

    KINDS = {"adamw": "OPTIM_ADAMW", "adam": "OPTIM_ADAM"}

    def __init__(self, reducer: GradReducer, kind: str = "adamw", lr: float = 5e-5, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, max_grad_norm: Optional[float] = None, clip_scaled: bool = False, loss_scale=None,
                 init_scale: float = 65536.0, growth_factor: float = 2.0, backoff_factor: float = 0.5, growth_interval: int = 2000):
        if kind not in self.KINDS:
            raise ValueError(f"GuardedAdam: kind must be one of {sorted(self.KINDS)}, got {kind!r}")
        if not (loss_scale is None or loss_scale == "dynamic" or (isinstance(loss_scale, (int, float)) and loss_scale > 0)):
            raise ValueError(f"GuardedAdam: loss_scale must be None, a positive number or 'dynamic', got {loss_scale!r}")
        self.reducer, self.kind, self._kind = reducer, kind, getattr(_lib, self.KINDS[kind])
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.max_grad_norm, self.clip_scaled = max_grad_norm, bool(clip_scaled)
        self.dynamic = loss_scale == "dynamic"
        self.growth_factor, self.backoff_factor, self.growth_interval = growth_factor, backoff_factor, int(growth_interval)
        self.flat_params = flatten_parameters(reducer)
        self.exp_avg = [torch.zeros_like(f) for f in self.flat_params]
        self.exp_avg_sq = [torch.zeros_like(f) for f in self.flat_params]
        dev = self.flat_params[0].device if self.flat_params else torch.device("cuda")
        self.state = torch.zeros(_lib.OPTIM_STATE_BYTES, device=dev, dtype=torch.uint8)
        self._i64, self._f32, self._i32 = self.state.view(torch.int64), self.state.view(torch.float32), self.state.view(torch.int32)
        self._scale = self._f32[8]                       # offset 32: a 0-dim view, read by scale() on the device
        self._scaling = loss_scale is not None
        self._scale.fill_(float(init_scale) if self.dynamic else float(loss_scale or 1.0))
        nmax = max((b.flat.numel() for b in reducer.buckets), default=0)
        self._ws = torch.empty(max(16, lib.meant_grad_stats_ws(nmax)), device=dev, dtype=torch.uint8)

    def scale(self, loss: torch.Tensor) -> torch.Tensor:
        """loss * scale with the scale read on the device; the loss itself when no loss scaling was asked for"""
        return loss * self._scale if self._scaling else loss

    @torch.no_grad()
    def step(self):
        st, state, first = ops._stream(), ops._p(self.state), 1
        for b in self.reducer.buckets:
            if b.flat.numel() == 0:
                continue
            check(lib.meant_grad_stats_f32(ops._p(b.flat), b.flat.numel(), state, first, ops._p(self._ws), self._ws.numel(), st),
                  "grad_stats_f32")
            first = 0
        for b, p, m, v in zip(self.reducer.buckets, self.flat_params, self.exp_avg, self.exp_avg_sq):
            check(lib.meant_optim_step_f32(ops._p(p), ops._p(b.flat), ops._p(m), ops._p(v), p.numel(), self._kind, self.lr,
                                           self.betas[0], self.betas[1], self.eps, self.weight_decay, float(self.max_grad_norm or 0.0),
                                           int(self.clip_scaled), state, st), "optim_step_f32")
        check(lib.meant_optim_finish(state, self.growth_factor, self.backoff_factor, self.growth_interval, int(self.dynamic), st),
              "optim_finish")
        ops.weights.invalidate()        # always: the host does not know whether the step was taken

    # the readers below copy from the device, and only when called
    def get_scale(self) -> float:
        s = self._scale.item()
        return s if s != 0.0 else 1.0

    def growth_tracker(self) -> int:
        return int(self._i32[9].item())

    def steps_taken(self) -> int:
        return int(self._i64[2].item())

    def steps_skipped(self) -> int:
        return int(self._i64[3].item())

    def last_skipped(self) -> bool:
        return bool(self._i32[11].item())

    def last_grad_norm(self) -> float:
        """global norm of the unscaled gradients of the last step taken"""
        return self._f32[10].item()

    def state_dict(self):
        return {"kind": self.kind, "state": self.state.clone(), "lr": self.lr, "exp_avg": [t.clone() for t in self.exp_avg],
                "exp_avg_sq": [t.clone() for t in self.exp_avg_sq]}

    def load_state_dict(self, sd):
        """a GuardedAdam state dict, or a FusedAdamW one: its `step` becomes the steps taken, the scale stays as constructed"""
        if "state" in sd:
            self.state.copy_(sd["state"])
        else:
            scale = self._scale.clone()
            self.state.zero_()
            self._scale.copy_(scale)
            self._i64[2].fill_(int(sd["step"]))
        self.lr = sd["lr"]
        for d, s in zip(self.exp_avg, sd["exp_avg"]):
            d.copy_(s)
        for d, s in zip(self.exp_avg_sq, sd["exp_avg_sq"]):
            d.copy_(s)


class _EpochSchedule:
    """a learning rate that is a function of the epoch, stepped once per epoch (in_loop_train.py:280): lr_at(epoch) and the keys
    of state_dict() come from the subclass"""
    KEYS = ()

    def step(self):
        self.epoch += 1
        self.opt.lr = self.lr_at(self.epoch)

    def state_dict(self):
        return {k: getattr(self, k) for k in ("epoch", "base_lr") + self.KEYS}

    def load_state_dict(self, sd):
        for k in ("epoch", "base_lr") + self.KEYS:
            setattr(self, k, sd[k])
        self.opt.lr = self.lr_at(self.epoch)


class CosineAnnealing(_EpochSchedule):
    """torch.optim.lr_scheduler.CosineAnnealingLR(T_max, eta_min) (in_loop_train.py:563), in its closed form:
    lr(e) = eta_min + (base - eta_min) * (1 + cos(pi * e / T_max)) / 2, periodic past T_max as torch's is."""
    KEYS = ("T_max", "eta_min")

    def __init__(self, optimizer, T_max: int, eta_min: float = 0.0):
        self.opt, self.T_max, self.eta_min = optimizer, T_max, eta_min
        self.base_lr = optimizer.lr
        self.epoch = 0

    def lr_at(self, epoch: int) -> float:
        return self.eta_min + (self.base_lr - self.eta_min) * (1 + math.cos(math.pi * epoch / self.T_max)) / 2


class LinearLR(_EpochSchedule):
    """torch.optim.lr_scheduler.LinearLR (in_loop_train.py:565 builds it with torch's defaults, which are the defaults here):
    lr(e) = base * (start_factor + (end_factor - start_factor) * min(e, total_iters) / total_iters).  The learning rate is set to
    base * start_factor at construction, as torch's scheduler does."""
    KEYS = ("start_factor", "end_factor", "total_iters")

    def __init__(self, optimizer, start_factor: float = 1.0 / 3, end_factor: float = 1.0, total_iters: int = 5):
        self.opt, self.start_factor, self.end_factor, self.total_iters = optimizer, start_factor, end_factor, total_iters
        self.base_lr = optimizer.lr
        self.epoch = 0
        optimizer.lr = self.lr_at(0)

    def lr_at(self, epoch: int) -> float:
        return self.base_lr * (self.start_factor + (self.end_factor - self.start_factor) * min(epoch, self.total_iters) / self.total_iters)


class CosineWarmRestarts:
    """torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(T_0, T_mult=1, eta_min) stepped once per epoch
    (in_loop_train.py:567, :280): lr(e) = eta_min + (base - eta_min) * (1 + cos(pi * (e mod T_0) / T_0)) / 2."""

    def __init__(self, optimizer: FusedAdamW, T_0: int = 7, eta_min: float = 0.0):
        self.opt, self.T_0, self.eta_min = optimizer, T_0, eta_min
        self.base_lr = optimizer.lr
        self.epoch = 0

    def lr_at(self, epoch: int) -> float:
        t = epoch % self.T_0
        return self.eta_min + (self.base_lr - self.eta_min) * (1 + math.cos(math.pi * t / self.T_0)) / 2

    def step(self):
        self.epoch += 1
        self.opt.lr = self.lr_at(self.epoch)

    def state_dict(self):
        return {"epoch": self.epoch, "base_lr": self.base_lr, "T_0": self.T_0, "eta_min": self.eta_min}

    def load_state_dict(self, sd):
        self.epoch, self.base_lr, self.T_0, self.eta_min = sd["epoch"], sd["base_lr"], sd["T_0"], sd["eta_min"]
        self.opt.lr = self.lr_at(self.epoch)


class TrainStep:
    """forward -> CE on probabilities -> backward (+ overlapped gradient all-reduce) -> clip + AdamW.

    step(*inputs, target=...): target is [B] class indices (in_loop_train.py:232) or a floating-point [B, C] of class
    probabilities / answer weights, the soft labels of the VQA loop (vqa.py:173,209) -- cross_entropy_on_probs picks the loss
    by the target's type; micro-batches slice either kind along the batch axis."""

    def __init__(self, model: torch.nn.Module, lr: float = 5e-5, weight_decay: float = 1e-2, max_grad_norm: float = 1.0,
                 bucket_mb: float = 64.0, direct_grads: bool = True, micro_batches: int = 1, metrics=None,
                 optimizer: str = "adamw", nonfinite: Optional[str] = None, loss_scale=None, clip_scaled: bool = False,
                 class_weight=None, label_smoothing: float = 0.0, ignore_index: Optional[int] = None):
        """micro_batches: run a step's batch as this many equal slices, one forward/backward each, gradients accumulated in the
        reducer's buckets (reducer.no_sync) -- the same gradients with 1/micro_batches of the activations in flight (the
        reference's CLI default of 12 encoder layers at 128 samples per GPU).
        direct_grads (GradReducer): parameter gradients are accumulated straight into the flat buckets by the backward
        kernels; pass False if the model's parameters are also differentiated outside this step (torch.autograd.grad,
        several backward passes per optimizer step without reducer.no_sync())
        metrics (meant_amd.metrics.f1_metrics, vqa_score for soft [B, C] targets, a metric_group, or None): when given, every step
        adds its batch to it -- metrics.update(out, target) on the detached output, one more launch and no host read; None leaves
        the step's launches as they are
        optimizer ("adamw" | "adam", the driver's -o), nonfinite (None | "skip"), loss_scale (None | float | "dynamic"), clip_scaled:
        with the defaults the tail is FusedAdamW, unguarded; optimizer="adam", nonfinite="skip" or any loss_scale builds GuardedAdam
        instead -- a step with an inf or NaN gradient (a class index outside [0, C) poisons one, as does an overflow) is skipped on
        the device and counted (opt.steps_skipped()), every micro-batch's loss goes through opt.scale() before backward, and the
        loss returned stays the unscaled one
        class_weight ([C]), label_smoothing, ignore_index: the arguments of cross_entropy_on_probs for class-index targets (the
        weight is kept as a float32 tensor on the model's device; balanced_class_weights makes one from labels or counts).  Each
        micro-batch is normalised by its OWN denominator -- the weights of its counted rows -- and scaled by 1 / micro_batches:
        with weights or ignored rows that is the mean of the micro-batches' weighted means, not the weighted mean of the whole
        batch (the two agree when every micro-batch has the same denominator)"""
        if optimizer not in ("adamw", "adam"):
            raise ValueError(f"TrainStep: optimizer must be 'adamw' or 'adam', got {optimizer!r}")
        if nonfinite not in (None, "skip"):
            raise ValueError(f"TrainStep: nonfinite must be None or 'skip', got {nonfinite!r}")
        self.model = model
        self.reducer = GradReducer(model.parameters(), bucket_mb=bucket_mb, direct_grads=direct_grads)
        if optimizer == "adamw" and nonfinite is None and loss_scale is None:
            self.opt = FusedAdamW(self.reducer, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
            self._scale = None
        else:
            self.opt = GuardedAdam(self.reducer, kind=optimizer, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                                   clip_scaled=clip_scaled, loss_scale=loss_scale)
            self._scale = self.opt.scale
        self.micro_batches = max(1, int(micro_batches))
        self.metrics = metrics
        self.label_smoothing = float(label_smoothing)
        self.ignore_index = None if ignore_index is None else int(ignore_index)
        self.class_weight = None
        if class_weight is not None:
            dev = next((p.device for p in model.parameters()), None)
            w = class_weight if torch.is_tensor(class_weight) else torch.as_tensor(class_weight, dtype=torch.float32)
            self.class_weight = ops.ce_options(w, self.label_smoothing, w.numel(), dev, "TrainStep")[0]
        else:
            ops.ce_options(None, self.label_smoothing, 0, None, "TrainStep")

    def _loss(self, out, target):
        return cross_entropy_on_probs(out, target, weight=self.class_weight, label_smoothing=self.label_smoothing,
                                      ignore_index=self.ignore_index)

    def __call__(self, *inputs, target):
        self.reducer.prepare()
        k = self.micro_batches
        if k == 1:
            out = self.model(*inputs)
            loss = self._loss(out, target)
            (loss if self._scale is None else self._scale(loss)).backward()
        else:
            B = target.shape[0]
            assert B % k == 0, "micro_batches must divide the batch"
            mb, outs, loss = B // k, [], 0.0
            for i in range(k):
                sl = slice(i * mb, (i + 1) * mb)
                part = tuple(t[sl] if torch.is_tensor(t) else t for t in inputs)
                if i < k - 1:
                    with self.reducer.no_sync():
                        o = self.model(*part)
                        li = self._loss(o, target[sl]) * (1.0 / k)
                        (li if self._scale is None else self._scale(li)).backward()
                else:
                    o = self.model(*part)
                    li = self._loss(o, target[sl]) * (1.0 / k)
                    (li if self._scale is None else self._scale(li)).backward()
                outs.append(o.detach())
                loss = loss + li.detach()
            out = torch.cat(outs)
        self.reducer.wait()
        self.opt.step()
        if self.metrics is not None:
            self.metrics.update(out.detach(), target)
        return loss.detach(), out.detach()


def evaluate(model: torch.nn.Module, batches: Iterable, metrics, target_index: int = -1):
    """Score `batches` with `model` into `metrics` (the validation / test loops of in_loop_train.py:281-319, 339-359): the model
    in eval() mode under torch.no_grad(), one forward and one metrics.update per batch, no host read; the model's previous
    training flag is restored at the end.  A batch is a sequence of tensors: the one at `target_index` is the target, the
    others are the model's positional inputs in order.  Returns `metrics`; read it with metrics.compute() / show()."""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for batch in batches:
                batch = list(batch)
                target = batch.pop(target_index)
                metrics.update(model(*batch), target)
    finally:
        model.train(was_training)
    return metrics
