"""Classification metrics counted on the device (reference: utils/f1_metrics.py, fed at in_loop_train.py:208-241, 281-319, 339-359).

The reference class wraps seven torchmetrics objects and is handed `out.detach().cpu()` every step: one full drain of the device
per batch, and a second one for `torch.isnan(out).any()` (in_loop_train.py:228).  Here `update` is one HIP launch
(meant_metrics_update) that adds the batch's counts to an int64 state on the device, and only `compute()` / `show()` read it.

    m = f1_metrics(num_classes=2, set_name="Train")
    for batch in loader:
        loss, out = step(*batch.inputs, target=batch.target)
        m.update(out, batch.target)          # launches and returns
    m.show(); assert m.nan_rows() == 0; m.reset()

State layout (include/meant_hip.h): int64 [3C + 4] = tp[C], npred[C], ntarget[C], n_rows, n_ignored, n_invalid, n_nan.  All
integers and only ever added to: two runs give the same bits, and a multi-GPU caller may `all_reduce` `m.state` as it is.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from ._lib import lib, check


def _split(state: torch.Tensor, C: int):
    if state.dtype != torch.int64 or state.numel() != 3 * C + 4:
        raise ValueError(f"f1_metrics: the state of {C} classes is int64 [{3 * C + 4}], got {state.dtype} [{state.numel()}]")
    s = state.detach().reshape(-1).cpu()
    return s[:C].double(), s[C:2 * C].double(), s[2 * C:3 * C].double(), s[3 * C:]


def _ratio(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
    """num / den, 0 where den == 0"""
    return torch.where(den > 0, num / den.clamp(min=1), torch.zeros_like(num))


class f1_metrics:
    """The reference class's surface (`update`, `compute`, `show`, `set_name`) on device counts.

    update(pred, target): pred [B, C] float32 / bfloat16 / float16 scores (the prediction is `pred.argmax(dim=1)` as torch computes
    it: lowest index on a tie, a NaN above everything) or [B] integer labels; target [B] integer.  A row whose target is
    `ignore_index` is left out, one whose target (or label) is otherwise outside [0, C) is counted in `invalid_rows()` and left
    out.  float16 scores are widened to float32 on the device: that is exact, whereas bfloat16 would drop three mantissa bits and
    could turn two different scores into a tie, i.e. change the prediction.  Tensors on the CPU (the reference loop hands over
    `.cpu()` copies) are copied to the current device; the counting always runs there.

    `state` (int64 [3C + 4], a plain device tensor) and the confusion matrix are allocated by the first `update`, on its tensors'
    device, or at construction with `device=`; `compute()` / `show()` / `per_class()` / `confusion_matrix()` each make one copy of
    them to the host, `nan_rows()` / `invalid_rows()` read one counter, and nothing else reads the device.

    absent_classes: how the macro averages treat a class that occurs neither in the predictions nor in the targets.  "skip"
    (default) leaves it out of the mean; this is, to the best of our reading, what the torchmetrics release the reference pins
    (1.3.0.post0) does -- torchmetrics was not available to check it against.  "zero" counts it as 0, as scikit-learn does with
    zero_division=0.  The two agree whenever every class occurs.
    """

    def __init__(self, num_classes: int, set_name: str, ignore_index: int = -100, confusion: bool = False,
                 absent_classes: str = "skip", device=None):
        if num_classes <= 0:
            raise ValueError("f1_metrics: num_classes must be positive")
        if absent_classes not in ("skip", "zero"):
            raise ValueError("f1_metrics: absent_classes is 'skip' or 'zero'")
        self.num_classes, self.set_name = int(num_classes), set_name
        self.ignore_index, self.absent_classes = int(ignore_index), absent_classes
        self._want_confusion = bool(confusion)
        self.state: Optional[torch.Tensor] = None        # allocated on the first update's device (or `device`)
        self._confusion: Optional[torch.Tensor] = None
        if device is not None:
            self._alloc(torch.device(device))

    # ---- device side ----------------------------------------------------------------------------
    def _alloc(self, device):
        C = self.num_classes
        self.state = torch.zeros(3 * C + 4, dtype=torch.int64, device=device)
        if self._want_confusion:
            self._confusion = torch.zeros(C, C, dtype=torch.int64, device=device)

    def update(self, pred: torch.Tensor, target: torch.Tensor) -> None:
        C = self.num_classes
        if not pred.is_cuda or not target.is_cuda:
            dev = pred.device if pred.is_cuda else target.device if target.is_cuda else torch.device("cuda", torch.cuda.current_device())
            pred, target = pred.to(dev), target.to(dev)
        ops._need_gpu(pred, target)
        if self.state is None:
            self._alloc(pred.device)
        ops._need_gpu(self.state)
        pred = pred.detach()
        if target.dtype.is_floating_point or target.dtype == torch.bool:
            raise TypeError("f1_metrics: target must be an integer tensor")
        target = ops._c(target.reshape(-1).long())
        B = target.shape[0]
        st = ops._stream()
        if pred.dtype.is_floating_point:
            if pred.dim() != 2 or pred.shape[0] != B or pred.shape[1] != C:
                raise ValueError(f"f1_metrics: scores must be [{B}, {C}], got {tuple(pred.shape)}")
            if pred.dtype not in (torch.float32, torch.bfloat16):
                pred = pred.float()                      # float16 (exact), float64
            if pred.stride(1) != 1 or (B > 1 and pred.stride(0) < C):
                pred = pred.contiguous()
            ld = pred.stride(0) if B > 1 else max(C, pred.stride(0))     # a column slice of a padded logits block is read in place
            check(lib.meant_metrics_update(ops._p(pred), ld, ops._dt(pred), ops._p(target), B, C, self.ignore_index,
                                           ops._p(self.state), ops._p(self._confusion), st), "metrics_update")
        else:
            if pred.dtype == torch.bool or pred.numel() != B:
                raise ValueError(f"f1_metrics: labels must be {B} integers, got {pred.dtype} {tuple(pred.shape)}")
            pred = ops._c(pred.reshape(-1).long())
            check(lib.meant_metrics_update_labels(ops._p(pred), ops._p(target), B, C, self.ignore_index, ops._p(self.state),
                                                  ops._p(self._confusion), st), "metrics_update_labels")

    def reset(self) -> None:
        if self.state is not None:
            self.state.zero_()
        if self._confusion is not None:
            self._confusion.zero_()

    def merge(self, other: "f1_metrics") -> "f1_metrics":
        """add another object's counts (same classes) to this one's, on this one's device"""
        if other.num_classes != self.num_classes:
            raise ValueError("f1_metrics.merge: different num_classes")
        if other.state is None:
            return self
        if self.state is None:
            self._alloc(other.state.device)
        self.state += other.state.to(self.state.device)
        if self._confusion is not None:
            if other._confusion is None:
                raise ValueError("f1_metrics.merge: the other object kept no confusion matrix")
            self._confusion += other._confusion.to(self._confusion.device)
        return self

    # ---- host side: each call below makes one copy of the state ------------------------------------
    def _host_state(self) -> torch.Tensor:
        if self.state is None:
            return torch.zeros(3 * self.num_classes + 4, dtype=torch.int64)
        return self.state.cpu()

    def compute(self):
        """(accuracy, f1 macro, f1 micro, precision macro, precision micro, recall macro, recall micro), 0-d float32 tensors"""
        return tuple(v.float() for v in self.from_counts(self._host_state(), self.num_classes, self.absent_classes))

    def per_class(self):
        """precision, recall, F1 (float64 [C]) and support = ntarget (int64 [C])"""
        return self.per_class_from_counts(self._host_state(), self.num_classes)

    def _tail(self, k: int) -> int:
        return 0 if self.state is None else int(self.state[3 * self.num_classes + k].item())

    def nan_rows(self) -> int:
        """counted rows with a NaN among their class scores (the reference's per-step `torch.isnan(out).any()`, once per epoch)"""
        return self._tail(3)

    def invalid_rows(self) -> int:
        return self._tail(2)

    def confusion_matrix(self) -> torch.Tensor:
        """int64 [C, C] on the CPU, row = target, column = prediction"""
        if not self._want_confusion:
            raise RuntimeError("f1_metrics: built without confusion=True")
        C = self.num_classes
        return torch.zeros(C, C, dtype=torch.int64) if self._confusion is None else self._confusion.cpu()

    def show(self, _class=None):
        state = self._host_state()
        (accuracy, f1_macro, f1_micro, precision_macro, precision_micro, recall_macro,
         recall_micro) = (v.float() for v in self.from_counts(state, self.num_classes, self.absent_classes))
        print(self.set_name + ' accuracy: ', accuracy)
        print('Macro ' + self.set_name + ' f1: ', f1_macro)
        print('Micro ' + self.set_name + ' f1: ', f1_micro)
        print('Macro ' + self.set_name + ' precision: ', precision_macro)
        print('Micro ' + self.set_name + ' precision: ', precision_micro)
        print('Macro ' + self.set_name + ' recall: ', recall_macro)
        print('Micro ' + self.set_name + ' recall: ', recall_micro)
        if _class is not None:
            # the reference indexes its 0-d averages here (f1_macro[_class]), which cannot run; the class's own values instead
            p, r, f1, _ = self.per_class_from_counts(state, self.num_classes)
            print(self.set_name + ' f1 for class ' + str(_class), f1[_class].item())
            print(self.set_name + ' precision for class ' + str(_class), p[_class].item())
            print(self.set_name + ' recall for class ' + str(_class), r[_class].item())
        return f1_macro, f1_micro

    # ---- finalisation: pure torch on the CPU ------------------------------------------------------------
    @staticmethod
    def per_class_from_counts(state: torch.Tensor, C: int):
        tp, npred, ntarget, _ = _split(state, C)
        return _ratio(tp, npred), _ratio(tp, ntarget), _ratio(2 * tp, npred + ntarget), ntarget.long()

    @staticmethod
    def from_counts(state: torch.Tensor, C: int, absent_classes: str = "skip"):
        """The seven values, as 0-d float64 tensors, from a state tensor: per class p = tp / npred, r = tp / ntarget,
        f1 = 2 tp / (npred + ntarget), 0 where the denominator is 0; accuracy = micro F1 = micro precision = micro recall =
        sum(tp) / n_rows (equal for single-label multiclass); macro = the mean over the classes, those with
        npred + ntarget == 0 left out ("skip") or counted as 0 ("zero").  Nothing counted: all zeros."""
        if absent_classes not in ("skip", "zero"):
            raise ValueError("f1_metrics: absent_classes is 'skip' or 'zero'")
        tp, npred, ntarget, tail = _split(state, C)
        p, r, f1 = _ratio(tp, npred), _ratio(tp, ntarget), _ratio(2 * tp, npred + ntarget)
        n_rows = tail[0].double()
        micro = _ratio(tp.sum(), n_rows)
        present = (npred + ntarget) > 0 if absent_classes == "skip" else torch.ones(C, dtype=torch.bool)
        n = present.sum().double()
        macro = lambda x: _ratio((x * present).sum(), n)
        return micro, macro(f1), micro.clone(), macro(p), micro.clone(), macro(r), micro.clone()
