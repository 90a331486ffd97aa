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

The paper's other two numbers (train.py:63-65, 103-117): the Matthews coefficient follows from the same counts (`f1_metrics.mcc()`);
the AUROC is a rank statistic and needs the scores, which `auroc.update` keeps on the device (meant_score_capture, one launch) until
`auroc.statistic()` sorts them there and counts the Mann-Whitney statistic exactly (meant_auroc_rank).  `metric_group` feeds several
such objects from one `TrainStep(metrics=...)` / `train.evaluate`.

meant_vqa's labels are soft: a float [B, C] row of answer weights per question (utils/custom_datasets.py:214-218).  `f1_metrics`
refuses them; `vqa_score` counts the number VQA results are reported in, the weight of the predicted answer averaged over the
questions, the same way: one launch per batch (meant_vqa_score_update), integers only, read by `compute()` / `show()`.
"""
from __future__ import annotations

from typing import Optional

import math

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

    def mcc(self) -> torch.Tensor:
        """Matthews correlation coefficient of the counted rows (multiclass form; at C = 2 the binary one), a 0-d float32 tensor"""
        return self.mcc_from_counts(self._host_state(), self.num_classes).float()

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
    def mcc_from_counts(state: torch.Tensor, C: int) -> torch.Tensor:
        """(c s - sum_k npred_k ntarget_k) / sqrt((s^2 - sum_k npred_k^2) (s^2 - sum_k ntarget_k^2)) with c = sum(tp) and s = n_rows, as
        a 0-d float64 tensor; 0 where the denominator is 0 (nothing counted, one class predicted throughout, one class the only
        target), as scikit-learn's matthews_corrcoef returns.  The sums are exact in float64 while s^2 stays below 2^53."""
        tp, npred, ntarget, tail = _split(state, C)
        c, s = tp.sum(), tail[0].double()
        num = c * s - (npred * ntarget).sum()
        den = (s * s - (npred * npred).sum()) * (s * s - (ntarget * ntarget).sum())
        return num / den.sqrt() if den.item() > 0 else torch.zeros((), dtype=torch.float64)

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


class auroc:
    """Area under the ROC curve from scores kept on the device (the reference's torchmetrics AUROC, utils/f1_metrics.py:3).

    update(pred, target): the tensors `f1_metrics.update` takes for scores -- pred [B, C] float32 / bfloat16 (float16 and float64
    through `.float()`), target [B] integer -- or, at num_classes == 2, pred [B]: the score of the positive class.  One launch
    (meant_score_capture) appends the batch to the device buffers: at num_classes == 2 the column `pos_label`, otherwise all C
    columns, each class against the rest.  A row whose target is `ignore_index`, whose target is otherwise outside [0, C)
    (`invalid_rows()`) or with a NaN among its captured scores (`nan_rows()`) is left out.  The buffers double when full, by device
    copies sized from the host's own row count: `update` never reads the device.

    statistic(): int64 [ncol, 3] on the CPU, per captured column (2U, P, N): P positives, N negatives and twice the Mann-Whitney
    statistic, 2U = sum over (positive, negative) pairs of 2 [negative's score below] + [scores equal] -- exact integers
    (meant_auroc_rank: a radix sort and integer scans on the device), the same bits for any batching.  The one place that reads back.
    per_class(): float64 [ncol], 2U / (2 P N), NaN where P or N is 0.  compute(): a 0-d float32 tensor: that value at
    num_classes == 2, otherwise the mean over the classes that have both a positive and a negative (macro average); NaN when no
    class has both -- the area is undefined then (scikit-learn raises; torchmetrics could not be consulted for its convention).
    -0.0 and +0.0 tie; scores are compared as float32 (bfloat16 widened exactly).
    """

    def __init__(self, num_classes: int = 2, set_name: str = "", pos_label: int = 1, ignore_index: int = -100, capacity: int = 65536,
                 device=None):
        if num_classes < 2:
            raise ValueError("auroc: num_classes must be at least 2")
        if num_classes == 2 and pos_label not in (0, 1):
            raise ValueError("auroc: pos_label is 0 or 1")
        if capacity <= 0:
            raise ValueError("auroc: capacity must be positive")
        self.num_classes, self.set_name = int(num_classes), set_name
        self.pos_label, self.ignore_index = int(pos_label), int(ignore_index)
        self.ncol = 1 if self.num_classes == 2 else self.num_classes
        self.capacity = int(capacity)
        self.count = 0                                   # slots handed out so far: the host's own sum of the batch sizes
        self.keys: Optional[torch.Tensor] = None         # int32 [ncol, capacity] holding the uint32 keys, class-major
        self.labels: Optional[torch.Tensor] = None       # int32 [capacity], -1 = left out
        self.counters: Optional[torch.Tensor] = None     # int64 [4] = n_rows, n_ignored, n_invalid, n_nan
        if device is not None:
            self._alloc(torch.device(device))

    # ---- device side ----------------------------------------------------------------------------
    def _alloc(self, device):
        self.keys = torch.empty(self.ncol, self.capacity, dtype=torch.int32, device=device)
        self.labels = torch.empty(self.capacity, dtype=torch.int32, device=device)
        self.counters = torch.zeros(4, dtype=torch.int64, device=device)

    def _reserve(self, rows: int) -> None:
        """room for `rows` more: double the buffers (device copies of the `count` slots in use, a size the host knows)"""
        need = self.count + rows
        if need <= self.capacity:
            return
        cap = self.capacity
        while cap < need:
            cap *= 2
        if cap >= 1 << 31:
            raise ValueError(f"auroc: {need} rows are beyond the 2^31 slots of one object")
        keys = torch.empty(self.ncol, cap, dtype=torch.int32, device=self.keys.device)
        labels = torch.empty(cap, dtype=torch.int32, device=self.keys.device)
        keys[:, :self.count].copy_(self.keys[:, :self.count])
        labels[:self.count].copy_(self.labels[:self.count])
        self.keys, self.labels, self.capacity = keys, labels, cap

    def update(self, pred: torch.Tensor, target: torch.Tensor) -> None:
        C = self.num_classes
        if not pred.is_cuda or not target.is_cuda:
            dev = pred.device if pred.is_cuda else target.device if target.is_cuda else torch.device("cuda", torch.cuda.current_device())
            pred, target = pred.to(dev), target.to(dev)
        ops._need_gpu(pred, target)
        if self.keys is None:
            self._alloc(pred.device)
        ops._need_gpu(self.keys)
        pred = pred.detach()
        if target.dtype.is_floating_point or target.dtype == torch.bool:
            raise TypeError("auroc: target must be an integer tensor")
        if not pred.dtype.is_floating_point:
            raise TypeError("auroc: pred must be floating-point scores (a ranking needs them; labels have none)")
        target = ops._c(target.reshape(-1).long())
        B = target.shape[0]
        if pred.dim() == 1 and C == 2:
            pred = pred.unsqueeze(1)
            col0 = 0
        else:
            if pred.dim() != 2 or pred.shape[1] != C:
                raise ValueError(f"auroc: scores must be [{B}, {C}]" + (f" or [{B}]" if C == 2 else "") + f", got {tuple(pred.shape)}")
            col0 = self.pos_label if C == 2 else 0
        if pred.shape[0] != B:
            raise ValueError(f"auroc: {pred.shape[0]} rows of scores for {B} targets")
        if pred.dtype not in (torch.float32, torch.bfloat16):
            pred = pred.float()                          # float16 (exact), float64
        width = pred.shape[1]
        if pred.stride(1) != 1 or (B > 1 and pred.stride(0) < width):
            pred = pred.contiguous()
        ld = pred.stride(0) if B > 1 else max(width, pred.stride(0))
        self._reserve(B)
        check(lib.meant_score_capture(ops._p(pred), ld, ops._dt(pred), ops._p(target), B, C, col0, self.ncol, self.ignore_index,
                                      ops._p(self.keys), ops._p(self.labels), self.capacity, self.count, ops._p(self.counters),
                                      ops._stream()), "score_capture")
        self.count += B

    def reset(self) -> None:
        self.count = 0
        if self.counters is not None:
            self.counters.zero_()

    def merge(self, other: "auroc") -> "auroc":
        """append another object's captured rows (same classes and positive label) to this one's, on this one's device: after a
        gather of the ranks' objects the statistic is that of all their rows"""
        if (other.num_classes, other.pos_label, other.ncol) != (self.num_classes, self.pos_label, self.ncol):
            raise ValueError("auroc.merge: different num_classes / pos_label")
        if other.keys is None:
            return self
        if self.keys is None:
            self._alloc(other.keys.device)
        self._reserve(other.count)
        a, b = self.count, self.count + other.count
        self.keys[:, a:b].copy_(other.keys[:, :other.count])
        self.labels[a:b].copy_(other.labels[:other.count])
        self.counters += other.counters.to(self.counters.device)
        self.count = b
        return self

    # ---- host side ------------------------------------------------------------------------------------
    def statistic(self) -> torch.Tensor:
        """int64 [ncol, 3] on the CPU: (2U, P, N) per captured column"""
        if self.keys is None or self.count == 0:
            return torch.zeros(self.ncol, 3, dtype=torch.int64)
        n = self.count
        with torch.cuda.device(self.keys.device):
            out = torch.empty(self.ncol, 3, dtype=torch.int64, device=self.keys.device)
            wsb = lib.meant_auroc_ws(n)
            ws = torch.empty(wsb, dtype=torch.uint8, device=self.keys.device)
            st = ops._stream()
            for c in range(self.ncol):
                positive = self.pos_label if self.num_classes == 2 else c
                check(lib.meant_auroc_rank(ops._p(self.keys[c]), ops._p(self.labels), n, positive, ops._p(out[c]), ops._p(ws), wsb, st),
                      "auroc_rank")
            return out.cpu()

    @staticmethod
    def from_statistic(stat: torch.Tensor) -> torch.Tensor:
        """float64 [ncol]: 2U / (2 P N), NaN where P or N is 0"""
        u2, P, N = (stat[:, i].double() for i in range(3))
        den = 2 * P * N
        return torch.where(den > 0, u2 / den.clamp(min=1), torch.full_like(den, math.nan))

    def per_class(self) -> torch.Tensor:
        return self.from_statistic(self.statistic())

    def compute(self) -> torch.Tensor:
        a = self.per_class()
        ok = ~torch.isnan(a)
        return (a[ok].mean() if ok.any() else torch.tensor(math.nan, dtype=torch.float64)).float()

    def _counter(self, k: int) -> int:
        return 0 if self.counters is None else int(self.counters[k].item())

    def invalid_rows(self) -> int:
        return self._counter(2)

    def nan_rows(self) -> int:
        """rows left out because one of their captured scores is a NaN"""
        return self._counter(3)

    def show(self):
        value = self.compute()
        print(self.set_name + ' AUROC: ', value)
        return value


class vqa_score:
    """The VQA score of soft labels, counted on the device: the answer weight of the predicted answer, averaged over the questions
    (the reference's loop hands `out.cpu()` and the float [B, C] target of utils/custom_datasets.py:214-218 to its metrics at
    vqa.py:223).

    update(pred, target): pred [B, C] float32 / bfloat16 scores (float16 and float64 through `.float()`), target [B, C] floating
    point of the same shape, float32 / bfloat16 read as they are and any other float type widened to float32; both may be column
    slices of wider blocks.  The prediction is `pred.argmax(dim=1)` as torch computes it (lowest index on a tie, a NaN above
    everything); the row scores `target[b, prediction]`.  A row whose weight there is not finite or outside [0, 16] is counted
    in `invalid_rows()` and left out; a row with a NaN among its scores is scored all the same and counted in `nan_rows()`.  Tensors
    on the CPU are copied to the current device.  One launch (meant_vqa_score_update), no host read.

    `state` (int64 [4] = sum of the weights in 2^-32 units, rows, nan rows, invalid rows) only ever has integers added: any
    batching gives the same bits, and the states of several devices may be summed.  `compute()` / `show()` make one copy of it.
    """

    def __init__(self, set_name: str = "", device=None):
        self.set_name = set_name
        self.state: Optional[torch.Tensor] = None        # allocated on the first update's device (or `device`)
        if device is not None:
            self._alloc(torch.device(device))

    def _alloc(self, device):
        self.state = torch.zeros(4, dtype=torch.int64, device=device)

    def update(self, pred: torch.Tensor, target: torch.Tensor) -> None:
        if not pred.dtype.is_floating_point or not target.dtype.is_floating_point:
            raise TypeError("vqa_score: pred and target must be floating-point [B, C] tensors (scores and answer weights)")
        if pred.dim() != 2 or target.shape != pred.shape:
            raise ValueError(f"vqa_score: scores and weights must both be [B, C], got {tuple(pred.shape)} and {tuple(target.shape)}")
        if not pred.is_cuda or not target.is_cuda:
            dev = pred.device if pred.is_cuda else target.device if target.is_cuda else torch.device("cuda", torch.cuda.current_device())
            pred, target = pred.to(dev), target.to(dev)
        ops._need_gpu(pred, target)
        if self.state is None:
            self._alloc(pred.device)
        ops._need_gpu(self.state)
        B, C = pred.shape
        if B == 0:
            return
        (pred, lds), (target, ldt) = (ops._rows(x if x.dtype in (torch.float32, torch.bfloat16) else x.float())     # float16 (exact), float64
                                      for x in (pred.detach(), target.detach()))
        check(lib.meant_vqa_score_update(ops._p(pred), lds, ops._dt(pred), ops._p(target), ldt, ops._dt(target), B, C, ops._p(self.state),
                                         ops._stream()), "vqa_score_update")

    def reset(self) -> None:
        if self.state is not None:
            self.state.zero_()

    def merge(self, other: "vqa_score") -> "vqa_score":
        """add another object's counts to this one's, on this one's device"""
        if other.state is None:
            return self
        if self.state is None:
            self._alloc(other.state.device)
        self.state += other.state.to(self.state.device)
        return self

    def _host_state(self) -> torch.Tensor:
        return torch.zeros(4, dtype=torch.int64) if self.state is None else self.state.cpu()

    @staticmethod
    def from_state(state: torch.Tensor) -> torch.Tensor:
        """the mean score, a 0-d float64 tensor: sum_fx / 2^32 / rows, 0 for no rows (pure torch on the CPU)"""
        if state.dtype != torch.int64 or state.numel() != 4:
            raise ValueError(f"vqa_score: the state is int64 [4], got {state.dtype} [{state.numel()}]")
        s = state.detach().reshape(-1).cpu()
        rows = s[1].double()
        return s[0].double() / 4294967296.0 / rows if rows.item() > 0 else torch.zeros((), dtype=torch.float64)

    def compute(self) -> torch.Tensor:
        return self.from_state(self._host_state())

    def nan_rows(self) -> int:
        """scored rows with a NaN among their scores"""
        return 0 if self.state is None else int(self.state[2].item())

    def invalid_rows(self) -> int:
        """rows left out because the weight at their prediction is not finite or outside [0, 16]"""
        return 0 if self.state is None else int(self.state[3].item())

    def show(self):
        value = self.compute()
        print(self.set_name + ' VQA score: ', value)
        return value


class metric_group:
    """Several metric objects behind one `update` / `reset` / `show`, so that one `TrainStep(metrics=...)` or `train.evaluate` feeds
    them all: metric_group(f1_metrics(2, "Train"), auroc(2, "Train"))"""

    def __init__(self, *metrics):
        self.metrics = tuple(metrics)

    def update(self, pred: torch.Tensor, target: torch.Tensor) -> None:
        for m in self.metrics:
            m.update(pred, target)

    def reset(self) -> None:
        for m in self.metrics:
            m.reset()

    def show(self, *args, **kwargs):
        return tuple(m.show(*args, **kwargs) if isinstance(m, f1_metrics) else m.show() for m in self.metrics)
