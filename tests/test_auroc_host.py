"""Host-side facts of MCC and AUROC (no GPU): the three entry points and meant_auroc_ws are in the header, the ctypes table and the
built library and their route names exist; every bad argument comes back with its status before anything is launched (the pointers
below are made-up addresses that are never dereferenced); the workspace size is host arithmetic; f1_metrics.mcc_from_counts -- pure
torch on the CPU -- against scikit-learn; the host halves of auroc and metric_group."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, -1, -2, -4
SPAN = 1 << 40                                         # distance between the made-up buffers
SCORES, TARGET, KEYS, LABELS, COUNTERS, OUT, WS = (SPAN * (i + 1) for i in range(7))
F32, BF16 = 0, 1
ROUTES = ("score_capture", "auroc_rank")


def test_symbols_in_header_table_and_library():
    from meant_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "meant_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("meant_score_capture", "meant_auroc_ws", "meant_auroc_rank"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES
        assert re.search(r" T %s$" % name, out, flags=re.M), name
    _lib.route_reset()
    for route in ROUTES:
        assert _lib.route_count(route) == 0


def test_python_names_are_exported():
    import meant_amd
    assert meant_amd.auroc is meant_amd.metrics.auroc and meant_amd.metric_group is meant_amd.metrics.metric_group
    assert callable(meant_amd.f1_metrics.mcc_from_counts) and callable(meant_amd.f1_metrics.mcc)


def _capture(lib, scores=SCORES, ld=8, dtype=F32, target=TARGET, B=4, C=2, col0=0, ncol=2, keys=KEYS, labels=LABELS, capacity=64, offset=0,
             counters=COUNTERS):
    return lib.meant_score_capture(scores, ld, dtype, target, B, C, col0, ncol, -100, keys, labels, capacity, offset, counters, None)


def _rank(lib, keys=KEYS, labels=LABELS, n=100, positive=1, out=OUT, ws=WS, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.meant_auroc_ws(n)
    return lib.meant_auroc_rank(keys, labels, n, positive, out, ws, ws_bytes, None)


@pytest.mark.parametrize("kw", [dict(scores=None), dict(target=None), dict(keys=None), dict(labels=None), dict(counters=None), dict(B=-1),
                                dict(C=0), dict(C=-2), dict(ncol=0), dict(ncol=-1), dict(col0=-1), dict(col0=7, ncol=2), dict(ld=1, ncol=2),
                                dict(col0=1, ncol=8), dict(offset=-1), dict(offset=61, B=4, capacity=64), dict(offset=0, B=65, capacity=64),
                                dict(offset=1 << 62, B=1 << 62), dict(capacity=-1, B=0), dict(dtype=7), dict(dtype=-1), dict(scores=SCORES + 2),
                                dict(dtype=BF16, scores=SCORES + 1), dict(target=TARGET + 4), dict(keys=KEYS + 2), dict(labels=LABELS + 1),
                                dict(counters=COUNTERS + 4)])
def test_capture_rejects_bad_arguments_before_any_launch(kw):
    from meant_amd import _lib
    _lib.route_reset()
    assert _capture(_lib.lib, **kw) == ERR_ARG, kw
    assert b"score_capture" in _lib.lib.meant_last_error()
    assert all(_lib.route_count(r) == 0 for r in ROUTES)


def test_capture_capacity_limit_and_empty_batch():
    from meant_amd import _lib
    _lib.route_reset()
    assert _capture(_lib.lib, capacity=1 << 31) == ERR_UNSUPPORTED
    assert b"2^31" in _lib.lib.meant_last_error()
    assert _capture(_lib.lib, capacity=1 << 40, offset=1 << 35) == ERR_UNSUPPORTED
    assert _capture(_lib.lib, capacity=(1 << 31) - 1, offset=(1 << 31) - 5, B=0) == OK
    assert _capture(_lib.lib, B=0) == OK                                     # nothing to capture: no launch
    assert _capture(_lib.lib, B=0, offset=64, capacity=64) == OK             # a full buffer takes an empty batch
    assert _capture(_lib.lib, B=0, C=0) == ERR_ARG                           # the argument checks come first
    assert _capture(_lib.lib, B=0, capacity=1 << 31, ncol=0) == ERR_ARG
    assert all(_lib.route_count(r) == 0 for r in ROUTES)


@pytest.mark.parametrize("kw,status", [(dict(out=None), ERR_ARG), (dict(keys=None), ERR_ARG), (dict(labels=None), ERR_ARG), (dict(n=-1), ERR_ARG),
                                       (dict(keys=KEYS + 2), ERR_ARG), (dict(labels=LABELS + 1), ERR_ARG), (dict(out=OUT + 4), ERR_ARG),
                                       (dict(ws=WS + 4), ERR_ARG), (dict(n=0, out=None), ERR_ARG),
                                       (dict(n=1 << 31), ERR_UNSUPPORTED), (dict(n=1 << 40, ws_bytes=1 << 50), ERR_UNSUPPORTED),
                                       (dict(ws=None), ERR_WORKSPACE), (dict(ws_bytes=0), ERR_WORKSPACE), (dict(n=1, ws_bytes=0), ERR_WORKSPACE),
                                       (dict(n=600001, ws_bytes="short"), ERR_WORKSPACE), (dict(n=(1 << 31) - 1, ws_bytes="short"), ERR_WORKSPACE)])
def test_rank_rejects_bad_arguments_before_any_launch(kw, status):
    from meant_amd import _lib
    _lib.route_reset()
    if kw.get("ws_bytes") == "short":
        kw = dict(kw, ws_bytes=_lib.lib.meant_auroc_ws(kw["n"]) - 1)
    assert _rank(_lib.lib, **kw) == status, kw
    assert b"auroc_rank" in _lib.lib.meant_last_error()
    assert all(_lib.route_count(r) == 0 for r in ROUTES)


def test_workspace_size_is_host_arithmetic():
    from meant_amd import _lib
    ws = _lib.lib.meant_auroc_ws
    assert ws(0) == 0 and ws(-5) == 0 and ws(1 << 31) == 0 and ws(1 << 40) == 0
    sizes = [ws(n) for n in (1, 2, 2048, 2049, 65536, 600001, 10 ** 6, (1 << 31) - 1)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    for n, s in zip((1, 2048, 10 ** 6), (sizes[0], sizes[2], sizes[6])):
        assert s >= 3 * 4 * n                                                # the class codes and the sorted (key, code) pairs at least
        assert s <= 64 * n + (1 << 16)                                       # ... and a small multiple of the input


# ---- MCC ------------------------------------------------------------------------------------------------------------------------
def _state(pred, target, C, extra=(0, 0, 0)):
    pred, target = np.asarray(pred), np.asarray(target)
    tp = np.bincount(pred[pred == target], minlength=C)
    s = np.concatenate([tp, np.bincount(pred, minlength=C), np.bincount(target, minlength=C), [len(target), *extra]])
    return torch.from_numpy(s.astype(np.int64))


@pytest.mark.parametrize("C", [2, 3, 7])
def test_mcc_matches_scikit_learn(C):
    from sklearn.metrics import matthews_corrcoef
    from meant_amd import f1_metrics
    rs = np.random.RandomState(10 + C)
    n = 60 * C
    target = np.concatenate([np.arange(C), rs.randint(0, C, n - C)])
    pred = np.where(rs.rand(n) < 0.6, target, rs.randint(0, C, n))
    got = f1_metrics.mcc_from_counts(_state(pred, target, C, extra=(4, 3, 2)), C)      # the other tail counters do not enter
    assert got.dtype == torch.float64 and got.dim() == 0
    assert abs(got.item() - matthews_corrcoef(target, pred)) <= 1e-12
    assert 0.2 < got.item() < 1.0
    absent = np.where(pred == C - 1, 0, pred)                                # a class absent from the predictions
    got = f1_metrics.mcc_from_counts(_state(absent, target, C), C).item()
    assert abs(got - matthews_corrcoef(target, absent)) <= 1e-12
    inverted = (target + 1) % C                                              # never right
    got = f1_metrics.mcc_from_counts(_state(inverted, target, C), C).item()
    assert abs(got - matthews_corrcoef(target, inverted)) <= 1e-12 and got < 0
    assert abs(f1_metrics.mcc_from_counts(_state(target, target, C), C).item() - 1.0) <= 1e-12


def test_mcc_binary_form_and_degenerate_states():
    from sklearn.metrics import matthews_corrcoef
    from meant_amd import f1_metrics
    target = np.array([1, 1, 1, 0, 0, 0, 0, 1, 0, 1])
    pred = np.array([1, 0, 1, 0, 0, 1, 0, 1, 0, 0])
    tp, tn, fp, fn = 3, 4, 1, 2
    binary = (tp * tn - fp * fn) / math.sqrt((tp + fp) * (tp + fn) * (tn + fp) * (tn + fn))
    got = f1_metrics.mcc_from_counts(_state(pred, target, 2), 2).item()
    assert abs(got - binary) <= 1e-15 and abs(got - matthews_corrcoef(target, pred)) <= 1e-12
    for C in (2, 3, 7):
        one = np.full(40, C - 1)                                             # everything predicted as one class
        t = np.arange(40) % C
        v = f1_metrics.mcc_from_counts(_state(one, t, C), C)
        assert v.item() == 0.0 and matthews_corrcoef(t, one) == 0.0
        assert f1_metrics.mcc_from_counts(_state(t, one, C), C).item() == 0.0        # one class the only target
        empty = f1_metrics.mcc_from_counts(torch.zeros(3 * C + 4, dtype=torch.int64), C)
        assert empty.item() == 0.0 and empty.dtype == torch.float64              # 0, not NaN
    m = f1_metrics(3, "Empty")                                               # never updated: no device touched
    assert m.mcc().item() == 0.0 and m.mcc().dtype == torch.float32 and m.mcc().dim() == 0
    with pytest.raises(ValueError):
        f1_metrics.mcc_from_counts(torch.zeros(9, dtype=torch.int64), 2)


# ---- the host halves of auroc and metric_group -----------------------------------------------------------------------------------
def test_auroc_before_any_update_and_from_statistic(capsys):
    from meant_amd import auroc
    for C, ncol in ((2, 1), (5, 5)):
        m = auroc(C, "Val")
        assert m.ncol == ncol and m.count == 0
        assert torch.equal(m.statistic(), torch.zeros(ncol, 3, dtype=torch.int64))
        v = m.compute()
        assert v.dtype == torch.float32 and v.dim() == 0 and math.isnan(v.item())
        assert m.per_class().dtype == torch.float64 and torch.isnan(m.per_class()).all()
        assert m.nan_rows() == 0 and m.invalid_rows() == 0
        m.reset()
    stat = torch.tensor([[12, 2, 4], [0, 0, 9], [5, 5, 0], [50, 5, 5]])
    a = auroc.from_statistic(stat)
    assert a[0].item() == 0.75 and math.isnan(a[1].item()) and math.isnan(a[2].item()) and a[3].item() == 1.0
    for bad in (dict(num_classes=1), dict(num_classes=2, pos_label=2), dict(capacity=0)):
        with pytest.raises(ValueError):
            auroc(**bad)
    auroc(2, "Val").show()
    assert "Val AUROC" in capsys.readouterr().out


def test_metric_group_fans_out():
    from meant_amd import metric_group

    class Probe:
        def __init__(self):
            self.calls = []

        def update(self, pred, target):
            self.calls.append(("update", pred, target))

        def reset(self):
            self.calls.append(("reset",))

        def show(self):
            self.calls.append(("show",))
            return len(self.calls)

    a, b = Probe(), Probe()
    g = metric_group(a, b)
    g.update("p", "t"); g.reset()
    assert g.show() == (3, 3)
    assert a.calls == b.calls == [("update", "p", "t"), ("reset",), ("show",)]
    assert g.metrics == (a, b)
