"""Host-side facts of the classification counts (no GPU): the two entry points are in the header, the ctypes table and the built
library and their route names exist; the drop-in `utils` package exports f1_metrics; bad arguments come back with their status
before anything is launched (the pointers below are made-up addresses that are never dereferenced); the finalisation
f1_metrics.from_counts -- pure torch on the CPU -- against scikit-learn and against hand-derived values."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2
SPAN = 1 << 40                                         # distance between the made-up buffers
SCORES, TARGET, STATE, CONF, PRED = (SPAN * (i + 1) for i in range(5))
F32, BF16 = 0, 1


def test_symbols_in_header_table_and_library():
    from meant_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "meant_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("meant_metrics_update", "meant_metrics_update_labels"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES
        assert re.search(r" T %s$" % name, out, flags=re.M), name
    _lib.route_reset()
    for route in ("metrics_rows", "metrics_wave", "metrics_labels"):
        assert _lib.route_count(route) == 0


def test_dropin_utils_exports_f1_metrics():
    """in_loop_train.py:30 / test_run.py:27: `from utils import f1_metrics` with <repo>/dropin ahead on the path"""
    import meant_amd
    stale = lambda: [m for m in list(sys.modules) if m == "utils" or m.startswith("utils.")]
    path = os.path.join(ROOT, "dropin")
    for mod in stale():
        del sys.modules[mod]
    sys.path.insert(0, path)
    try:
        from utils import f1_metrics, RMSNorm  # noqa: F401
        assert f1_metrics is meant_amd.f1_metrics and f1_metrics is meant_amd.metrics.f1_metrics
    finally:
        sys.path.remove(path)
        for mod in stale():
            del sys.modules[mod]


def _update(lib, scores=SCORES, ld=8, dtype=F32, target=TARGET, B=4, C=8, state=STATE, conf=None):
    return lib.meant_metrics_update(scores, ld, dtype, target, B, C, -100, state, conf, None)


def _labels(lib, pred=PRED, target=TARGET, B=4, C=8, state=STATE, conf=None):
    return lib.meant_metrics_update_labels(pred, target, B, C, -100, state, conf, None)


@pytest.mark.parametrize("kw", [dict(ld=7, C=8), dict(ld=2999, C=3000), dict(C=0, ld=0), dict(C=-3), dict(state=None), dict(scores=None),
                                dict(target=None), dict(B=-1), dict(dtype=7), dict(scores=SCORES + 2), dict(dtype=BF16, scores=SCORES + 1),
                                dict(target=TARGET + 4), dict(state=STATE + 4), dict(conf=CONF + 2)])
def test_update_rejects_bad_arguments_before_any_launch(kw):
    from meant_amd import _lib
    _lib.route_reset()
    assert _update(_lib.lib, **kw) == ERR_ARG, kw
    assert b"metrics_update" in _lib.lib.meant_last_error()
    assert _lib.route_count("metrics_rows") == 0 and _lib.route_count("metrics_wave") == 0


@pytest.mark.parametrize("kw", [dict(C=0), dict(state=None), dict(pred=None), dict(target=None), dict(B=-1), dict(pred=PRED + 4)])
def test_update_labels_rejects_bad_arguments_before_any_launch(kw):
    from meant_amd import _lib
    _lib.route_reset()
    assert _labels(_lib.lib, **kw) == ERR_ARG, kw
    assert b"metrics_update_labels" in _lib.lib.meant_last_error()
    assert _lib.route_count("metrics_labels") == 0


def test_row_limit_and_empty_batch():
    from meant_amd import _lib
    _lib.route_reset()
    for C, ld in ((2, 2), (3000, 3000)):
        assert _update(_lib.lib, B=1 << 40, C=C, ld=ld) == ERR_UNSUPPORTED
        assert b"2^40" in _lib.lib.meant_last_error()
        assert _update(_lib.lib, B=0, C=C, ld=ld) == OK              # nothing to count: no launch
    assert _labels(_lib.lib, B=1 << 40) == ERR_UNSUPPORTED
    assert _labels(_lib.lib, B=0) == OK
    assert _update(_lib.lib, B=0, C=0, ld=0) == ERR_ARG              # the argument checks come first
    assert all(_lib.route_count(r) == 0 for r in ("metrics_rows", "metrics_wave", "metrics_labels"))


# ---- finalisation ---------------------------------------------------------------------------------------------------------
def _state(pred, target, C, extra=(0, 0, 0)):
    pred, target = np.asarray(pred), np.asarray(target)
    tp = np.bincount(pred[pred == target], minlength=C)
    s = np.concatenate([tp, np.bincount(pred, minlength=C), np.bincount(target, minlength=C), [len(target), *extra]])
    return torch.from_numpy(s.astype(np.int64))


@pytest.mark.parametrize("C", [2, 3, 7, 100])
def test_from_counts_matches_scikit_learn(C):
    from sklearn.metrics import accuracy_score, precision_recall_fscore_support
    from meant_amd import f1_metrics
    rs = np.random.RandomState(C)
    n = 50 * C
    target = np.concatenate([np.arange(C), rs.randint(0, C, n - C)])          # every class occurs
    pred = np.where(rs.rand(n) < 0.6, target, rs.randint(0, C, n))
    state = _state(pred, target, C, extra=(5, 2, 1))                         # the other tail counters do not enter
    labels = list(range(C))
    want = {avg: precision_recall_fscore_support(target, pred, labels=labels, average=avg, zero_division=0)[:3] for avg in ("macro", "micro")}
    for absent in ("skip", "zero"):
        got = f1_metrics.from_counts(state, C, absent)
        assert all(v.dtype == torch.float64 and v.dim() == 0 for v in got)
        ref = (accuracy_score(target, pred), want["macro"][2], want["micro"][2], want["macro"][0], want["micro"][0], want["macro"][1],
               want["micro"][1])
        for g, w in zip(got, ref):
            assert abs(g.item() - float(w)) <= 1e-12, (absent, got, ref)
    p, r, f, sup = precision_recall_fscore_support(target, pred, labels=labels, average=None, zero_division=0)
    gp, gr, gf, gsup = f1_metrics.per_class_from_counts(state, C)
    for g, w in ((gp, p), (gr, r), (gf, f)):
        assert np.abs(g.numpy() - w).max() <= 1e-12
    assert np.array_equal(gsup.numpy(), sup)


def test_absent_class_skip_against_zero():
    """C = 3, class 2 neither predicted nor a target.  target 0 0 0 1 1, pred 0 0 1 1 0:
    class 0: tp 2, npred 3, ntarget 3 -> p = r = f1 = 2/3;  class 1: tp 1, npred 2, ntarget 2 -> p = r = f1 = 1/2;  class 2: 0 / 0 -> 0.
    micro = 3/5.  macro over the two present classes = 7/12 ("skip"), over all three = 7/18 ("zero")."""
    from meant_amd import f1_metrics
    state = _state([0, 0, 1, 1, 0], [0, 0, 0, 1, 1], 3)
    assert state.tolist() == [2, 1, 0, 3, 2, 0, 3, 2, 0, 5, 0, 0, 0]
    skip = [v.item() for v in f1_metrics.from_counts(state, 3, "skip")]
    zero = [v.item() for v in f1_metrics.from_counts(state, 3, "zero")]
    for got, macro in ((skip, 7 / 12), (zero, 7 / 18)):
        want = [0.6, macro, 0.6, macro, 0.6, macro, 0.6]
        assert max(abs(g - w) for g, w in zip(got, want)) <= 1e-15, (got, want)
    assert [v.item() for v in f1_metrics.from_counts(state, 3)] == skip          # the default
    p, r, f, sup = f1_metrics.per_class_from_counts(state, 3)
    assert p[2] == 0 and r[2] == 0 and f[2] == 0 and sup.tolist() == [3, 2, 0]
    with pytest.raises(ValueError):
        f1_metrics.from_counts(state, 3, "ignore")
    with pytest.raises(ValueError):
        f1_metrics.from_counts(state[:-1], 3)


@pytest.mark.parametrize("absent", ["skip", "zero"])
def test_empty_state_gives_zeros_not_nan(absent):
    from meant_amd import f1_metrics
    for C in (1, 2, 9):
        state = torch.zeros(3 * C + 4, dtype=torch.int64)
        assert [v.item() for v in f1_metrics.from_counts(state, C, absent)] == [0.0] * 7
        assert all(torch.equal(v.double(), torch.zeros(C, dtype=torch.float64)) for v in f1_metrics.per_class_from_counts(state, C))
    m = f1_metrics(4, "Empty", absent_classes=absent)                         # never updated: no device touched
    assert [v.item() for v in m.compute()] == [0.0] * 7 and all(v.dtype == torch.float32 and v.dim() == 0 for v in m.compute())
    assert m.nan_rows() == 0 and m.invalid_rows() == 0

