"""The yardsticks of test_gpu_ce_hard.py, checked on the host.  ce_hard_ref.reference against F.cross_entropy in float64 with the same
weight=, label_smoothing= and ignore_index= ('none', 'sum', 'mean' and the autograd gradient); this project's convention where the
denominator is 0; the gates recomputed from the float32 emulation; the wrappers' argument errors that need no device; and
balanced_class_weights against a numpy count.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ce_hard_ref as R

EPS = (0.0, 0.1, 1.0)
WKINDS = (None, "rand", "zeros")
SHAPES = [(1, 1), (6, 2), (7, 5), (9, 67), (5, 1030)]


def _inputs(T, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, C, generator=g) * 4
    y = torch.randint(0, C, (T,), generator=g)
    if T >= 5:
        y[1] = R.IGNORE
        y[T - 1] = R.IGNORE
    return x, y


@pytest.mark.parametrize("wkind", WKINDS, ids=["w_none", "w_rand", "w_zeros"])
@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("T,C", SHAPES, ids=[f"{t}x{c}" for t, c in SHAPES])
def test_reference_equals_torch_in_float64(T, C, eps, wkind):
    x, y = _inputs(T, C, T * 31 + C)
    w = R.make_weight(wkind, C, T)
    ref = R.reference(x, y, w, eps)
    kw = dict(weight=None if w is None else w.double(), label_smoothing=eps, ignore_index=R.IGNORE)
    xd = x.double().requires_grad_(True)
    rows = F.cross_entropy(xd, y, reduction="none", **kw)
    assert torch.allclose(ref["row_loss"], rows.detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(ref["num"], F.cross_entropy(xd, y, reduction="sum", **kw).detach(), rtol=1e-12, atol=1e-12)
    g_rows, = torch.autograd.grad(rows.sum(), xd)
    assert torch.allclose(ref["grad_rows"], g_rows, rtol=1e-12, atol=1e-13)
    assert ref["n_counted"] + ref["n_ignored"] + ref["n_invalid"] == T and ref["n_invalid"] == 0
    if float(ref["den"]) != 0:
        mean = F.cross_entropy(xd, y, **kw)
        assert torch.allclose(ref["loss"], mean.detach(), rtol=1e-12, atol=1e-12)
        g, = torch.autograd.grad(mean, xd)
        assert torch.allclose(ref["grad"], g, rtol=1e-12, atol=1e-13)
    else:                                                # torch: 0 / 0; here: 0 and a zero gradient
        assert float(ref["loss"]) == 0.0 and float(ref["grad"].abs().max()) == 0.0


def test_zero_denominator_convention():
    x, y = _inputs(6, 5, 3)
    for yy, w in ((torch.full_like(y, R.IGNORE), None), (torch.full_like(y, 2), torch.tensor([1.0, 1.0, 0.0, 2.0, 1.0])),
                  (torch.tensor([5, -1, 2 ** 31 + 3, R.IGNORE, 7, -5]), None)):
        for eps in (0.0, 0.1):
            ref, emu = R.reference(x, yy, w, eps), R.emulate(x, yy, w, eps)
            assert float(ref["den"]) == 0 and float(ref["loss"]) == 0 and float(ref["grad"].abs().max()) == 0
            assert float(emu["loss"]) == 0
    ref = R.reference(x, torch.tensor([5, -1, 2 ** 31 + 3, R.IGNORE, 7, -5]))
    assert (ref["n_counted"], ref["n_ignored"], ref["n_invalid"]) == (0, 1, 5)
    garbage = torch.full((6, 5), float("nan"))
    ref = R.reference(garbage, torch.full_like(y, R.IGNORE))
    assert float(ref["row_loss"].abs().max()) == 0 and float(ref["grad_rows"].abs().max()) == 0


def test_masked_column_at_eps_zero():
    x, y = _inputs(4, 9, 1)
    x[:, 3] = R.NEG_INF
    y[:] = torch.tensor([0, 1, 2, 4])
    w = R.make_weight("rand", 9, 1)
    ref = R.reference(x, y, w, 0.0)
    assert bool(torch.isfinite(ref["row_loss"]).all()) and float(ref["grad_rows"][:, 3].abs().max()) == 0
    xd = x.double().requires_grad_(True)
    assert torch.allclose(ref["loss"], F.cross_entropy(xd, y, weight=w.double()).detach(), rtol=1e-12, atol=0)
    for form in ("reg", "stream", "vocab"):
        assert R.errors(R.emulate(x, y, w, 0.0, form=form), ref)["row_loss"] <= R.GATES["f32"]["row_loss"]


@pytest.mark.parametrize("C", [1, 5, 8, 12, 1023, 1024, 1025, 2049, 4101, 5000])
def test_the_emulations_walk_every_column_once(C):
    for form in ("stream", "vocab"):
        cols = torch.cat([s.reshape(-1) for s in R._steps(C, form)])
        assert sorted(cols[cols >= 0].tolist()) == list(range(C)), form


@pytest.mark.parametrize("tier", ["probs", "f32", "bf16"])
def test_gates_are_four_times_the_emulation(tier):
    worst = R.emulation_worst(tier)
    print(tier, {k: f"{v:.3e}" for k, v in worst.items()})
    assert set(worst) == set(R.GATES[tier])
    for name, gate in R.GATES[tier].items():
        if gate == 0.0:
            assert worst[name] == 0.0, (name, worst[name])
        else:
            assert 3.2 * worst[name] <= gate <= 8.0 * worst[name], (name, worst[name], gate)


def test_wrapper_argument_errors():
    from meant_amd import ops
    from meant_amd.train import TrainStep, cross_entropy_on_probs
    p, y = torch.rand(4, 3), torch.tensor([0, 1, 2, 0])
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="label_smoothing"):
            cross_entropy_on_probs(p, y, label_smoothing=bad)
        with pytest.raises(ValueError, match="label_smoothing"):
            ops.softmax_cross_entropy(p, y, label_smoothing=bad)
        with pytest.raises(ValueError, match="label_smoothing"):
            TrainStep(torch.nn.Linear(2, 2), label_smoothing=bad)
    for w in (torch.ones(4), torch.ones(3, 1), torch.ones(2)):
        with pytest.raises(ValueError, match="weight"):
            cross_entropy_on_probs(p, y, weight=w)
        with pytest.raises(ValueError, match="weight"):
            ops.softmax_cross_entropy(p, y, weight=w)
    soft = torch.rand(4, 3)
    for kw in (dict(weight=torch.ones(3)), dict(label_smoothing=0.1), dict(ignore_index=-100)):
        with pytest.raises(ValueError, match="class-index"):
            cross_entropy_on_probs(p, soft, **kw)
    with pytest.raises(ValueError, match="target"):
        cross_entropy_on_probs(p, y[:3], label_smoothing=0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # the options do not open a fallback: a missing device is an error
        cross_entropy_on_probs(p, y, label_smoothing=0.1)
    w, eps = ops.ce_options([1, 2, 3], 0.25, 3)
    assert w.dtype == torch.float32 and w.tolist() == [1.0, 2.0, 3.0] and eps == 0.25 and w.data_ptr() % 16 == 0
    assert ops.ce_options(None, 0, 3) == (None, 0.0)


@pytest.mark.parametrize("C", [2, 7, 3129])
def test_balanced_class_weights_against_numpy(C):
    from meant_amd import balanced_class_weights
    rs = np.random.RandomState(C)
    lab = rs.randint(0, C, size=500).astype(np.int64)
    lab[lab == 1] = 0                                    # class 1 is empty
    lab[::17] = -100                                     # an ignore value is left out of the counts and of n
    inside = lab[(lab >= 0) & (lab < C)]
    cnt = np.bincount(inside, minlength=C).astype(np.float64)
    want = np.where(cnt > 0, len(inside) / (C * np.maximum(cnt, 1)), 0.0).astype(np.float32)
    got = balanced_class_weights(torch.from_numpy(lab).view(20, 25), C)
    assert got.dtype == torch.float32 and got.shape == (C,) and got[1].item() == 0.0
    assert np.array_equal(got.numpy(), want)
    # the ntarget slice of an f1_metrics state (int64 [3C + 4]: tp, npred, ntarget, ...) gives the same weights
    state = torch.zeros(3 * C + 4, dtype=torch.int64)
    state[2 * C:3 * C] = torch.from_numpy(cnt).long()
    assert torch.equal(balanced_class_weights(state[2 * C:3 * C], C, counts=True), got)
    with pytest.raises(ValueError):
        balanced_class_weights(torch.rand(5), C)
    with pytest.raises(ValueError):
        balanced_class_weights(torch.ones(C + 1, dtype=torch.int64), C, counts=True)
