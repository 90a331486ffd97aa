"""Soft-target cross-entropy on the device (meant_ce_probs_soft, meant_amd.train.cross_entropy_on_probs with a float [B, C] target)
against torch.nn.functional.cross_entropy(probs.double(), target.double()) on the CPU -- the reference loop's own call
(vqa.py:173,209) in fp64 -- with the row losses from reduction='none' and the gradient from autograd.

Gates (from an fp32 evaluation of the same shift-invariant form on the CPU, which stayed within 1.4e-7 * max(1, |ref|) on the loss
and 1.6e-7 absolute on the gradient over probabilities, randn * 8 and probabilities + 1000): the loss and every row loss within
1e-6 * max(1, |ref|), the gradient within 1e-6 absolute."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CUT = 1024                                             # C <= CUT: a wave per row ("ce_soft_wave"); above: a workgroup per row
SHAPES = [(1, 1), (3, 5), (5, 63), (4, 64), (4, 65), (7, 255), (7, 257), (4, CUT), (4, CUT + 1), (130, 3129), (3, 4096), (2, 4097), (9, 64001)]
KINDS = ("probs", "randn8", "shifted")
WEIGHTS = np.array([0.3, 0.6, 0.9, 1.0], dtype=np.float32)     # utils/custom_datasets.py:214-218


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def make_target(B, C, seed):
    """per row 0-4 distinct answer columns (at most C) with weights from WEIGHTS; with more than one row, row 0 is all zero and row 1
    holds the most answers a row can, which sum above 1"""
    rs = np.random.RandomState(seed)
    t = np.zeros((B, C), dtype=np.float32)
    for b in range(B):
        k = rs.randint(0, 5)
        if B > 1 and b < 2:
            k = 4 * b
        k = min(k, C)
        t[b, rs.choice(C, size=k, replace=False)] = WEIGHTS[rs.randint(0, 4, size=k)]
    if B > 1:
        sums = t.sum(1)
        assert (sums == 0).any() and (sums > 1).any()
    return torch.from_numpy(t)


def make_probs(B, C, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "randn8":
        return torch.randn(B, C, generator=g) * 8
    p = torch.rand(B, C, generator=g)
    return p + 1000 if kind == "shifted" else p


@functools.lru_cache(maxsize=None)
def case(B, C, kind, target_dtype=torch.float32):
    """inputs and the fp64 reference of one case, computed once and shared (never written to)"""
    p = make_probs(B, C, kind, seed=B * 131 + C)
    t = make_target(B, C, seed=B * 7 + C).to(target_dtype)
    pd = p.double().requires_grad_(True)
    td = t.double()                                    # what the kernel reads, widened exactly
    rows = F.cross_entropy(pd, td, reduction="none").detach()
    loss = F.cross_entropy(pd, td)
    loss.backward()
    return p, t, rows, loss.detach(), pd.grad


def run_entry(p, t, dev, with_grad=True):
    """one call of the C entry on contiguous device copies: (loss [1], row_loss [B], dprobs [B, C]), and the route counters it moved"""
    from meant_amd import _lib, ops
    B, C = p.shape
    p, t = p.to(dev).contiguous(), t.to(dev).contiguous()
    rows = torch.full((B,), float("nan"), device=dev)
    loss = torch.full((1,), float("nan"), device=dev)                    # overwritten, not added to
    dp = torch.full((B, C), float("nan"), device=dev) if with_grad else None
    _lib.route_reset()
    _lib.check(_lib.lib.meant_ce_probs_soft(p.data_ptr(), C, t.data_ptr(), C, ops._dt(t), rows.data_ptr(), loss.data_ptr(), ops._p(dp), C, B, C,
                                            ops._stream()), "ce_probs_soft")
    return loss, rows, dp, (_lib.route_count("ce_soft_wave"), _lib.route_count("ce_soft_block"))


def close(got, ref):
    """|got - ref| <= 1e-6 * max(1, |ref|), elementwise"""
    got, ref = got.detach().double().cpu().reshape(-1), ref.double().reshape(-1)
    err = (got - ref).abs()
    bound = 1e-6 * ref.abs().clamp(min=1.0)
    worst = (err / bound).max().item()
    return bool((err <= bound).all()), worst


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,C", SHAPES, ids=[f"{b}x{c}" for b, c in SHAPES])
def test_parity_with_fp64(dev, B, C, kind):
    from meant_amd.train import cross_entropy_on_probs
    p, t, ref_rows, ref_loss, ref_grad = case(B, C, kind)
    loss, rows, dp, routes = run_entry(p, t, dev)
    assert routes == ((1, 0) if C <= CUT else (0, 1)), routes           # the form this shape is meant to test
    ok_l, w_l = close(loss, ref_loss)
    ok_r, w_r = close(rows, ref_rows)
    gerr = (dp.double().cpu() - ref_grad).abs().max().item()
    print(f"[{B}, {C}] {kind}: loss {loss.item():.9g} ref {ref_loss.item():.9g} ({w_l:.3f} of the gate), rows {w_r:.3f} of the gate, grad err {gerr:.3e}")
    assert ok_l, (loss.item(), ref_loss.item())
    assert ok_r, w_r
    assert gerr <= 1e-6, gerr
    # the public route: the same bits, forward and backward
    pg = p.to(dev).requires_grad_(True)
    got = cross_entropy_on_probs(pg, t.to(dev))
    (got * 3.0).backward()
    assert got.dim() == 0 and torch.equal(got.detach(), loss[0])
    assert torch.equal(pg.grad, dp * 3.0)
    loss2, rows2, none, _ = run_entry(p, t, dev, with_grad=False)          # dprobs is optional
    assert none is None and torch.equal(loss2, loss) and torch.equal(rows2, rows)


@pytest.mark.parametrize("target_dtype", [torch.bfloat16, torch.float64, torch.float16], ids=["bf16", "f64", "f16"])
@pytest.mark.parametrize("B,C,ldp,ldt,poison", [(5, 63, 64, 72, float("nan")), (130, 3129, 3136, 3131, 1e30), (3, 4099, 4104, 4100, float("nan")),
                                                 (1, 257, 300, 258, float("nan"))])
def test_strides_and_target_types(dev, B, C, ldp, ldt, poison, target_dtype):
    """probs and target as column slices of wider blocks with a spare row after the last, everything outside the slices poisoned:
    not a bit of the loss or the gradient differs from the contiguous call, which itself meets the fp64 gates"""
    from meant_amd import _lib
    from meant_amd.train import cross_entropy_on_probs
    p, t, _, ref_loss, ref_grad = case(B, C, "randn8", target_dtype if target_dtype == torch.bfloat16 else torch.float32)
    t = t.to(target_dtype)
    if target_dtype == torch.float16:                                  # widened on the device: the reference sees the rounded weights
        ref = p.double().requires_grad_(True)
        ref_loss = F.cross_entropy(ref, t.double())
        ref_loss.backward()
        ref_loss, ref_grad = ref_loss.detach(), ref.grad
    pc = p.to(dev).requires_grad_(True)
    want = cross_entropy_on_probs(pc, t.to(dev))
    want.backward()
    assert close(want, ref_loss)[0] and (pc.grad.double().cpu() - ref_grad).abs().max().item() <= 1e-6
    pblock = torch.full((B + 1, ldp), poison, device=dev)
    tblock = torch.full((B + 1, ldt), poison, device=dev).to(target_dtype)      # 1e30 is inf in float16
    pblock[:B, :C] = p.to(dev)
    tblock[:B, :C] = t.to(dev)
    pblock.requires_grad_(True)
    _lib.route_reset()
    got = cross_entropy_on_probs(pblock[:B, :C], tblock[:B, :C])
    got.backward()
    assert _lib.route_count("ce_soft_wave") + _lib.route_count("ce_soft_block") == 1
    assert torch.equal(got.detach(), want.detach())
    assert torch.equal(pblock.grad[:B, :C], pc.grad)
    assert pblock.grad[B].abs().sum().item() == 0 and pblock.grad[:, C:].abs().sum().item() == 0


def test_repeated_calls_and_row_permutation(dev):
    """five calls give the same bits with the `deterministic` option off and on; permuting the rows permutes the row losses and the
    gradient rows exactly (a row's result does not depend on where it runs)"""
    from meant_amd import _lib
    B, C = 130, 3129
    p, t, _, _, _ = case(B, C, "probs")
    saved = _lib.get_option("deterministic")
    try:
        runs = []
        for i in range(5):
            _lib.set_option("deterministic", i % 2)
            loss, rows, dp, _ = run_entry(p, t, dev)
            runs.append((loss.clone(), rows.clone(), dp.clone()))
    finally:
        _lib.set_option("deterministic", saved)
    for loss, rows, dp in runs[1:]:
        assert torch.equal(loss, runs[0][0]) and torch.equal(rows, runs[0][1]) and torch.equal(dp, runs[0][2])
    perm = torch.from_numpy(np.random.RandomState(5).permutation(B))
    _, rows_p, dp_p, _ = run_entry(p[perm], t[perm], dev)
    assert torch.equal(rows_p.cpu(), runs[0][1].cpu()[perm])
    assert torch.equal(dp_p.cpu(), runs[0][2].cpu()[perm])
    for Bw, Cw in ((7, 257), (9, 64001)):                              # the wave form and the two-read form as well
        p, t, _, _, _ = case(Bw, Cw, "randn8")
        _, rows, dp, _ = run_entry(p, t, dev)
        perm = torch.from_numpy(np.random.RandomState(Bw).permutation(Bw))
        _, rows_p, dp_p, _ = run_entry(p[perm], t[perm], dev)
        assert torch.equal(rows_p.cpu(), rows.cpu()[perm]) and torch.equal(dp_p.cpu(), dp.cpu()[perm])


@pytest.mark.parametrize("B,C", [(128, 2), (33, 17), (6, 3129)])
def test_one_hot_target_agrees_with_the_integer_route(dev, B, C):
    from meant_amd import _lib
    from meant_amd.train import cross_entropy_on_probs
    g = torch.Generator().manual_seed(C)
    p = torch.rand(B, C, generator=g)
    idx = torch.randint(0, C, (B,), generator=g)
    res = []
    for target in (idx, F.one_hot(idx, C).float()):
        pg = p.to(dev).requires_grad_(True)
        _lib.route_reset()
        loss = cross_entropy_on_probs(pg, target.to(dev))
        loss.backward()
        res.append((loss.detach().cpu(), pg.grad.cpu(), _lib.route_count("ce_soft_wave") + _lib.route_count("ce_soft_block")))
    (li, gi, ni), (ls, gs, ns) = res
    assert ni == 0 and ns == 1                                         # the integer route did not touch the new counters
    assert abs(li.item() - ls.item()) <= 1e-5 and (gi - gs).abs().max().item() <= 1e-6


# ---- TrainStep ---------------------------------------------------------------------------------------------------------------------
def _tiny_vqa(dev):
    import meant_amd
    torch.manual_seed(0)
    m = meant_amd.meant_vqa(128, 128, 4, 32, 32, 16, 1, 7, torch.nn.Embedding(100, 128), num_heads=2).to(dev).eval()
    m.compute_dtype = torch.bfloat16
    return m


def _batch(B, dev, seed):
    rs = np.random.RandomState(seed)
    ids = torch.from_numpy(rs.randint(0, 100, (B, 16)).astype("int64")).to(dev)
    img = torch.from_numpy(rs.standard_normal((B, 4, 32, 32)).astype("float32")).to(dev)
    return ids, img, torch.ones(B, 16, device=dev), make_target(B, 7, seed).to(dev)


def test_train_step_with_soft_targets_and_the_score(dev):
    from meant_amd import _lib, vqa_score
    from meant_amd.train import TrainStep, cross_entropy_on_probs
    B = 8
    model = _tiny_vqa(dev)
    score = vqa_score("train")
    ts = TrainStep(model, lr=1e-3, metrics=score)
    ids, img, mask, soft = _batch(B, dev, 1)
    ts(ids, img, mask, target=soft)                                    # the first step builds the rotary tables and the weight caches
    before = [q.detach().clone() for q in model.parameters()]
    ids, img, mask, soft = _batch(B, dev, 2)
    torch.cuda.synchronize()
    _lib.route_reset()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, out = ts(ids, img, mask, target=soft)                    # nothing in the step reads the device ...
        with pytest.raises(RuntimeError):
            score.state.cpu()                                          # ... which this mode would have refused
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert _lib.route_count("ce_soft_wave") == 1 and _lib.route_count("vqa_score") == 1
    assert out.shape == (B, 7) and loss.dim() == 0
    assert torch.equal(loss, cross_entropy_on_probs(out, soft))
    assert any(not torch.equal(a, q.detach()) for a, q in zip(before, model.parameters()))
    state = score.state.cpu()
    assert state[1].item() == 2 * B and score.nan_rows() == 0 and score.invalid_rows() == 0
    assert 0.0 <= score.compute().item() <= 1.0


def test_train_step_micro_batches_slice_soft_targets(dev):
    from meant_amd.train import TrainStep, cross_entropy_on_probs
    B = 8
    ts = TrainStep(_tiny_vqa(dev), lr=1e-3, micro_batches=2)
    ids, img, mask, soft = _batch(B, dev, 3)
    loss, out = ts(ids, img, mask, target=soft)
    halves = [cross_entropy_on_probs(out[i * 4:(i + 1) * 4], soft[i * 4:(i + 1) * 4]) * (1.0 / 2) for i in range(2)]
    assert out.shape == (B, 7) and torch.equal(loss, 0.0 + halves[0] + halves[1])
