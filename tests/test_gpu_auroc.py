"""AUROC on the device (meant_score_capture, meant_auroc_rank, meant_amd.auroc / metric_group) against numpy on the host.

The reference makes the keys by the same bit rule (the float32 bits, -0.0 first made +0.0, the sign bit flipped for a non-negative
value and all bits for a negative one) and counts 2U = sum over positives of searchsorted(neg, k, 'left') + searchsorted(neg, k,
'right').  The triples (2U, P, N) must be EQUAL: every quantity is an integer.  Sizes sit around a wave's 64 and the sort / scan tile
of 2048; n = 600 001 has more than 256 tiles, so that the carry loop of the scan of the tile sums runs more than once.  n = 1 cannot
hold a positive and a negative; every other case has both unless it is the degenerate one."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
IGNORE = -100
SIZES = [1, 2, 63, 64, 65, 2047, 2048, 2049, 4097]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- the host side --------------------------------------------------------------------------------------------------------------
def np_keys(x):
    """uint32 keys of float32 scores, any shape"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    return np.where(b & 0x80000000, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def np_labels(cols, target, C):
    """int32 labels of the rows: the target, or -1 for a row left out; and the counters n_rows, n_ignored, n_invalid, n_nan"""
    target = np.asarray(target, dtype=np.int64)
    ignored = target == IGNORE
    invalid = ~ignored & ((target < 0) | (target >= C))
    nan = ~ignored & ~invalid & np.isnan(cols.reshape(len(target), -1)).any(axis=1)
    valid = ~ignored & ~invalid & ~nan
    return np.where(valid, target, -1).astype(np.int32), [int(valid.sum()), int(ignored.sum()), int(invalid.sum()), int(nan.sum())]


def np_triple(keys, labels, positive):
    pos = np.sort(keys[labels == positive])
    neg = np.sort(keys[(labels >= 0) & (labels != positive)])
    u2 = (np.searchsorted(neg, pos, "left").astype(np.int64) + np.searchsorted(neg, pos, "right").astype(np.int64)).sum()
    return [int(u2), len(pos), len(neg)]


def want_statistic(scores, target, C, pos_label=1):
    """scores: float32 numpy [n] (C == 2, the positive class's score) or [n, C]"""
    if C == 2:
        cols = scores.reshape(len(target), -1)
        cols = cols[:, pos_label:pos_label + 1] if cols.shape[1] == 2 else cols
        labels, counters = np_labels(cols, target, C)
        return torch.tensor([np_triple(np_keys(cols[:, 0]), labels, pos_label)]), counters
    labels, counters = np_labels(scores, target, C)
    keys = np_keys(scores)
    return torch.tensor([np_triple(keys[:, c], labels, c) for c in range(C)]), counters


def make_scores(kind, n, rs):
    if kind == "normal":
        return rs.standard_normal(n).astype(np.float32)
    if kind == "quantised":
        return rs.randint(0, 4, n).astype(np.float32) * 0.25 - 0.5
    if kind == "equal":
        return np.full(n, 0.625, dtype=np.float32)
    assert kind == "mix"                                  # all four digits of the key: both signs, every exponent range, specials
    with np.errstate(over="ignore"):
        wide = (rs.standard_normal(n) * 10.0 ** rs.uniform(-44, 38, n)).astype(np.float32)
    pool = np.array([np.inf, -np.inf, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 0.0, -0.0, -3e38, -1e30, 3e38, 1.0, -1.0], dtype=np.float32)
    return np.where(rs.rand(n) < 0.5, pool[rs.randint(0, len(pool), n)], wide).astype(np.float32)


def make_target(n, C, rs):
    t = rs.randint(0, C, n).astype(np.int64)
    t[:min(n, C)] = np.arange(C)[::-1][:min(n, C)]         # every class occurs: a positive and a negative for every column (n >= 2)
    return t


def feed(m, scores, target, dev):
    m.update(torch.from_numpy(scores).to(dev), torch.from_numpy(target).to(dev))
    return m


def counters_of(m):
    return m.counters.cpu().tolist()


# ---- sizes and score patterns -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["normal", "quantised", "equal", "mix"])
@pytest.mark.parametrize("n", SIZES)
def test_triple_is_exact(dev, n, kind):
    from meant_amd import _lib, auroc
    rs = np.random.RandomState(n + len(kind))
    scores, target = make_scores(kind, n, rs), make_target(n, 2, rs)
    want, counters = want_statistic(scores, target, 2)
    _lib.route_reset()
    m = feed(auroc(2, "Val"), scores, target, dev)
    got = m.statistic()
    assert got.dtype == torch.int64 and got.device.type == "cpu" and torch.equal(got, want), (got, want)
    assert _lib.route_count("score_capture") == 1 and _lib.route_count("auroc_rank") == 1
    assert counters_of(m) == counters == [n, 0, 0, 0]
    assert np.array_equal(m.keys[0, :n].cpu().numpy().view(np.uint32), np_keys(scores))       # the captured keys themselves
    assert np.array_equal(m.labels[:n].cpu().numpy(), target.astype(np.int32))
    if n >= 2:
        P, N = want[0, 1].item(), want[0, 2].item()
        assert P >= 1 and N >= 1
        if kind == "equal":
            assert got[0, 0].item() == P * N                  # one run of equal keys across every tile boundary: AUROC 1/2
            assert m.compute().item() == 0.5
        assert abs(m.compute().item() - want[0, 0].item() / (2 * P * N)) <= 1e-7
    else:
        assert math.isnan(m.compute().item())


def test_many_tiles(dev):
    """600 001 rows are 293 tiles: the scan of the tile sums carries from one round of 256 tiles into the next; scores rounded to
    two decimals tie in runs that cross tile boundaries"""
    from meant_amd import auroc
    n = 600001
    rs = np.random.RandomState(5)
    target = make_target(n, 2, rs)
    scores = np.round(rs.standard_normal(n) + 0.5 * target, 2).astype(np.float32)
    want, counters = want_statistic(scores, target, 2)
    m = feed(auroc(2, "Val", capacity=1 << 20), scores, target, dev)
    got = m.statistic()
    assert torch.equal(got, want), (got, want)
    assert torch.equal(m.statistic(), got)
    assert counters_of(m) == counters
    assert 0.55 < m.compute().item() < 0.75


def test_signed_zeros_tie(dev):
    from meant_amd import auroc
    scores = np.array([-0.0, 0.0, 0.0, -0.0, -0.0, 0.0], dtype=np.float32)
    target = np.array([1, 0, 1, 0, 1, 0], dtype=np.int64)
    m = feed(auroc(2), scores, target, dev)
    assert m.statistic().tolist() == [[9, 3, 3]] and m.compute().item() == 0.5
    keys = m.keys[0, :6].cpu().numpy().view(np.uint32)
    assert (keys == 0x80000000).all()
    scores = np.array([-0.0, -1.4e-45, 0.0, 1.4e-45], dtype=np.float32)          # the denormals next to zero stay apart from it
    m = feed(auroc(2), scores, np.array([1, 0, 0, 1], dtype=np.int64), dev)
    assert m.statistic().tolist() == [[2 * 1 + 1 + 2 * 2, 2, 2]]


@pytest.mark.parametrize("pos_label", [1, 0])
def test_bf16_block_read_in_place(dev, pos_label):
    """the two class columns of a padded [B, 8] bfloat16 block, handed over as a view: read where they are (row stride 8)"""
    from meant_amd import _lib, auroc
    n = 2049
    rs = np.random.RandomState(8)
    block = torch.from_numpy(rs.standard_normal((n, 8)).astype(np.float32)).bfloat16()
    block[::5, 2:4] = float("nan")                          # NaNs next to the class columns: never captured
    target = make_target(n, 2, rs)
    for first in (0, 4):                                    # the block's start, and two columns inside it
        view_cpu = block[:, first:first + 2]
        want, counters = want_statistic(view_cpu.float().numpy(), target, 2, pos_label)
        d = block.to(dev)
        view = d[:, first:first + 2]
        assert view.stride(0) == 8 and not view.is_contiguous()
        _lib.route_reset()
        m = auroc(2, "Val", pos_label=pos_label)
        m.update(view, torch.from_numpy(target).to(dev))
        assert _lib.route_count("score_capture") == 1
        assert torch.equal(m.statistic(), want) and counters_of(m) == counters == [n, 0, 0, 0]
        assert want[0, 1].item() >= 1 and want[0, 2].item() >= 1


def test_float16_and_float64_scores(dev):
    from meant_amd import auroc
    n = 65
    rs = np.random.RandomState(9)
    target = make_target(n, 2, rs)
    base = rs.standard_normal((n, 2))
    for dtype in (torch.float16, torch.float64):
        s = torch.from_numpy(base).to(dtype)
        want, _ = want_statistic(s.float().numpy(), target, 2)
        m = auroc(2)
        m.update(s.to(dev), torch.from_numpy(target).to(dev))
        assert torch.equal(m.statistic(), want)


# ---- degenerate and left-out rows ---------------------------------------------------------------------------------------------------
def test_all_targets_positive(dev):
    from meant_amd import auroc
    n = 300
    scores = np.random.RandomState(1).standard_normal(n).astype(np.float32)
    m = feed(auroc(2), scores, np.ones(n, dtype=np.int64), dev)
    assert m.statistic().tolist() == [[0, n, 0]]
    v = m.compute()
    assert v.dtype == torch.float32 and v.dim() == 0 and math.isnan(v.item())
    assert torch.isnan(m.per_class()).all()


@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("n", [65, 2049])
def test_left_out_rows(dev, n, C):
    """rows with the ignore index, with a target outside [0, C) and with a NaN score: out of the triples, each in its counter; less
    than a quarter of the rows in all"""
    from meant_amd import auroc
    rs = np.random.RandomState(n + C)
    scores, target = rs.standard_normal((n, C)).astype(np.float32), make_target(n, C, rs)
    k = n // 16
    rows = rs.permutation(np.arange(C, n))[:3 * k]          # the first C rows keep every class present
    target[rows[:k]] = IGNORE
    target[rows[k:2 * k]] = np.array([-1, C, 7, -(1 << 40), 1 << 40])[np.arange(k) % 5]
    cols = rs.randint(0, C, k)
    cols[0] = 1
    scores[rows[2 * k:], cols] = np.nan                     # in any one column; at C == 2 only column 1 is captured
    scores[rows[:k // 2], 0] = np.nan                       # a NaN in an ignored row is not looked at
    want, counters = want_statistic(scores, target, C)
    assert counters[1] == k and counters[2] == k and 1 <= counters[3] <= k and 4 * (n - counters[0]) <= n
    assert (want[:, 1] >= 1).all() and (want[:, 2] >= 1).all()
    m = feed(auroc(C, "Val"), scores, target, dev)
    got = m.statistic()
    assert torch.equal(got, want), (got, want)
    assert counters_of(m) == counters
    assert m.nan_rows() == counters[3] and m.invalid_rows() == counters[2]
    labels = m.labels[:n].cpu().numpy()
    assert np.array_equal(labels, np_labels(scores[:, 1:2] if C == 2 else scores, target, C)[0])
    assert (m.keys[:, :n].cpu().numpy()[:, labels < 0] == 0).all()                # the keys of a row left out are 0
    m.reset()
    assert m.count == 0 and counters_of(m) == [0, 0, 0, 0] and m.statistic().tolist() == [[0, 0, 0]] * (1 if C == 2 else C)


# ---- batching and growth ------------------------------------------------------------------------------------------------------------
def test_batches_and_growth_give_the_same_triple_without_a_sync(dev):
    """the same 4097 rows as one batch and as uneven batches into capacity 128 (six doublings): identical triples; the updates run
    under torch's sync debug mode "error" and must not raise"""
    from meant_amd import _lib, auroc
    n = 4097
    rs = np.random.RandomState(12)
    scores, target = make_scores("quantised", n, rs) + (rs.rand(n) < 0.3).astype(np.float32), make_target(n, 2, rs)
    target[100:140] = IGNORE
    scores[200:220] = np.nan
    want, counters = want_statistic(scores, target, 2)
    one = feed(auroc(2, "Val"), scores, target, dev)
    sizes, left, cycle = [], n, [1, 7, 64, 129, 300, 1000]
    while left:
        sizes.append(min(left, cycle[len(sizes) % len(cycle)]))
        left -= sizes[-1]
    s, t = torch.from_numpy(scores).to(dev), torch.from_numpy(target).to(dev)
    parts, a = [], 0
    for b in sizes:
        parts.append((s[a:a + b], t[a:a + b]))
        a += b
    m = auroc(2, "Val", capacity=128, device=dev)
    torch.cuda.synchronize()
    _lib.route_reset()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for ps, pt in parts:
            m.update(ps, pt)
        control = False
        try:
            m.counters.cpu()
        except RuntimeError:
            control = True
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert _lib.route_count("score_capture") == len(sizes)
    assert m.count == n and m.capacity == 8192
    got = m.statistic()
    assert torch.equal(got, want) and torch.equal(one.statistic(), want), (got, want)
    assert torch.equal(m.statistic(), got)                  # read twice: the same
    assert counters_of(m) == counters_of(one) == counters
    if not control:
        pytest.skip("this torch build does not raise on a device read under set_sync_debug_mode('error'): the updates ran in that mode "
                    "without raising, which then shows nothing; every other assertion of this test passed")


def test_merge(dev):
    from meant_amd import auroc
    n = 2049
    rs = np.random.RandomState(13)
    scores, target = make_scores("quantised", n, rs), make_target(n, 3, rs)
    scores3 = np.stack([scores, -scores, rs.standard_normal(n).astype(np.float32)], axis=1)
    target[50:60] = IGNORE
    whole = feed(auroc(3), scores3, target, dev)
    a = feed(auroc(3, capacity=256), scores3[:700], target[:700], dev)
    b = feed(auroc(3, capacity=64), scores3[700:], target[700:], dev)
    assert a.merge(b) is a and a.count == n
    assert torch.equal(a.statistic(), whole.statistic()) and counters_of(a) == counters_of(whole)
    fresh = auroc(3).merge(whole)                           # into an object that has seen nothing
    assert torch.equal(fresh.statistic(), whole.statistic())
    with pytest.raises(ValueError):
        auroc(2).merge(whole)


# ---- one-vs-rest and the definition ---------------------------------------------------------------------------------------------------
def test_three_classes_one_vs_rest(dev):
    from meant_amd import _lib, auroc
    n = 2049
    rs = np.random.RandomState(14)
    target = make_target(n, 3, rs)
    scores = (rs.standard_normal((n, 3)) + 1.5 * np.eye(3)[target]).astype(np.float32)
    scores[:, 2] = np.round(scores[:, 2])                   # ties in one column
    want, _ = want_statistic(scores, target, 3)
    _lib.route_reset()
    m = feed(auroc(3, "Val"), scores, target, dev)
    got = m.statistic()
    assert _lib.route_count("score_capture") == 1 and _lib.route_count("auroc_rank") == 3
    assert torch.equal(got, want), (got, want)
    per = want[:, 0].double() / (2 * want[:, 1].double() * want[:, 2].double())
    assert torch.equal(m.per_class(), per) and (per > 0.7).all()
    assert m.compute().item() == per.mean().float().item()
    # class 2 never a target: its column has no positive and is left out of the mean
    target2 = np.where(target == 2, 0, target)
    want2, _ = want_statistic(scores, target2, 3)
    m2 = feed(auroc(3, "Val"), scores, target2, dev)
    assert torch.equal(m2.statistic(), want2) and want2[2].tolist() == [0, 0, n]
    per2 = m2.per_class()
    assert math.isnan(per2[2].item()) and not math.isnan(per2[0].item())
    assert m2.compute().item() == per2[:2].mean().float().item()


@pytest.mark.parametrize("n", [2049, 4097])
def test_compute_matches_scikit_learn(dev, n):
    """a cross-check of the definition (the integer triple is the test): roc_auc_score on the same scores in float64.  Both are
    U / (P N) with U a multiple of 1/2 below 2^24: the integers are exact in float64, and the two divisions round once each"""
    from sklearn.metrics import roc_auc_score
    from meant_amd import auroc
    rs = np.random.RandomState(n)
    target = make_target(n, 2, rs)
    scores = np.round(rs.standard_normal(n) + target, 1).astype(np.float32)
    m = feed(auroc(2), scores, target, dev)
    assert abs(m.per_class()[0].item() - roc_auc_score(target, scores.astype(np.float64))) <= 1e-9
    two = np.stack([-scores, scores], axis=1)               # [n, 2]: the column pos_label
    m = feed(auroc(2), two, target, dev)
    assert abs(m.per_class()[0].item() - roc_auc_score(target, scores.astype(np.float64))) <= 1e-9


# ---- the C ABI next to sentinels ---------------------------------------------------------------------------------------------------
def test_capture_and_rank_write_only_their_slots(dev):
    """columns 2..3 of a [130, 5] block into slots 37..166 of buffers of capacity 300: every other slot, the space around the buffers
    and around `out` keep their sentinel values"""
    from meant_amd import _lib
    B, ld, col0, ncol, cap, off, C = 130, 5, 2, 2, 300, 37, 4
    rs = np.random.RandomState(15)
    scores, target = rs.standard_normal((B, ld)).astype(np.float32), make_target(B, C, rs)
    target[5], target[6], scores[7, 3], scores[8, 0] = IGNORE, C, np.nan, np.nan
    SK, SL, SO = 0x5A5A5A5A, -77, -0x0123456789ABCDEF
    keys = torch.full((ncol * cap + 16,), SK, dtype=torch.int32, device=dev)
    labels = torch.full((cap + 16,), SL, dtype=torch.int32, device=dev)
    out = torch.full((3 + 16,), SO, dtype=torch.int64, device=dev)
    counters = torch.zeros(4, dtype=torch.int64, device=dev)
    s, t = torch.from_numpy(scores).to(dev), torch.from_numpy(target).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    kview, lview, oview = keys[8:8 + ncol * cap], labels[8:8 + cap], out[8:11]
    _lib.check(_lib.lib.meant_score_capture(s.data_ptr(), ld, 0, t.data_ptr(), B, C, col0, ncol, IGNORE, kview.data_ptr(), lview.data_ptr(),
                                            cap, off, counters.data_ptr(), st))
    want_labels, want_counters = np_labels(scores[:, col0:col0 + ncol], target, C)
    want_keys = np.where(want_labels >= 0, np_keys(scores[:, col0:col0 + ncol]).T, 0).astype(np.uint32)
    k = keys.cpu().numpy().view(np.uint32).copy()
    inner = k[8:8 + ncol * cap].reshape(ncol, cap)
    assert np.array_equal(inner[:, off:off + B], want_keys)
    inner[:, off:off + B] = SK
    assert (k == SK).all(), "keys written outside the batch's slots"
    lab = labels.cpu().numpy().copy()
    assert np.array_equal(lab[8 + off:8 + off + B], want_labels)
    lab[8 + off:8 + off + B] = SL
    assert (lab == SL).all(), "labels written outside the batch's slots"
    assert counters.cpu().tolist() == want_counters == [B - 3, 1, 1, 1]
    # the rank of column 1 over the slots in use, class 1 against the rest
    n = B
    wsb = _lib.lib.meant_auroc_ws(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib.meant_auroc_rank(kview[cap + off:].data_ptr(), lview[off:].data_ptr(), n, 1, oview.data_ptr(), ws.data_ptr(), wsb, st))
    o = out.cpu()
    assert o[8:11].tolist() == np_triple(want_keys[1], want_labels, 1)
    assert (o[:8] == SO).all() and (o[11:] == SO).all()
    _lib.check(_lib.lib.meant_auroc_rank(None, None, 0, 1, oview.data_ptr(), None, 0, st))          # n == 0: zeros
    assert out.cpu()[8:11].tolist() == [0, 0, 0]


# ---- under the train step ---------------------------------------------------------------------------------------------------------
def _tiny(dev):
    import meant_amd
    torch.manual_seed(0)
    m = meant_amd.meant(128, 128, 4, 32, 32, 16, 3, 2, torch.nn.Embedding(100, 128), num_heads=2, num_encoders=1).to(dev).eval()
    m.compute_dtype = torch.bfloat16
    return m


def test_metric_group_under_the_train_step(dev, capsys):
    from meant_amd import _lib, auroc, f1_metrics, metric_group
    from meant_amd.train import TrainStep
    rs = np.random.RandomState(3)
    B, steps = 8, 2
    group = metric_group(f1_metrics(2, "t"), auroc(2, "t"))
    ts = TrainStep(_tiny(dev), lr=1e-3, metrics=group)
    outs, targets = [], []
    _lib.route_reset()
    for _ in range(steps):
        ids = torch.from_numpy(rs.randint(0, 100, (B, 3, 16)).astype("int64")).to(dev)
        img = torch.from_numpy(rs.standard_normal((B, 3, 4, 32, 32)).astype("float32")).to(dev)
        tgt = torch.from_numpy(rs.randint(0, 2, (B,)).astype("int64")).to(dev)
        _, out = ts(ids, img, torch.ones(B, 3, 16, device=dev), target=tgt)
        outs.append(out.detach().float().cpu().numpy())
        targets.append(tgt.cpu().numpy())
    assert _lib.route_count("score_capture") == steps and _lib.route_count("metrics_rows") == steps
    f1, au = group.metrics
    assert f1.state[6].item() == B * steps and au.count == B * steps and au.counters[0].item() == B * steps
    want, _ = want_statistic(np.concatenate(outs), np.concatenate(targets), 2)
    assert torch.equal(au.statistic(), want)
    assert -1.0 <= f1.mcc().item() <= 1.0
    shown = group.show()
    assert len(shown) == 2 and "t AUROC" in capsys.readouterr().out
    group.reset()
    assert f1.state.cpu().abs().sum().item() == 0 and au.count == 0
