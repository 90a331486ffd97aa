"""The classification counts on the device (meant_metrics_update / meant_metrics_update_labels, meant_amd.f1_metrics) against counts
made on the CPU with torch.argmax and numpy.bincount from the same tensors.  Every comparison is exact (torch.equal on int64): the
counters are integers.  The state and the confusion matrix always sit in the middle of a larger int64 buffer of sentinel values,
which must be unchanged afterwards.  Shapes are the smallest that reach each edge: one lane, the wave edge, past one workgroup,
several workgroups for the lane-per-row form (C <= 16); the lane and 16-byte-chunk boundaries, rows with and without 16-byte
alignment and the unrolled main loop (C = 3129) for the wave-per-row form."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
IGNORE = -100
SENTINEL = -0x0123456789ABCDEF
PAD = 24
DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- the CPU side -----------------------------------------------------------------------------------------------------------
def cpu_counts(C, target, scores=None, pred=None, ignore_index=IGNORE):
    """state int64 [3C + 4] and confusion int64 [C, C] from CPU tensors: torch.argmax over the class columns, numpy.bincount"""
    target = target.cpu().numpy().astype(np.int64)
    if scores is not None:
        cls = scores.cpu()[:, :C]
        pred = torch.argmax(cls, dim=1).numpy().astype(np.int64)
        has_nan = torch.isnan(cls.float()).any(dim=1).numpy()
    else:
        pred = pred.cpu().numpy().astype(np.int64)
        has_nan = np.zeros(len(target), dtype=bool)
    ignored = target == ignore_index
    valid = ~ignored & (target >= 0) & (target < C) & (pred >= 0) & (pred < C)
    p, t = pred[valid], target[valid]
    state = np.concatenate([np.bincount(p[p == t], minlength=C), np.bincount(p, minlength=C), np.bincount(t, minlength=C),
                            [valid.sum(), ignored.sum(), (~ignored & ~valid).sum(), (has_nan & valid).sum()]]).astype(np.int64)
    conf = np.bincount(t * C + p, minlength=C * C).reshape(C, C).astype(np.int64)
    return torch.from_numpy(state), torch.from_numpy(conf)


# ---- the device side, at the C ABI ----------------------------------------------------------------------------------------------
class Guarded:
    """a zeroed int64 [n] in the middle of sentinels"""

    def __init__(self, n, dev):
        self.buf = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.int64, device=dev)
        self.t = self.buf[PAD:PAD + n]
        self.t.zero_()

    def cpu(self):
        b = self.buf.cpu()
        assert (b[:PAD] == SENTINEL).all() and (b[-PAD:] == SENTINEL).all(), "wrote outside its buffer"
        return b[PAD:-PAD].clone()


def dev_update(C, target, scores=None, pred=None, state=None, conf=None, ignore_index=IGNORE):
    """one call on device tensors; scores may be any [B, >= C] view with unit column stride"""
    from meant_amd import _lib, ops
    dev = target.device
    state = state or Guarded(3 * C + 4, dev)
    conf = conf or Guarded(C * C, dev)
    st = torch.cuda.current_stream().cuda_stream
    B = target.shape[0]
    if scores is not None:
        assert scores.stride(1) == 1 and (B == 1 or scores.stride(0) >= C)
        _lib.check(_lib.lib.meant_metrics_update(scores.data_ptr(), scores.stride(0) if B > 1 else scores.shape[1], ops._dt(scores),
                                                 target.data_ptr(), B, C, ignore_index, state.t.data_ptr(), conf.t.data_ptr(), st))
    else:
        _lib.check(_lib.lib.meant_metrics_update_labels(pred.data_ptr(), target.data_ptr(), B, C, ignore_index, state.t.data_ptr(),
                                                        conf.t.data_ptr(), st))
    return state, conf


def check(C, target_cpu, scores_view, scores_cpu, route):
    """device counts of one update == CPU counts; the route counter names the form that ran"""
    from meant_amd import _lib
    _lib.route_reset()
    state, conf = dev_update(C, target_cpu.to(scores_view.device), scores=scores_view)
    want_state, want_conf = cpu_counts(C, target_cpu, scores=scores_cpu)
    got_state, got_conf = state.cpu(), conf.cpu()
    assert torch.equal(got_state, want_state), (got_state, want_state)
    assert torch.equal(got_conf.view(C, C), want_conf)
    assert _lib.route_count(route) == 1 and sum(_lib.route_count(r) for r in ("metrics_rows", "metrics_wave", "metrics_labels")) == 1
    return got_state


def plant_ties(s, C):
    """the row maximum duplicated at (7, 8), (63, 64) and (C - 1, 0), one pair per row in turn (every fourth row left alone)"""
    pairs = [(7, 8), (63, 64), (C - 1, 0)]
    top = s[:, :C].float().max(dim=1).values + 1.0
    for r in range(s.shape[0]):
        k = r % 4
        if k < 3 and max(pairs[k]) < C:
            s[r, pairs[k][0]] = s[r, pairs[k][1]] = top[r]
    return s


def make_scores(B, C, ld, dtype, dev, seed, offset=0, pad_value=float("inf"), ties=False):
    """CPU scores [B, ld] (a fifth of the rows rounded to one decimal: ties; the padding columns set to pad_value) and the same
    values as a device view whose first element sits `offset` elements into its allocation"""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(B, ld, generator=g)
    s[::5] = torch.round(s[::5], decimals=1)
    s[:, C:] = pad_value
    s = s.to(dtype)
    if ties:
        s = plant_ties(s, C)
    flat = torch.zeros(B * ld + 16, dtype=dtype, device=dev)
    view = flat[offset:offset + B * ld].view(B, ld)
    view.copy_(s)
    return s, view


def make_target(B, C, seed):
    return torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(1000 + seed))


# ---- rows form --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [2, 3, 16])
def test_rows_form(dev, C, dtype):
    for B in (1, 63, 64, 65, 257, 1000):
        for ld in (C, C + 5):
            s, view = make_scores(B, C, ld, dtype, dev, seed=B + ld)
            t = make_target(B, C, B)
            st = check(C, t, view, s, "metrics_rows")
            assert st[3 * C].item() == B
    # more rows than one pass of the capped grid covers: the stride loop
    B = 1024 * 256 + 77
    s, view = make_scores(B, C, C, dtype, dev, seed=9)
    check(C, make_target(B, C, 9), view, s, "metrics_rows")


# ---- wave form --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [17, 64, 65, 1000, 3129])
def test_wave_form(dev, C, dtype):
    ld8 = (C + 7) // 8 * 8
    for B in (1, 5, 300):
        for ld, offset in ((ld8, 0), (ld8 + 8, 0), (ld8, 1), (ld8 + 3, 0), (C if C % 8 else C + 1, 0)):
            s, view = make_scores(B, C, ld, dtype, dev, seed=B + ld + offset, offset=offset, ties=True)
            assert (view.data_ptr() % 16 == 0) == (offset == 0)
            t = make_target(B, C, B + ld)
            st = check(C, t, view, s, "metrics_wave")
            assert st[3 * C].item() == B
            pred = torch.argmax(s[:, :C], dim=1)
            for r in range(min(B, 4)):                       # the lower index of each planted pair won
                want = {0: 7, 1: 63, 2: 0}.get(r % 4)
                if want is not None and max(((7, 8), (63, 64), (C - 1, 0))[r % 4]) < C:
                    assert pred[r].item() == want


def test_wave_form_all_minus_inf_and_more_rows_than_the_grid(dev):
    """rows of -inf only (the prediction is column 0, whichever lane holds it) and a batch beyond the capped grid's first pass"""
    from meant_amd import _lib
    C = 40
    for dtype in DTYPES:
        s = torch.full((6, 40), float("-inf")).to(dtype)
        s[1, 33] = -1e30
        s[2, 39] = float("-inf")
        view = s.to(dev)
        check(C, torch.tensor([0, 33, 0, 5, 39, IGNORE]), view, s, "metrics_wave")
    B = 64 * _lib.lib.meant_num_cus() + 301                  # beyond 16 waves x 4 workgroups per CU
    s, view = make_scores(B, 24, 24, torch.bfloat16, dev, seed=4)
    check(24, make_target(B, 24, 4), view, s, "metrics_wave")


# ---- NaN ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,ld,route", [(2, 2, "metrics_rows"), (16, 21, "metrics_rows"), (17, 24, "metrics_wave"), (65, 65, "metrics_wave"),
                                         (1000, 1000, "metrics_wave"), (3129, 3136, "metrics_wave")])
def test_nan_rows(dev, C, ld, route, dtype):
    B = 70
    nan, inf = float("nan"), float("inf")
    s, _ = make_scores(B, C, ld, dtype, dev, seed=C, pad_value=0.0)
    hi = C - 1
    mid = C // 2
    s[3, hi] = nan                                        # one NaN, last column
    s[4, 0] = nan                                         # first column
    s[5, mid] = nan; s[5, hi] = nan                       # two: the first one is the prediction
    s[6, 0] = inf; s[6, hi] = nan                         # beside a +inf at a lower ...
    s[7, hi] = inf; s[7, 0 if C == 2 else mid] = nan      # ... and at a higher index
    s[8, :C] = nan                                        # a row of nothing else
    s[66, 1] = nan                                        # in the second wave of the lane-per-row form
    if ld > C:
        s[9, C:] = nan                                    # padding only: not a NaN row
        s[10, C] = nan; s[10, 0] = inf
    view = s.to(dev)
    t = make_target(B, C, C)
    st = check(C, t, view, s, route)
    assert st[3 * C + 3].item() == 7
    pred = torch.argmax(s[:, :C], dim=1)
    assert pred[3] == hi and pred[4] == 0 and pred[5] == mid and pred[6] == hi and pred[8] == 0      # what torch does, spelled out


# ---- targets ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,route", [(3, "metrics_rows"), (100, "metrics_wave")])
def test_targets_outside_the_classes(dev, C, route):
    B = 333
    s, view = make_scores(B, C, C + 3, torch.float32, dev, seed=1)
    t = make_target(B, C, 1)
    t[::7] = IGNORE
    t[1::11] = -1
    t[2::13] = C
    t[3::17] = 1 << 40
    t[4::19] = -(1 << 40)
    st = check(C, t, view, s, route)
    n_ign = int((t == IGNORE).sum())
    n_inv = int(((t != IGNORE) & ((t < 0) | (t >= C))).sum())
    assert n_ign > 0 and n_inv > 0
    assert st[3 * C:].tolist() == [B - n_ign - n_inv, n_ign, n_inv, 0]
    # a row that is left out is not read either: NaN scores there count nowhere
    s2 = s.clone()
    s2[t == IGNORE] = float("nan")
    s2[t == C] = float("nan")
    st2 = check(C, t, s2.to(dev), s2, route)
    assert torch.equal(st2, st)
    # another ignore index
    t3 = make_target(B, C, 2)
    t3[::3] = -1
    state, _ = dev_update(C, t3.to(dev), scores=view, ignore_index=-1)
    assert torch.equal(state.cpu(), cpu_counts(C, t3, scores=s, ignore_index=-1)[0])


# ---- accumulation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 70])
def test_updates_accumulate_and_repeat_bit_for_bit(dev, C):
    sizes = (1, 7, 64, 130, 300)
    parts = [make_scores(B, C, C, torch.bfloat16, dev, seed=B) for B in sizes]
    targets = [make_target(B, C, B) for B in sizes]
    for t in targets:
        t[::9] = IGNORE
    runs = []
    for _ in range(2):
        state, conf = Guarded(3 * C + 4, dev), Guarded(C * C, dev)
        for (s, view), t in zip(parts, targets):
            dev_update(C, t.to(dev), scores=view, state=state, conf=conf)
        runs.append((state.cpu(), conf.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    all_s, all_t = torch.cat([s for s, _ in parts]), torch.cat(targets)
    once, once_conf = dev_update(C, all_t.to(dev), scores=all_s.to(dev))
    assert torch.equal(once.cpu(), runs[0][0]) and torch.equal(once_conf.cpu(), runs[0][1])
    assert torch.equal(runs[0][0], cpu_counts(C, all_t, scores=all_s)[0])


# ---- labels, confusion ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 16, 17, 3129])
def test_update_labels_equals_update(dev, C):
    from meant_amd import _lib
    B = 777
    s, view = make_scores(B, C, C, torch.float32, dev, seed=C)
    t = make_target(B, C, C)
    t[::10] = IGNORE
    t[5::31] = C + 2
    a, ac = dev_update(C, t.to(dev), scores=view)
    pred = torch.argmax(s, dim=1)
    _lib.route_reset()
    b, bc = dev_update(C, t.to(dev), pred=pred.to(dev))
    assert _lib.route_count("metrics_labels") == 1
    assert torch.equal(a.cpu(), b.cpu()) and torch.equal(ac.cpu(), bc.cpu())
    pred[7::23] = -3                                         # a prediction outside the classes: an invalid row
    pred[8::29] = C
    c, cc = dev_update(C, t.to(dev), pred=pred.to(dev))
    want, want_conf = cpu_counts(C, t, pred=pred)
    assert torch.equal(c.cpu(), want) and torch.equal(cc.cpu().view(C, C), want_conf)
    assert want[3 * C + 2] > b.cpu()[3 * C + 2]


@pytest.mark.parametrize("C", [5, 40])
def test_confusion_matrix(dev, C):
    from meant_amd import f1_metrics
    m = f1_metrics(C, "Val", confusion=True)
    all_s, all_t = [], []
    for B in (50, 300):
        s, view = make_scores(B, C, C, torch.float32, dev, seed=B + C)
        t = make_target(B, C, B + C)
        t[::6] = IGNORE
        m.update(view, t.to(dev))
        all_s.append(s); all_t.append(t)
    want_state, want_conf = cpu_counts(C, torch.cat(all_t), scores=torch.cat(all_s))
    conf = m.confusion_matrix()
    state = m.state.cpu()
    assert torch.equal(conf, want_conf) and torch.equal(state, want_state)
    assert torch.equal(conf.sum(dim=1), state[2 * C:3 * C]) and torch.equal(conf.sum(dim=0), state[C:2 * C])
    assert conf.diagonal().sum() == state[:C].sum() and conf.sum() == state[3 * C]
    with pytest.raises(RuntimeError):
        f1_metrics(C, "Val").confusion_matrix()


# ---- the class ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,B,dtype", [(3129, 300, torch.bfloat16), (2, 128, torch.float32)])
def test_class_surface(dev, C, B, dtype, capsys):
    from meant_amd import f1_metrics
    s, view = make_scores(B, C, (C + 7) // 8 * 8, dtype, dev, seed=C)
    t = make_target(B, C, C)
    t[::8] = IGNORE
    want_state, _ = cpu_counts(C, t, scores=s)
    want = tuple(v.float() for v in f1_metrics.from_counts(want_state, C))
    m = f1_metrics(C, "Test")
    m.update(view[:, :C], t.to(dev))                         # a column slice of the padded block, read in place
    assert torch.equal(m.state.cpu(), want_state)
    got = m.compute()
    assert len(got) == 7 and all(g.dim() == 0 and g.dtype == torch.float32 and torch.equal(g, w) for g, w in zip(got, want))
    assert got[0] == got[2] == got[4] == got[6]
    f1_macro, f1_micro = m.show(_class=1)
    assert torch.equal(f1_macro, want[1]) and torch.equal(f1_micro, want[2])
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].startswith("Test accuracy: ") and lines[1].startswith("Macro Test f1: ") and len(lines) == 10
    p, r, f1, support = m.per_class()
    assert torch.equal(support, want_state[2 * C:3 * C]) and torch.equal(p, f1_metrics.per_class_from_counts(want_state, C)[0])
    assert m.nan_rows() == 0 and m.invalid_rows() == 0
    # CPU tensors (what the reference loop hands over), float16 scores, integer labels: the same counts
    for scores in (s[:, :C], s[:, :C].to(torch.float16).to(dev), torch.argmax(s[:, :C], dim=1), torch.argmax(s[:, :C], dim=1).int().to(dev)):
        m2 = f1_metrics(C, "Test")
        m2.update(scores, t if not scores.is_cuda else t.to(dev))
        ref = s[:, :C].to(torch.float16) if scores.dtype == torch.float16 else s
        assert torch.equal(m2.state.cpu(), cpu_counts(C, t, scores=ref)[0])
    # merge, reset, state as a plain tensor
    m2.merge(m)
    assert torch.equal(m2.state.cpu(), 2 * want_state) and m2.state.dtype == torch.int64 and m2.state.is_cuda
    m2.reset()
    assert not m2.state.any() and [v.item() for v in m2.compute()] == [0.0] * 7
    with pytest.raises(ValueError):
        m.update(view[:, :C - 1], t.to(dev))


def test_update_does_not_synchronise(dev):
    """with device tensors update() launches and returns: under torch's sync debug mode "error" nothing raises (the control: reading
    the state in the same mode does)"""
    from meant_amd import f1_metrics
    cases = []
    for C, B, dtype in ((2, 128, torch.float32), (3129, 64, torch.bfloat16), (7, 33, torch.float16)):
        s, view = make_scores(B, C, C, dtype, dev, seed=C)
        m = f1_metrics(C, "Train", confusion=True, device=dev)
        cases.append((m, s, view, make_target(B, C, C).to(dev), torch.argmax(s, dim=1).to(dev)))
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for m, s, view, t, labels in cases:
            m.update(view, t)
            m.update(labels, t)
        with pytest.raises(RuntimeError):
            cases[0][0].state.cpu()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    for m, s, view, t, labels in cases:
        assert torch.equal(m.state.cpu(), 2 * cpu_counts(m.num_classes, t, scores=s)[0])


# ---- the train step and the evaluation loop ----------------------------------------------------------------------------------------
def _tiny(dev):
    import meant_amd
    torch.manual_seed(0)
    m = meant_amd.meant(128, 128, 4, 32, 32, 16, 3, 2, torch.nn.Embedding(100, 128), num_heads=2, num_encoders=1).to(dev).eval()
    m.compute_dtype = torch.bfloat16
    return m


def _batches(dev, n, B=8):
    rs = np.random.RandomState(3)
    out = []
    for _ in range(n):
        ids = torch.from_numpy(rs.randint(0, 100, (B, 3, 16)).astype("int64")).to(dev)
        img = torch.from_numpy(rs.standard_normal((B, 3, 4, 32, 32)).astype("float32")).to(dev)
        mask = torch.ones(B, 3, 16, device=dev)
        mask[1, :, 11:] = 0
        out.append((ids, img, mask, torch.from_numpy(rs.randint(0, 2, (B,)).astype("int64")).to(dev)))
    return out


@pytest.mark.parametrize("micro_batches", [1, 2])
def test_train_step_feeds_the_metrics_and_changes_nothing_else(dev, micro_batches):
    """two steps with metrics=m: m's state is the counts of the two returned outputs, and the parameters are bit-equal to a run
    without metrics (option `deterministic`: the step's float reductions in one order, so that two runs can be compared at all)"""
    from meant_amd import _lib, f1_metrics
    from meant_amd.train import TrainStep
    old = _lib.get_option("deterministic")
    _lib.set_option("deterministic", 1)
    try:
        data = _batches(dev, 2)
        params, outs = [], []
        for with_metrics in (True, False):
            model = _tiny(dev)
            m = f1_metrics(2, "Train") if with_metrics else None
            ts = TrainStep(model, lr=1e-3, micro_batches=micro_batches, metrics=m)
            _lib.route_reset()
            for ids, img, mask, tgt in data:
                _, out = ts(ids, img, mask, target=tgt)
                if with_metrics:
                    outs.append((out.cpu(), tgt.cpu()))
            assert _lib.route_count("metrics_rows") == (2 if with_metrics else 0)
            params.append([p.detach().cpu().clone() for p in model.parameters()])
            if with_metrics:
                state = m.state.cpu()
        want = sum(cpu_counts(2, t, scores=o)[0] for o, t in outs)
        assert torch.equal(state, want) and state[6].item() == 16
        assert all(torch.equal(a, b) for a, b in zip(*params))
        fresh = [p.detach().cpu() for p in _tiny(dev).parameters()]
        assert sum(not torch.equal(a, b) for a, b in zip(params[0], fresh)) > len(fresh) // 2      # and the steps did train
    finally:
        _lib.set_option("deterministic", old)


def test_evaluate(dev):
    from meant_amd import _lib, f1_metrics
    from meant_amd.train import evaluate
    model = _tiny(dev)
    data = _batches(dev, 3, B=5)
    with torch.no_grad():
        outs = [model(*b[:3]).cpu() for b in data]
    want = sum(cpu_counts(2, b[3], scores=o)[0] for o, b in zip(outs, data))
    for training in (True, False):
        model.train(training)
        m = f1_metrics(2, "Val")
        _lib.route_reset()
        assert evaluate(model, data, m) is m
        assert model.training == training
        assert _lib.route_count("metrics_rows") == 3
        assert torch.equal(m.state.cpu(), want) and want[6].item() == 15
    m = f1_metrics(2, "Val")                                  # the target first in each batch
    evaluate(model, [(b[3], b[0], b[1], b[2]) for b in data], m, target_index=0)
    assert torch.equal(m.state.cpu(), want)
    model.train()

    class Boom(RuntimeError):
        pass

    def broken():
        yield data[0]
        raise Boom()
    with pytest.raises(Boom):
        evaluate(model, broken(), f1_metrics(2, "Val"))
    assert model.training                                     # restored on the way out of a failure too
