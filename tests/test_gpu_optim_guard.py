"""GPU tests of the guarded optimizer tail: exact gradient statistics, Adam / AdamW against torch, the skipped step, the
reference's GradScaler recipe step by step, TrainStep end to end, no host read, route counts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SPAN, GRID_CAP = 4096, 2048                      # elements per partial; workgroups per launch (a workgroup strides over spans beyond)
# the vector body, the scalar tail, both sides of a span boundary, a second span of one element, hundreds of spans, and more spans than
# workgroups (the stride over spans wraps)
SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 8193, 1300003, SPAN * GRID_CAP + 4097]
SHAPES = [(768, 768), (768,), (3, 5, 7), (1,), (2304, 768)]          # of test_fused_adamw_matches_torch: several 1 MB buckets
HYPER = dict(lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05)
BOUND = 2e-6                                     # of test_fused_adamw_matches_torch


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ints(n, seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(-3, 4, n).astype(np.float32))


class _Stats:
    """meant_grad_stats_f32 at the C ABI over a list of buckets; the first 16 bytes of the state are (sumsq, nonfinite)"""

    def __init__(self, dev):
        from meant_amd import _lib
        self.lib, self.dev = _lib.lib, dev
        self.state = torch.zeros(_lib.OPTIM_STATE_BYTES, dtype=torch.uint8, device=dev)

    def __call__(self, buckets):
        from meant_amd import _lib, ops
        self.state[:16] = 0xAB                   # stale values: first != 0 has to overwrite them
        ws = torch.empty(max(16, max(self.lib.meant_grad_stats_ws(b.numel()) for b in buckets)), dtype=torch.uint8, device=self.dev)
        for i, b in enumerate(buckets):
            _lib.check(self.lib.meant_grad_stats_f32(b.data_ptr(), b.numel(), self.state.data_ptr(), int(i == 0), ws.data_ptr(), ws.numel(),
                                                     ops._stream()), "grad_stats_f32")
        raw = self.state[:16].cpu()
        return raw.view(torch.float64)[0].item(), raw.view(torch.int64)[1].item(), bytes(raw.numpy())


@pytest.mark.parametrize("n", SIZES)
def test_stats_are_exact_and_reproducible(dev, n):
    """small integers: the sum of squares is an exact integer in float and in double, so `==` against integer arithmetic; one bucket,
    then three (first, add, add).  Random floats: the same bytes on two runs and under either value of `deterministic`."""
    from meant_amd import _lib
    stats = _Stats(dev)
    g = _ints(n, n % 1000)
    want = int((g.long() ** 2).sum())
    sumsq, bad, _ = stats([g.to(dev)])
    assert sumsq == want and bad == 0, (sumsq, want, bad)
    others = [_ints(max(1, n // 2), 7), _ints(5, 8)]
    want3 = want + sum(int((o.long() ** 2).sum()) for o in others)
    sumsq, bad, _ = stats([g.to(dev)] + [o.to(dev) for o in others])
    assert sumsq == want3 and bad == 0, (sumsq, want3, bad)
    x = torch.randn(n, generator=torch.Generator().manual_seed(n % 1000 + 1)) * 3.0
    xd = x.to(dev)
    old = _lib.get_option("deterministic")
    try:
        runs = []
        for det in (0, 0, 1, 1):
            _lib.set_option("deterministic", det)
            runs.append(stats([xd, xd[: (n // 2) & ~3] if n >= 8 else xd]))
    finally:
        _lib.set_option("deterministic", old)
    assert all(r[2] == runs[0][2] for r in runs), [r[:2] for r in runs]
    ref = (x.double() ** 2).sum().item() + ((x[: (n // 2) & ~3] if n >= 8 else x).double() ** 2).sum().item()
    assert abs(runs[0][0] - ref) <= 1e-12 * ref and runs[0][1] == 0        # double squares are exact, the sums are double


@pytest.mark.parametrize("n", [7, 2 * SPAN + 3, 1300003])
def test_stats_count_planted_nonfinite_elements(dev, n):
    """NaN, +inf and -inf at index 0, at n - 1 and inside the scalar tail (n % 4 != 0), on the last element of the first span and the first
    of the second: nonfinite is the number planted, sumsq that of the remaining elements"""
    stats = _Stats(dev)
    g = _ints(n, 3)
    spots = sorted({i for i in (0, n - 1, n - 2, SPAN - 1, SPAN, 2 * SPAN) if 0 <= i < n})
    assert n % 4 and n - 2 >= (n & ~3)                                      # n - 1 and n - 2 are read by the element loads
    for k, i in enumerate(spots):
        g[i] = (float("nan"), float("inf"), float("-inf"))[k % 3]
    keep = torch.ones(n, dtype=torch.bool)
    keep[spots] = False
    want = int((g[keep].long() ** 2).sum())
    sumsq, bad, _ = stats([g.to(dev)])
    assert bad == len(spots) and sumsq == want, (bad, len(spots), sumsq, want)
    sumsq, bad, _ = stats([_ints(9, 1).to(dev), g.to(dev), g.to(dev)])      # counts add up over buckets
    assert bad == 2 * len(spots) and sumsq == 2 * want + int((_ints(9, 1).long() ** 2).sum())


def test_stats_keep_a_norm_beyond_float32(dev):
    """every element finite, the norm past float32's range: sumsq is a double sum and nothing counts as non-finite"""
    g = torch.full((4099,), 1e30)
    sumsq, bad, _ = _Stats(dev)([g.to(dev)])
    assert bad == 0 and abs(sumsq - 4099 * float(np.float32(1e30)) ** 2) <= 1e-12 * sumsq


def _pair(dev, kind, max_norm, seed=1, **kw):
    """the same parameters on the CPU under torch.optim and on the device under GuardedAdam over several buckets"""
    from meant_amd.parallel import GradReducer
    from meant_amd.train import GuardedAdam
    g = torch.Generator().manual_seed(seed)
    ref_params = [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in SHAPES]
    hip_params = [torch.nn.Parameter(p.detach().clone().to(dev)) for p in ref_params]
    ref_opt = (torch.optim.AdamW if kind == "adamw" else torch.optim.Adam)(ref_params, **HYPER)
    red = GradReducer(hip_params, bucket_mb=1.0)
    assert red.num_buckets >= 2
    return g, ref_params, hip_params, ref_opt, red, GuardedAdam(red, kind=kind, max_grad_norm=max_norm, **HYPER, **kw)


def _load(red, hip_params, grads, dev):
    red.prepare()
    for p, gr in zip(hip_params, grads):
        p.grad.copy_(gr.to(dev))
    red.wait()


def _worst(hip_params, ref_params):
    return max((a.detach().cpu() - b.detach()).abs().max().item() for a, b in zip(hip_params, ref_params))


# torch.optim.Adam adds weight_decay * p to the gradient.  Where the two nearly cancel, m / (sqrt(v) + eps) turns a rounding of the sum
# into a visible fraction of lr, in any float32 implementation: on these inputs torch's own float32 step is 1e-5 .. 4.5e-5 away from
# its float64 step without clipping and at max_norm = 1 (5e-7 at max_norm = 1e-3 and in every AdamW mode, where 2e-6 holds).  Those
# two modes are held to 4 x the float32-to-float64 distance of torch itself, measured on the same inputs: the differing order of
# a handful of roundings.
WIDE_MODES = {("adam", None), ("adam", 1.0)}


class _Twin64:
    """torch's optimizer in float64 beside the float32 one, fed the same gradients"""

    def __init__(self, kind, ref_params):
        self.params = [torch.nn.Parameter(p.detach().double().clone()) for p in ref_params]
        self.opt = (torch.optim.AdamW if kind == "adamw" else torch.optim.Adam)(self.params, **HYPER)

    def step(self, grads, max_norm):
        for p, gr in zip(self.params, grads):
            p.grad = gr.double().clone()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(self.params, max_norm)
        self.opt.step()

    def bound(self, kind, max_norm, ref_params):
        if (kind, max_norm) not in WIDE_MODES:
            return BOUND
        return 4.0 * max((a.detach().double() - b.detach()).abs().max().item() for a, b in zip(ref_params, self.params))


@pytest.mark.parametrize("max_norm", [None, 1.0, 1e-3])
@pytest.mark.parametrize("kind", ["adamw", "adam"])
def test_guarded_adam_matches_torch(dev, kind, max_norm):
    """3 steps of clip_grad_norm_ + torch.optim.AdamW / Adam on the CPU against the guarded kernels: the shapes, hyperparameters and
    bound of test_fused_adamw_matches_torch"""
    g, ref_params, hip_params, ref_opt, red, opt = _pair(dev, kind, max_norm)
    twin = _Twin64(kind, ref_params)
    for step in range(3):
        grads = [torch.randn(*s, generator=g) * (10.0 if step == 1 else 0.1) for s in SHAPES]
        for p, gr in zip(ref_params, grads):
            p.grad = gr.clone()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(ref_params, max_norm)
        ref_opt.step()
        twin.step(grads, max_norm)
        _load(red, hip_params, grads, dev)
        opt.step()
        worst, bound = _worst(hip_params, ref_params), twin.bound(kind, max_norm, ref_params)
        print(f"guarded {kind} max_norm={max_norm} step {step}: max abs difference {worst:.3e}, bound {bound:.3e}")
        assert worst < bound, (step, worst, bound)
    assert opt.steps_taken() == 3 and opt.steps_skipped() == 0 and not opt.last_skipped()
    norm = torch.sqrt(sum((gr.double() ** 2).sum() for gr in grads)).item()
    assert abs(opt.last_grad_norm() - norm) <= 1e-6 * norm


@pytest.mark.parametrize("kind", ["adamw", "adam"])
def test_skipped_step_changes_nothing_and_is_not_counted(dev, kind):
    """one inf in one bucket of several: p, m and v keep their bits, the step is counted as skipped; the next clean step is then
    torch's FIRST step (bias corrections with t = 1: the count the kernels use is the device's count of steps taken)"""
    g, ref_params, hip_params, ref_opt, red, opt = _pair(dev, kind, 1.0)
    for m, v in zip(opt.exp_avg, opt.exp_avg_sq):                            # moments that a wrongly taken step would change
        m.fill_(0.25)
        v.fill_(0.5)
    grads = [torch.randn(*s, generator=g) for s in SHAPES]
    grads[2][1, 2, 3] = float("inf")
    _load(red, hip_params, grads, dev)
    before = [[t.clone() for t in ts] for ts in (opt.flat_params, opt.exp_avg, opt.exp_avg_sq)]
    opt.step()
    for old, new in zip(before, (opt.flat_params, opt.exp_avg, opt.exp_avg_sq)):
        assert all(torch.equal(a, b) for a, b in zip(old, new))
    assert opt.steps_taken() == 0 and opt.steps_skipped() == 1 and opt.last_skipped()
    for m, v in zip(opt.exp_avg, opt.exp_avg_sq):
        m.zero_()
        v.zero_()
    grads = [torch.randn(*s, generator=g) for s in SHAPES]
    for p, gr in zip(ref_params, grads):
        p.grad = gr.clone()
    torch.nn.utils.clip_grad_norm_(ref_params, 1.0)
    twin = _Twin64(kind, ref_params)                                         # before torch's step: the same starting point
    ref_opt.step()
    twin.step(grads, 1.0)
    _load(red, hip_params, grads, dev)
    opt.step()
    worst, bound = _worst(hip_params, ref_params), twin.bound(kind, 1.0, ref_params)
    print(f"first step after a skipped one, {kind}: max abs difference {worst:.3e}, bound {bound:.3e}")
    assert worst < bound, (worst, bound)
    # Adam's wide bound (single elements where gradient and decay cancel) would let a step taken with t = 2 through: that one is
    # 0.26 lr = 7.7e-4 away on EVERY element, so the mean difference is held to the plain bound as well
    mean = max((a.detach().cpu() - b.detach()).abs().mean().item() for a, b in zip(hip_params, ref_params))
    assert mean < BOUND, mean
    assert opt.steps_taken() == 1 and opt.steps_skipped() == 1 and not opt.last_skipped()


def test_reference_recipe_step_by_step(dev):
    """scaler.scale(loss).backward(); clip_grad_norm_ on the still-scaled gradients; scaler.step; scaler.update -- 8 steps, steps 2 and
    5 with an inf, against torch.amp.GradScaler on the CPU: scale, growth tracker and the taken / skipped counts agree after every step"""
    kw = dict(init_scale=8.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    g, ref_params, hip_params, ref_opt, red, opt = _pair(dev, "adamw", 1.0, clip_scaled=True, loss_scale="dynamic", **kw)
    scaler = torch.amp.GradScaler("cpu", **kw)
    scaler.scale(torch.ones(1))                                              # creates the scaler's scale tensor
    skipped_ref, scales = 0, []
    for step in range(1, 9):
        assert opt.get_scale() == scaler.get_scale()
        true = [torch.randn(*s, generator=g) * 0.1 for s in SHAPES]
        grads = [t * scaler.get_scale() for t in true]
        if step in (2, 5):
            grads[4][17, 5] = float("inf")
        for p, gr in zip(ref_params, grads):
            p.grad = gr.clone()
        torch.nn.utils.clip_grad_norm_(ref_params, 1.0)
        scaler.step(ref_opt)
        scaler.update()
        skipped_ref += step in (2, 5)
        _load(red, hip_params, grads, dev)
        opt.step()
        scales.append(opt.get_scale())
        assert opt.get_scale() == scaler.get_scale() and opt.growth_tracker() == scaler._get_growth_tracker(), step
        assert opt.steps_taken() == int(ref_opt.state[ref_params[0]]["step"].item()) == step - skipped_ref
        assert opt.steps_skipped() == skipped_ref and opt.last_skipped() == (step in (2, 5))
        assert _worst(hip_params, ref_params) < BOUND, step
    assert scales == [8.0, 4.0, 4.0, 4.0, 2.0, 2.0, 2.0, 4.0]               # two back-offs, one growth after three finite steps


def test_growth_leaves_a_scale_that_cannot_grow(dev):
    """2^127 * 2 is not a float32: torch's rule keeps the scale and restarts the tracker"""
    g, ref_params, hip_params, ref_opt, red, opt = _pair(dev, "adamw", None, loss_scale="dynamic", init_scale=2.0 ** 127, growth_interval=1)
    _load(red, hip_params, [torch.zeros(*s) for s in SHAPES], dev)
    opt.step()
    assert opt.get_scale() == 2.0 ** 127 and opt.growth_tracker() == 0 and opt.steps_taken() == 1


def test_state_dict_round_trip_and_fused_adamw_state(dev):
    """a fresh GuardedAdam continues from state_dict(); a FusedAdamW state dict loads with its `step` as the steps taken"""
    g, ref_params, hip_params, ref_opt, red, opt = _pair(dev, "adam", 1.0, loss_scale=4.0)
    _load(red, hip_params, [torch.randn(*s, generator=g) for s in SHAPES], dev)
    opt.step()
    sd = opt.state_dict()
    _, _, hip2, _, red2, opt2 = _pair(dev, "adam", 1.0, loss_scale="dynamic")
    opt2.load_state_dict(sd)
    assert opt2.steps_taken() == 1 and opt2.get_scale() == 4.0 and torch.equal(opt2.exp_avg[0], opt.exp_avg[0])
    opt2.load_state_dict({"step": 7, "lr": 1e-4, "exp_avg": sd["exp_avg"], "exp_avg_sq": sd["exp_avg_sq"]})
    assert opt2.steps_taken() == 7 and opt2.steps_skipped() == 0 and opt2.get_scale() == 4.0 and opt2.lr == 1e-4


# ---- TrainStep ----------------------------------------------------------------------------------------------------------------------
def _tiny(dev):
    """the model and batch of test_train_step_learns_and_refreshes_weight_copies"""
    import meant_amd
    torch.manual_seed(0)
    m = meant_amd.meant(128, 128, 4, 32, 32, 16, 3, 2, torch.nn.Embedding(100, 128), num_heads=2).to(dev).eval()
    m.compute_dtype = torch.bfloat16
    ids = torch.randint(0, 100, (8, 3, 16), device=dev)
    img = torch.randn(8, 3, 4, 32, 32, device=dev)
    mask = torch.ones(8, 3, 16, device=dev)
    tgt = torch.tensor([0, 1, 0, 1, 1, 0, 1, 0], device=dev)
    return m, ids, img, mask, tgt


def test_train_step_skips_a_poisoned_batch_and_learns_on(dev):
    """a class index outside [0, C) makes meant_ce_probs poison its gradient row with NaN: with nonfinite="skip" every parameter
    keeps its bits and the step is counted as skipped, and the clean steps that follow bring the loss down; with the default
    arguments the same batch leaves NaN parameters (the unguarded tail's behaviour, stated here as what the guard is for)"""
    from meant_amd.train import TrainStep, GuardedAdam, FusedAdamW
    m, ids, img, mask, tgt = _tiny(dev)
    bad = tgt.clone()
    bad[3] = 2
    ts = TrainStep(m, lr=2e-3, weight_decay=0.0, max_grad_norm=1.0, nonfinite="skip")
    assert isinstance(ts.opt, GuardedAdam) and ts.opt.kind == "adamw"
    before = [p.detach().clone() for p in m.parameters()]
    loss, out = ts(ids, img, mask, target=bad)
    assert torch.isnan(loss)
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))
    assert ts.opt.steps_skipped() == 1 and ts.opt.steps_taken() == 0 and ts.opt.last_skipped()
    losses = [ts(ids, img, mask, target=tgt)[0].item() for _ in range(30)]
    assert np.isfinite(losses).all() and losses[-1] < losses[0] - 0.02, losses
    assert ts.opt.steps_taken() == 30 and ts.opt.steps_skipped() == 1
    ts.reducer.close()
    m2, ids, img, mask, tgt = _tiny(dev)
    plain = TrainStep(m2, lr=2e-3, weight_decay=0.0, max_grad_norm=1.0)
    assert isinstance(plain.opt, FusedAdamW)
    plain(ids, img, mask, target=bad)
    assert any(torch.isnan(p).any().item() for p in m2.parameters())


def test_train_step_adam_with_dynamic_loss_scale(dev):
    """-o Adam under a dynamic loss scale: 10 steps, the loss stays finite and falls, and the loss returned is the unscaled one"""
    from meant_amd.train import TrainStep, cross_entropy_on_probs
    m, ids, img, mask, tgt = _tiny(dev)
    ts = TrainStep(m, lr=2e-3, weight_decay=0.0, max_grad_norm=1.0, optimizer="adam", loss_scale="dynamic")
    assert ts.opt.kind == "adam" and ts.opt.get_scale() == 65536.0
    losses = []
    for _ in range(10):
        loss, out = ts(ids, img, mask, target=tgt)
        assert abs(loss.item() - cross_entropy_on_probs(out, tgt).item()) <= 1e-6
        losses.append(loss.item())
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    assert ts.opt.steps_taken() + ts.opt.steps_skipped() == 10 and ts.opt.steps_taken() >= 8


def test_every_micro_batch_is_scaled(dev):
    """micro_batches=2 under a fixed loss scale: the unscaled gradient norm the step saw is that of the one-pass step (a micro-batch
    that missed opt.scale() would enter 1024 times too small), and the loss returned is the unscaled one"""
    from meant_amd.train import TrainStep, cross_entropy_on_probs
    norms, losses = [], []
    for k in (1, 2):
        m, ids, img, mask, tgt = _tiny(dev)
        ts = TrainStep(m, lr=1e-3, max_grad_norm=1.0, micro_batches=k, loss_scale=1024.0)
        loss, out = ts(ids, img, mask, target=tgt)
        assert abs(loss.item() - cross_entropy_on_probs(out, tgt).item()) <= 1e-6
        assert ts.opt.steps_taken() == 1 and ts.opt.get_scale() == 1024.0
        norms.append(ts.opt.last_grad_norm())
        losses.append(loss.item())
        ts.reducer.close()
    assert abs(losses[0] - losses[1]) < 2e-3                                  # the tolerances of test_train_step_micro_batches_give_the_same_update
    assert abs(norms[0] - norms[1]) <= 2e-2 * norms[0] and norms[0] > 0, norms


def test_guarded_train_step_does_not_synchronise(dev):
    """under torch's sync debug mode "error" a guarded step with a dynamic loss scale raises nothing (the control: reading the
    state block in the same mode does)"""
    from meant_amd.train import TrainStep
    m, ids, img, mask, tgt = _tiny(dev)
    ts = TrainStep(m, lr=1e-3, nonfinite="skip", loss_scale="dynamic")
    ts(ids, img, mask, target=tgt)                                           # the first step builds the rotary tables and the weight caches
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2):
            ts(ids, img, mask, target=tgt)
        with pytest.raises(RuntimeError):
            ts.opt.state.cpu()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert ts.opt.steps_taken() + ts.opt.steps_skipped() == 3


def test_route_counts_per_bucket(dev):
    from meant_amd import _lib
    g, ref_params, hip_params, ref_opt, red, opt = _pair(dev, "adamw", 1.0)
    _load(red, hip_params, [torch.randn(*s, generator=g) for s in SHAPES], dev)
    _lib.route_reset()
    opt.step()
    k = red.num_buckets
    assert k >= 2 and _lib.route_count("grad_stats") == k and _lib.route_count("optim_step") == k
