"""Hard-label cross-entropy with class weights, label smoothing and ignore_index on the device (csrc/ce_hard.hip: meant_ce_probs_hard,
meant_softmax_ce_hard_fwd / _bwd, meant_ce_hard_reduce, and the wrappers around them) against float64 on the CPU: the reference,
the cases and the gates are those of tests/ce_hard_ref.py, whose reference test_ce_hard_host.py holds against F.cross_entropy."""
import functools

import numpy as np
import pytest
import torch

from tests import ce_hard_ref as R
from tests import loss_ref

pytestmark = pytest.mark.gpu
NAN = float("nan")
HARD_ROUTES = ("ce_hard_wave", "ce_hard_block", "ce_hard_vocab")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def run_probs(p, y, w, eps, dev, ignore_index=R.IGNORE, with_grad=True):
    """one meant_ce_probs_hard call on device copies into poisoned buffers: row_loss, row_w, grad_rows (dprobs as the entry leaves
    it), loss and gscale (0-dim device views of the block), stats (the block read back), routes"""
    from meant_amd import _lib, ops
    B, C = p.shape
    p, y = p.to(dev).contiguous(), y.to(dev)
    w = None if w is None else w.to(dev)
    rows, roww = torch.full((B,), NAN, device=dev), torch.full((B,), NAN, device=dev)
    blk = torch.full((ops.CE_STATS_FLOATS,), NAN, device=dev)
    dp = torch.full((B, C), NAN, device=dev) if with_grad else None
    _lib.route_reset()
    _lib.check(_lib.lib.meant_ce_probs_hard(p.data_ptr(), C, y.data_ptr(), _ptr(w), eps, ignore_index, rows.data_ptr(), roww.data_ptr(),
                                            _ptr(dp), C, B, C, blk.data_ptr(), _stream()), "ce_probs_hard")
    out = dict(row_loss=rows, row_w=roww, loss=blk[0], gscale=blk[1], stats=ops.ce_stats(blk),
               routes=tuple(_lib.route_count(r) for r in HARD_ROUTES))
    if with_grad:
        out["grad_rows"] = dp
    return out


def run_vocab(logits, y, w, eps, V, gscale, dev, ignore_index=R.IGNORE, in_place=True):
    """the forward / backward pair on a device copy of logits [T, ld] (its dtype is the tier), the backward in place: row_loss,
    row_w, dlogits [T, ld], loss, gscale of the block, stats"""
    from meant_amd import _lib, ops
    T, ld = logits.shape
    x, y = logits.to(dev).contiguous(), y.to(dev)
    w = None if w is None else w.to(dev)
    rows, roww = torch.full((T,), NAN, device=dev), torch.full((T,), NAN, device=dev)
    stat = torch.full((T, 4), NAN, device=dev)
    blk = torch.full((ops.CE_STATS_FLOATS,), NAN, device=dev)
    g = torch.tensor([gscale], device=dev, dtype=torch.float32)
    _lib.route_reset()
    _lib.check(_lib.lib.meant_softmax_ce_hard_fwd(x.data_ptr(), ld, y.data_ptr(), _ptr(w), eps, T, V, ignore_index, rows.data_ptr(),
                                                  roww.data_ptr(), stat.data_ptr(), blk.data_ptr(), ops._dt(x), _stream()), "softmax_ce_hard_fwd")
    routes = tuple(_lib.route_count(r) for r in HARD_ROUTES)
    dl = x if in_place else torch.full_like(x, NAN)
    _lib.check(_lib.lib.meant_softmax_ce_hard_bwd(x.data_ptr(), ld, y.data_ptr(), _ptr(w), eps, stat.data_ptr(), T, V, ignore_index,
                                                  g.data_ptr(), dl.data_ptr(), ops._dt(x), _stream()), "softmax_ce_hard_bwd")
    return dict(row_loss=rows, row_w=roww, dlogits=dl, loss=blk[0], gscale=blk[1], stats=ops.ce_stats(blk), routes=routes)


def _counts(stats):
    return stats.n_counted, stats.n_ignored, stats.n_invalid


def _ref_counts(ref):
    return ref["n_counted"], ref["n_ignored"], ref["n_invalid"]


@functools.lru_cache(maxsize=None)
def probs_case(B, C, kind, eps, wk):
    """inputs and the float64 reference of one class-head case, computed once and shared (never written to)"""
    p, y = R.probs_inputs(B, C, kind)
    w = R.make_weight(wk, C, B)
    return p, y, w, R.reference(p, y, w, eps)


# ---- the class head's form -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.PROBS_KINDS)
@pytest.mark.parametrize("B,C", R.PROBS_SHAPES, ids=[f"{b}x{c}" for b, c in R.PROBS_SHAPES])
def test_class_head_against_float64(dev, B, C, kind):
    from meant_amd.train import cross_entropy_on_probs
    for eps, wk in R.PROBS_OPTS:
        p, y, w, ref = probs_case(B, C, kind, eps, wk)
        got = run_probs(p, y, w, eps, dev)
        assert got["routes"] == ((1, 0, 0) if C <= R.CUT_WAVE else (0, 1, 0)), got["routes"]     # the form this shape is meant to test
        fig = R.errors(got, ref)
        print(f"[{B}, {C}] {kind} eps={eps} w={wk}: loss {got['loss'].item():.9g} ref {float(ref['loss']):.9g} " +
              " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
        R.check(got, ref, "probs", f"[{B}, {C}] {kind} eps={eps} w={wk}")
        st = got["stats"]
        assert _counts(st) == _ref_counts(ref)
        assert abs(st.num - float(ref["num"])) <= R.GATES["probs"]["row_loss"] * float(ref["row_loss"].abs().clamp(min=1.0).sum())
        assert abs(st.den - float(ref["den"])) <= 1e-12 * max(1.0, float(ref["den"]))     # float32 weights added in double, in another order
        # the public route: the same bits forward, the entry's gradient times the block's 1 / den backward
        pg = p.to(dev).requires_grad_(True)
        loss = cross_entropy_on_probs(pg, y.to(dev), weight=None if w is None else w.to(dev), label_smoothing=eps, ignore_index=R.IGNORE)
        (loss * 3.0).backward()
        assert loss.dim() == 0 and torch.equal(loss.detach(), got["loss"])
        assert torch.equal(pg.grad, got["grad_rows"] * (torch.tensor(3.0, device=dev) * got["gscale"]))
        if float(ref["den"]) != 0:
            gerr = (pg.grad.double().cpu() / 3.0 - ref["grad"]).abs().max().item() * float(ref["den"])
            # three more float32 roundings on the way: 1 / den, its product with d loss, the product with the gradient row
            assert gerr <= R.GATES["probs"]["grad"] + 3 * 2.0 ** -24 * float(ref["grad_rows"].abs().max()), gerr
    p, y, w, ref = probs_case(B, C, kind, *R.PROBS_OPTS[0])
    lean = run_probs(p, y, w, R.PROBS_OPTS[0][0], dev, with_grad=False)                          # dprobs is optional
    full = run_probs(p, y, w, R.PROBS_OPTS[0][0], dev)
    assert torch.equal(lean["row_loss"], full["row_loss"]) and torch.equal(lean["loss"], full["loss"])


def test_class_head_reads_rows_in_place(dev):
    """probs as a column slice of a wider, poisoned block: not a bit differs from the contiguous call"""
    from meant_amd.train import cross_entropy_on_probs
    for B, C, ldp in ((5, 7, 9), (130, 3129, 3131), (2, 4097, 4100)):
        p, y, w, _ = probs_case(B, C, "randn8", 0.1, "zeros")
        kw = dict(weight=w.to(dev), label_smoothing=0.1, ignore_index=R.IGNORE)
        pc = p.to(dev).requires_grad_(True)
        want = cross_entropy_on_probs(pc, y.to(dev), **kw)
        want.backward()
        block = torch.full((B + 1, ldp), NAN, device=dev)
        block[:B, :C] = p.to(dev)
        block.requires_grad_(True)
        got = cross_entropy_on_probs(block[:B, :C], y.to(dev), **kw)
        got.backward()
        assert torch.equal(got.detach(), want.detach()) and torch.equal(block.grad[:B, :C], pc.grad)
        assert block.grad[B].abs().sum().item() == 0 and block.grad[:, C:].abs().sum().item() == 0


# ---- the large-vocabulary form ---------------------------------------------------------------------------------------------------
def _tier_dtype(tier):
    return torch.bfloat16 if tier == "bf16" else torch.float32


@pytest.mark.parametrize("tier,regime", [(t, r) for t in ("f32", "bf16") for r in loss_ref.regimes(t)])
def test_vocab_form_against_float64(dev, tier, regime):
    worst = {}
    for V in loss_ref.GATE_VS:
        t = loss_ref.regime_inputs(regime, R.VOCAB_T, V, loss_ref.ceil8(V) + 256, 0, tier, pad=NAN)      # the padding is never read
        x, y, g = t["logits"][:, :V], t["targets"], t["gscale"]
        for eps, wk in R.vocab_opts(regime):
            w = R.make_weight(wk, V, V)
            ref = R.reference(x, y, w, eps, t["ignore_index"])
            got = run_vocab(t["logits"].to(_tier_dtype(tier)), y, w, eps, V, g, dev, t["ignore_index"])
            assert got["routes"] == (0, 0, 1)
            got["grad_rows"] = got["dlogits"].double().cpu() / g                 # the measure divides by gscale
            fig = R.check(got, ref, tier, f"{regime} {tier} V={V} eps={eps} w={wk}", bf16_grad=tier == "bf16")
            assert _counts(got["stats"]) == _ref_counts(ref)
            for k, v in fig.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print(f"{regime} {tier}: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()))


def test_vocab_form_bf16_at_the_vocabulary_size(dev):
    T, V = 3, 64001
    ld = loss_ref.ceil8(V) + 256
    g = torch.Generator().manual_seed(11)
    logits = torch.full((T, ld), NAN)
    logits[:, :V] = (torch.randn(T, V, generator=g) * 3).bfloat16().float()
    y = torch.tensor([V - 1, R.IGNORE, 8 * (V >> 3)])
    w = R.make_weight("rand", V, 1)
    for eps in (0.0, 0.1):
        ref = R.reference(logits[:, :V], y, w, eps)
        got = run_vocab(logits.bfloat16(), y, w, eps, V, 0.5, dev)
        got["grad_rows"] = got["dlogits"].double().cpu() / 0.5
        fig = R.check(got, ref, "bf16", f"[3, 64001] bf16 eps={eps}", bf16_grad=True)
        print(f"[3, 64001] bf16 eps={eps}: " + " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
        assert _counts(got["stats"]) == (2, 1, 0)


def test_wrapper_matches_the_entries_and_float64(dev):
    """ops.softmax_cross_entropy(weight=, label_smoothing=) on rows that need re-homing (V % 8 != 0): float64 within the gates"""
    from meant_amd import _lib, ops
    T, V = 7, 2059
    g = torch.Generator().manual_seed(2)
    x = torch.randn(T, V, generator=g) * 3
    y = torch.randint(0, V, (T,), generator=g)
    y[2], y[5] = R.IGNORE, V
    w = R.make_weight("zeros", V, 3)
    ref = R.reference(x, y, w, 0.1)
    xg = x.to(dev).requires_grad_(True)
    _lib.route_reset()
    loss = ops.softmax_cross_entropy(xg, y.to(dev), weight=w.to(dev), label_smoothing=0.1)
    loss.backward()
    assert _lib.route_count("ce_hard_vocab") == 1 and _lib.route_count("softmax_ce") == 0
    assert abs(loss.item() - float(ref["loss"])) <= R.GATES["f32"]["loss"] * max(1.0, abs(float(ref["loss"])))
    gerr = (xg.grad.double().cpu() - ref["grad"]).abs().max().item() * float(ref["den"])
    assert gerr <= R.GATES["f32"]["grad"] + 3 * 2.0 ** -24 * float(ref["grad_rows"].abs().max()), gerr      # 1 / den and two products
    assert xg.grad[2].abs().sum().item() == 0 and xg.grad[5].abs().sum().item() == 0


# ---- properties ------------------------------------------------------------------------------------------------------------------
def test_repeated_calls_give_the_same_bits(dev):
    from meant_amd import _lib
    saved = _lib.get_option("deterministic")
    p, y, w, _ = probs_case(130, 3129, "probs", 0.1, "zeros")
    t = R.vocab_case("plain", 4101, "f32")
    wv = R.make_weight("rand", 4101, 1)
    try:
        runs = []
        for i in range(4):
            _lib.set_option("deterministic", i % 2)
            a = run_probs(p, y, w, 0.1, dev)
            b = run_vocab(t["logits"], t["targets"], wv, 0.1, 4101, 0.25, dev)
            runs.append((a["loss"].clone(), a["row_loss"].clone(), a["grad_rows"].clone(), b["loss"].clone(), b["row_loss"].clone(), b["dlogits"].clone()))
    finally:
        _lib.set_option("deterministic", saved)
    for r in runs[1:]:
        assert all(torch.equal(u, v) for u, v in zip(r, runs[0]))


@pytest.mark.parametrize("B,C", [(7, 257), (130, 3129), (9, 64001)])
def test_garbage_rows_that_do_not_count_leave_zeros(dev, B, C):
    p, y, w, ref = probs_case(B, C, "probs", 0.1, "rand")
    clean = run_probs(p, y, w, 0.1, dev)
    dirty = p.clone()
    junk = torch.tensor([NAN, float("inf"), 3e38, float("-inf"), -3e38])
    dead = (~ref["counted"]).nonzero()[:, 0]
    assert len(dead) == 2
    for k, r in enumerate(dead.tolist()):
        dirty[r] = junk[(torch.arange(C) + k) % 5]
    got = run_probs(dirty, y, w, 0.1, dev)
    for name in ("row_loss", "row_w", "grad_rows", "loss"):
        assert torch.equal(got[name], clean[name]), name
    assert got["row_loss"][dead].abs().sum().item() == 0 and got["row_w"][dead].abs().sum().item() == 0
    assert got["grad_rows"][dead].abs().sum().item() == 0


@pytest.mark.parametrize("bad", [None, -1, 2 ** 31 + 3], ids=["C", "-1", "2^31+3"])
def test_invalid_targets_are_counted_and_poison_nothing(dev, bad):
    from meant_amd import ops
    from meant_amd.train import cross_entropy_on_probs
    B, C = 12, 300
    g = torch.Generator().manual_seed(5)
    p = torch.rand(B, C, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    w = R.make_weight("rand", C, 2)
    keep = torch.ones(B, dtype=torch.bool)
    keep[[1, 7, 8]] = False
    yb = y.clone()
    yb[~keep] = C if bad is None else bad
    got = run_probs(p, yb, w, 0.1, dev, ignore_index=ops.IGNORE_NONE)
    sub = run_probs(p[keep], y[keep], w, 0.1, dev, ignore_index=ops.IGNORE_NONE)
    assert _counts(got["stats"]) == (B - 3, 0, 3) and _counts(sub["stats"]) == (B - 3, 0, 0)
    assert bool(torch.isfinite(got["loss"])) and bool(torch.isfinite(got["grad_rows"]).all())
    assert torch.equal(got["row_loss"][keep.to(dev)], sub["row_loss"]) and torch.equal(got["grad_rows"][keep.to(dev)], sub["grad_rows"])
    assert got["grad_rows"][(~keep).to(dev)].abs().sum().item() == 0
    assert abs(got["loss"].item() - sub["loss"].item()) <= 1e-6          # the same rows, added in another order
    pg = p.to(dev).requires_grad_(True)                                  # ignore_index=None through the wrapper: the same route
    loss = cross_entropy_on_probs(pg, yb.to(dev), weight=w.to(dev), label_smoothing=0.1)
    assert torch.equal(loss.detach(), got["loss"])
    x = torch.full((B, 512), NAN)
    x[:, :C] = p
    v = run_vocab(x, yb, w, 0.1, C, 1.0, dev)
    assert _counts(v["stats"]) == (B - 3, 0, 3) and bool(torch.isfinite(v["dlogits"]).all())


def test_all_rows_ignored_gives_zero_loss_and_zero_gradients(dev):
    from meant_amd import ops
    from meant_amd.train import cross_entropy_on_probs
    B, C = 6, 1500
    p = torch.full((B, C), NAN, device=dev).requires_grad_(True)         # never read
    y = torch.full((B,), -100, device=dev)
    w = R.make_weight("rand", C, 1).to(dev)
    loss = cross_entropy_on_probs(p, y, weight=w, label_smoothing=0.1, ignore_index=-100)
    loss.backward()
    assert loss.item() == 0.0 and p.grad.abs().sum().item() == 0.0
    x = torch.full((B, C), NAN, device=dev).requires_grad_(True)
    loss = ops.softmax_cross_entropy(x, y, weight=w, label_smoothing=0.1)
    loss.backward()
    assert loss.item() == 0.0 and x.grad.abs().sum().item() == 0.0


def test_zero_weight_class_has_a_zero_gradient_row_at_eps_zero(dev):
    for C in (9, 3129, 5000):
        p, y = torch.rand(4, C), torch.tensor([0, 3, 0, 5])
        w = R.make_weight("rand", C, 1)
        w[0] = 0.0
        got = run_probs(p, y, w, 0.0, dev, ignore_index=-100)
        v = run_vocab(torch.nn.functional.pad(p, (0, loss_ref.ceil8(C) - C)), y, w, 0.0, C, 1.0, dev)
        for g in (got["grad_rows"], v["dlogits"]):
            assert g[0].abs().sum().item() == 0 and g[2].abs().sum().item() == 0 and g[1].abs().sum().item() > 0
        assert got["row_loss"][0].item() == 0 and got["row_w"][0].item() == 0 and got["stats"].n_counted == 4


# ---- the reduction alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 255, 256, 257, 70001])
def test_reduction_is_exact_on_integers(dev, T):
    from meant_amd import _lib, ops
    rs = np.random.RandomState(T)
    C = 10
    rows = rs.randint(0, 1000, size=T).astype(np.float32)
    roww = rs.randint(0, 8, size=T).astype(np.float32)
    y = rs.randint(0, C, size=T).astype(np.int64)
    kind = rs.randint(0, 4, size=T) if T > 1 else np.zeros(1, dtype=np.int64)    # 0, 1: counts; 2: ignored; 3: invalid
    y[kind == 2] = -100
    y[kind == 3] = rs.choice(np.array([C, -1, 2 ** 31 + 3], np.int64), size=int((kind == 3).sum()))
    live = kind < 2
    rows_d, roww_d = rows.copy(), roww.copy()
    rows_d[~live], roww_d[~live] = NAN, NAN                              # the rows that do not count are not read
    for scale in (1.0, 0.0):                                             # the second pass: weights of zero, the denominator is 0
        blk = torch.full((ops.CE_STATS_FLOATS,), NAN, device=dev)
        rd, wd, yd = (torch.from_numpy(a).to(dev) for a in (rows_d, roww_d * np.float32(scale), y))
        _lib.check(_lib.lib.meant_ce_hard_reduce(rd.data_ptr(), wd.data_ptr(), yd.data_ptr(), T, C, -100, blk.data_ptr(), _stream()),
                   "ce_hard_reduce")
        st = ops.ce_stats(blk)
        num, den = float(rows[live].astype(np.float64).sum()), float(roww[live].astype(np.float64).sum()) * scale
        assert st.num == num and st.den == den
        assert _counts(st) == (int(live.sum()), int((kind == 2).sum()), int((kind == 3).sum()))
        if den:
            assert st.loss == float(np.float32(num / den)) and st.gscale == float(np.float32(1.0 / den))
        else:
            assert st.loss == 0.0 and st.gscale == 0.0


def test_argument_checks_at_the_c_abi(dev):
    from meant_amd import _lib, ops
    lib = _lib.lib
    B, C = 4, 16
    p, d = torch.rand(B, C, device=dev), torch.empty(B, C, device=dev)
    y = torch.zeros(B, dtype=torch.int64, device=dev)
    rows, roww, stat = torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(B, 4, device=dev)
    blk = torch.empty(ops.CE_STATS_FLOATS + 1, device=dev)
    w = torch.ones(C + 4, device=dev)
    g = torch.ones(1, device=dev)
    P, D, Y, RL, RW, ST, BK, W, G = (t.data_ptr() for t in (p, d, y, rows, roww, stat, blk, w, g))
    s = _stream()

    def probs(**kw):
        a = dict(probs=P, ldp=C, target=Y, weight=W, eps=0.1, ign=-100, rl=RL, rw=RW, dp=D, ldd=C, B=B, C=C, blk=BK)
        a.update(kw)
        return lib.meant_ce_probs_hard(a["probs"], a["ldp"], a["target"], a["weight"], a["eps"], a["ign"], a["rl"], a["rw"], a["dp"], a["ldd"],
                                       a["B"], a["C"], a["blk"], s)

    def fwd(**kw):
        a = dict(x=P, ld=C, target=Y, weight=W, eps=0.1, T=B, V=C, rl=RL, rw=RW, st=ST, blk=BK, dt=_lib.F32)
        a.update(kw)
        return lib.meant_softmax_ce_hard_fwd(a["x"], a["ld"], a["target"], a["weight"], a["eps"], a["T"], a["V"], -100, a["rl"], a["rw"], a["st"],
                                             a["blk"], a["dt"], s)

    def bwd(**kw):
        a = dict(x=P, ld=C, target=Y, weight=W, eps=0.1, st=ST, T=B, V=C, g=G, dl=D, dt=_lib.F32)
        a.update(kw)
        return lib.meant_softmax_ce_hard_bwd(a["x"], a["ld"], a["target"], a["weight"], a["eps"], a["st"], a["T"], a["V"], -100, a["g"], a["dl"],
                                             a["dt"], s)

    assert probs() == _lib.OK and fwd() == _lib.OK and bwd() == _lib.OK and bwd(dl=P) == _lib.OK       # the backward may run in place
    bad_eps = [dict(eps=-0.1), dict(eps=1.5), dict(eps=NAN), dict(eps=float("inf"))]
    for kw in bad_eps + [dict(probs=None), dict(target=None), dict(rl=None), dict(rw=None), dict(blk=None), dict(ldp=C - 1), dict(ldd=C - 1),
                         dict(B=0), dict(C=0), dict(dp=P), dict(rw=RL), dict(probs=P + 2), dict(weight=W + 2), dict(blk=BK + 4)]:
        assert probs(**kw) == _lib.ERR_ARG, kw
    for kw in bad_eps + [dict(x=None), dict(st=None), dict(blk=None), dict(ld=C + 4), dict(V=C + 8), dict(V=0), dict(T=-1), dict(dt=7),
                         dict(x=P + 4), dict(weight=W + 4), dict(st=ST + 4), dict(rw=RL)]:
        assert fwd(**kw) == _lib.ERR_ARG, kw
    for kw in bad_eps + [dict(x=None), dict(st=None), dict(g=None), dict(dl=None), dict(ld=C + 4), dict(V=0), dict(dt=7), dict(dl=D + 4),
                         dict(weight=W + 4)]:
        assert bwd(**kw) == _lib.ERR_ARG, kw
    assert fwd(T=2 ** 31) == _lib.ERR_UNSUPPORTED and bwd(T=2 ** 31) == _lib.ERR_UNSUPPORTED
    assert probs(B=2 ** 31, C=2000, ldp=2000, ldd=2000) == _lib.ERR_UNSUPPORTED and probs(C=2 ** 31 - 8, ldp=2 ** 31, ldd=2 ** 31) == _lib.ERR_UNSUPPORTED
    assert lib.meant_ce_hard_reduce(RL, RW, Y, B, C, -100, None, s) == _lib.ERR_ARG
    assert lib.meant_ce_hard_reduce(RL, RW, Y, -1, C, -100, BK, s) == _lib.ERR_ARG
    assert lib.meant_ce_hard_reduce(RL, RW, Y, B, C, -100, BK + 4, s) == _lib.ERR_ARG


# ---- unchanged defaults ----------------------------------------------------------------------------------------------------------
def test_defaults_keep_their_routes_and_bits(dev):
    from meant_amd import _lib, ops
    from meant_amd.train import cross_entropy_on_probs
    g = torch.Generator().manual_seed(9)
    p, t = torch.rand(33, 17, generator=g).to(dev), torch.randint(0, 17, (33,), generator=g).to(dev)
    res = []
    for kw in ({}, dict(weight=None, label_smoothing=0.0, ignore_index=None)):
        pg = p.clone().requires_grad_(True)
        _lib.route_reset()
        loss = cross_entropy_on_probs(pg, t, **kw)
        loss.backward()
        assert _lib.route_count("ce_probs") == 1 and sum(_lib.route_count(r) for r in HARD_ROUTES) == 0
        res.append((loss.detach(), pg.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    x, tv = (torch.randn(21, 2059, generator=g) * 3).to(dev), torch.randint(0, 2059, (21,), generator=g).to(dev)
    tv[4] = -100
    res = []
    for kw in ({}, dict(weight=None, label_smoothing=0.0)):
        xg = x.clone().requires_grad_(True)
        _lib.route_reset()
        loss = ops.softmax_cross_entropy(xg, tv, **kw)
        loss.backward()
        assert _lib.route_count("softmax_ce") == 1 and sum(_lib.route_count(r) for r in HARD_ROUTES) == 0
        res.append((loss.detach(), xg.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# ---- through the modules ---------------------------------------------------------------------------------------------------------
def _tiny_vision(dev):
    import meant_amd
    torch.manual_seed(0)
    m = meant_amd.meant_vision(128, 4, 32, 32, 16, 3, 3, num_heads=2, num_encoders=1, channels=4).to(dev).eval()
    m.compute_dtype = torch.bfloat16
    rs = np.random.RandomState(4)
    img = torch.from_numpy(rs.standard_normal((8, 3, 4, 32, 32)).astype("float32")).to(dev)
    return m, img, torch.tensor([0, 1, 2, -100, 1, 0, 2, 2], device=dev)


@pytest.mark.parametrize("k", [1, 2])
def test_train_step_with_class_weights_and_smoothing(dev, k):
    from meant_amd import _lib
    from meant_amd.train import TrainStep, cross_entropy_on_probs
    m, img, tgt = _tiny_vision(dev)
    w = [0.5, 2.0, 1.25]
    ts = TrainStep(m, lr=1e-3, micro_batches=k, class_weight=w, label_smoothing=0.1, ignore_index=-100)
    assert ts.class_weight.dtype == torch.float32 and ts.class_weight.device == img.device
    before = [q.detach().clone() for q in m.parameters()]
    _lib.route_reset()
    loss, out = ts(img, target=tgt)
    assert _lib.route_count("ce_hard_wave") == k and _lib.route_count("ce_probs") == 0
    kw = dict(weight=ts.class_weight, label_smoothing=0.1, ignore_index=-100)
    if k == 1:
        assert torch.equal(loss, cross_entropy_on_probs(out, tgt, **kw))
    else:                                                # each micro-batch by its own denominator, times 1 / k
        halves = [cross_entropy_on_probs(out[i * 4:(i + 1) * 4], tgt[i * 4:(i + 1) * 4], **kw) * (1.0 / 2) for i in range(2)]
        assert torch.equal(loss, 0.0 + halves[0] + halves[1])
    ref = R.reference(out.cpu(), tgt.cpu(), torch.tensor(w), 0.1)
    if k == 1:
        assert abs(loss.item() - float(ref["loss"])) <= R.GATES["probs"]["loss"] * max(1.0, float(ref["loss"]))
    assert bool(torch.isfinite(loss)) and any(not torch.equal(a, q.detach()) for a, q in zip(before, m.parameters()))
    ts.reducer.close()


class _StandInHead(torch.nn.Module):
    """the three attributes of a RobertaLMHead, decoder tied to the word embedding (pretrain_mlm.py:318-319)"""

    def __init__(self, emb, d, V):
        super().__init__()
        self.dense = torch.nn.Linear(d, d)
        self.layer_norm = torch.nn.LayerNorm(d, eps=1e-5)
        self.decoder = torch.nn.Linear(d, V)
        self.decoder.weight = emb.weight


@pytest.mark.parametrize("only", [False, True], ids=["all_rows", "labelled_rows"])
def test_mlm_pretrainer_loss_with_smoothing(dev, only):
    """loss(label_smoothing=0.1, class_weight=) of a tiny float32 pretrainer against the float64 loss of its own logits, and the
    decoder bias gradient -- the column sums of d loss / d logits -- against float64 too.  Bounds: the logits the two calls see
    come from the same kernels but, on the labelled rows, from a GEMM over other row tiles, so the loss is held to the 1e-5 that
    test_gpu_mlm_labelled.py allows between the two routes in this tier, the bias gradient to 1e-5 of its largest entry"""
    import meant_amd as M
    torch.manual_seed(3)
    d, V = 128, 120
    emb = torch.nn.Embedding(V, d)
    m = M.meant_language_pretrainer(1, d, emb, _StandInHead(emb, d, V), text_dim=d, num_heads=2).to(dev).eval()
    m.compute_dtype = torch.float32
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, V, (3, 24), generator=g)
    mask = torch.ones(3, 24)
    mask[1, 20:] = 0
    labels = torch.full((3, 24), -100, dtype=torch.int64)
    pick = torch.rand(3, 24, generator=g) < 0.15
    labels[pick] = ids[pick]
    w = R.make_weight("rand", V, 5)
    with torch.no_grad():
        logits = m(ids.to(dev), mask.to(dev)).float().cpu().reshape(-1, V)
    ref = R.reference(logits, labels.reshape(-1), w, 0.1)
    assert ref["n_counted"] == int(pick.sum()) > 0
    loss = m.loss(ids.to(dev), mask.to(dev), labels.to(dev), labelled_only=only, label_smoothing=0.1, class_weight=w.to(dev))
    assert m.last_head_rows == ((ref["n_counted"] + 7) // 8 * 8 if only else 72)
    loss.backward()
    assert abs(loss.item() - float(ref["loss"])) <= 1e-5 * max(1.0, float(ref["loss"])), (loss.item(), float(ref["loss"]))
    db = m.mlm_head.decoder.bias.grad.double().cpu()
    want = ref["grad"].sum(0)
    assert (db - want).abs().max().item() <= 1e-5 * want.abs().max().item()
