"""The hard-label losses of csrc/optim.hip under shifted, peaked, wide, masked, uniform and garbage-in-ignored-rows logits against
float64: meant_softmax_ce_fwd / meant_softmax_ce_bwd (the MLM pretrainer's loss, the source of every gradient of that run) and
meant_ce_probs (the loss of every fine-tuning step).

The entries are called at the C ABI with data_ptr(), so that ld, the padding columns, gscale and the aliasing of dlogits are the
test's own; a smaller set goes through ops.softmax_cross_entropy and ops._SoftmaxCE with autograd.  Inputs, float64 references, error
measures and gates are loss_ref's (its docstring derives every gate: 4 x the worst figure of a float32 host evaluation of the same
shift-invariant form); tests/test_loss_regimes_host.py shows on the host that these checks reject a logsumexp handed over in one
float, a missing -inf guard, a lost chunk, tail column or wave, a sum over the padding, a target off by one, ignored rows that are
not zeroed, a dropped gscale and padding that is not zeroed -- and that randn * 3 rows accept the first two.

Shapes: the smallest V at which the kernel's structure changes.  V = 1, 5 (tail only), 8 (one chunk), 12 (a tail column in a thread
with no chunk), 2047, 2048 (one pass of the 256 threads), 2049, 2056 (thread 0's second chunk), 2059, 4101.  ld = ceil8(V), and
ceil8(V) + 256 with the padding poisoned once with NaN and once with 1e30: the forward must not see it, the backward overwrites it
with zeros.  T = 1 and 5, and for `peaked` one row per peak position.  Every poisoned or out-of-range value lies inside a buffer
the test owns, and the kernels compare a target with [0, V) before they use it.  The outputs are pre-filled with NaN, so a value
that is not written is a value that is not finite.  Every case prints one `loss-regime-errors` line; tools/loss_regimes_errors.py
collects the worst per entry, regime and tier (profiles/loss_regimes_errors.txt)."""
import functools

import pytest
import torch

from tests import loss_ref as L
from tests.util import DTYPES, IDS

pytestmark = pytest.mark.gpu
SEED = 5
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _tier(dtype):
    return IDS[DTYPES.index(dtype)]


def run_entries(t, dev, dtype, alias=False, with_bwd=True):
    """meant_softmax_ce_fwd, then meant_softmax_ce_bwd (into the logits' own buffer with alias), on device copies of the case; the
    mean as the wrapper forms it.  Returns what loss_ref.check takes, plus the raw outputs."""
    from meant_amd import _lib, ops
    x = t["logits"].to(dtype).to(dev).contiguous()
    T, ld = x.shape
    tg = t["targets"].to(dev)
    row_loss = torch.full((T,), NAN, device=dev)
    lse = torch.full((T, 2), NAN, device=dev)
    g = torch.tensor([t["gscale"]], device=dev, dtype=torch.float32)
    _lib.check(_lib.lib.meant_softmax_ce_fwd(x.data_ptr(), ld, tg.data_ptr(), T, t["V"], t["ignore_index"], row_loss.data_ptr(), lse.data_ptr(),
                                             ops._dt(x), ops._stream()), "softmax_ce_fwd")
    n = L.counted(tg, t["V"], t["ignore_index"]).sum().clamp_(min=1).float()
    got = dict(row_loss=row_loss, lse=lse[:, 0].double() + lse[:, 1].double(), mean=row_loss.sum() / n, pair=lse)
    if with_bwd:
        dl = x if alias else torch.full_like(x, NAN)
        _lib.check(_lib.lib.meant_softmax_ce_bwd(x.data_ptr(), ld, tg.data_ptr(), lse.data_ptr(), T, t["V"], t["ignore_index"], g.data_ptr(),
                                                 dl.data_ptr(), ops._dt(x), ops._stream()), "softmax_ce_bwd")
        got["dlogits"] = dl
    torch.cuda.synchronize()
    return got


def _shapes(regime, V):
    """(T, ld, pad): one row on the tight stride, then the rows of the regime on the padded stride under either poison"""
    rows = len(L.peak_positions(V)) if regime == "peaked" else 5
    return [(1, L.ceil8(V), 0.0), (rows, L.ceil8(V) + 256, NAN), (rows, L.ceil8(V) + 256, 1e30)]


def _cases():
    return [(dtype, regime) for dtype in DTYPES for regime in L.regimes(_tier(dtype))]


@pytest.mark.parametrize("V", L.GATE_VS)
@pytest.mark.parametrize("dtype,regime", _cases(), ids=[f"{_tier(d)}-{r}" for d, r in _cases()])
def test_regimes_at_the_c_abi(dev, dtype, regime, V):
    """both entries against float64; a second call gives the same bits; dlogits written over the logits gives the out-of-place bits"""
    tier = _tier(dtype)
    worst = {}
    for T, ld, pad in _shapes(regime, V):
        t = L.regime_inputs(regime, T, V, ld, SEED, tier, pad=pad)
        ref = L.reference(t)
        got = run_entries(t, dev, dtype)
        fig = L.check(got, ref, t, f"{regime} V={V} ld={ld} T={T} pad={pad} {tier}")
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0.0), v)
        again = run_entries(t, dev, dtype)
        inplace = run_entries(t, dev, dtype, alias=True)
        for other in (again, inplace):
            assert torch.equal(other["row_loss"], got["row_loss"])
            cnt = ref["counted"].to(dev)
            assert torch.equal(other["pair"][cnt], got["pair"][cnt])
            assert torch.equal(other["dlogits"].view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                               got["dlogits"].view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
    L.report("softmax_ce", t, worst, gscale=f"{t['gscale']:.3g}")


@pytest.mark.parametrize("ignore_index", [-100, 0])
@pytest.mark.parametrize("V", L.GATE_VS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_kind_of_target(dev, dtype, V, ignore_index):
    """one row per target: column 0, the last chunk's last column, the first tail column, V - 1, and the rows that do not count:
    the ignore value (-100, or 0: a valid class used as the ignore value), V and ld - 1 (inside the buffer, outside the row), -1,
    2^31 + 3.  Rows that do not count: row_loss 0 and a gradient row of zeros; the others as the reference has them."""
    tier = _tier(dtype)
    for ld in (L.ceil8(V), L.ceil8(V) + 256):
        targets = [0, 8 * (V >> 3) - 1, 8 * (V >> 3), V - 1, ignore_index, V, ld - 1, -1, 2 ** 31 + 3]
        t = L.regime_inputs("plain", len(targets), V, ld, SEED, tier, ignore_index=ignore_index, pad=NAN)
        t["targets"] = torch.tensor(targets, dtype=torch.int64)
        ref = L.reference(t)
        want = [0 <= c < V and c != ignore_index for c in targets]
        assert ref["counted"].tolist() == want
        got = run_entries(t, dev, dtype)
        fig = L.check(got, ref, t, f"targets V={V} ld={ld} ignore={ignore_index} {tier}")
        dead = ~ref["counted"].to(dev)
        assert bool((got["row_loss"][dead] == 0).all()) and bool((got["dlogits"][dead] == 0).all())
    L.report("softmax_ce", dict(t, regime=f"targets_ignore{ignore_index}"), fig)


@pytest.mark.parametrize("V", [12, 2059])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gscale_is_read_from_the_device(dev, dtype, V):
    """1, 1 / 7 and -3 on the same rows: each gradient within its gate, and the forward does not depend on it"""
    tier = _tier(dtype)
    first = None
    for g in L.GSCALES:
        t = L.regime_inputs("plain", 5, V, L.ceil8(V) + 256, SEED, tier, gscale=g, pad=NAN)
        got = run_entries(t, dev, dtype)
        fig = L.check(got, L.reference(t), t, f"gscale={g} V={V} {tier}")
        first = first or got
        assert torch.equal(got["row_loss"], first["row_loss"])
        L.report("softmax_ce", dict(t, regime="gscale"), fig, gscale=f"{g:.3g}")
    assert not torch.equal(got["dlogits"], first["dlogits"])


# ------------------------------------------------------------------------------------------------------------------------------
# through ops.softmax_cross_entropy and ops._SoftmaxCE, with autograd
WRAPPER_REGIMES = ("plain", "peaked", "shifted+1000", "masked", "garbage_ignored")
UPSTREAM = -3.0                                        # d (UPSTREAM * loss): the wrapper's gscale is UPSTREAM / n


def _wrapper_case(regime, T, V, ld, tier, pad=0.0):
    t = L.regime_inputs(regime, T, V, ld, SEED, tier, pad=pad)
    n = max(1, int(L.counted(t["targets"], V, t["ignore_index"]).sum()))
    t["gscale"] = (torch.tensor(UPSTREAM, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)).item()
    return t, L.reference(t)


def _through(fn, x, t, ref, what):
    """loss = fn(x); (UPSTREAM * loss).backward(); the mean and the gradient of the [T, ld] buffer through check"""
    x.requires_grad_(True)
    loss = fn(x)
    (loss * UPSTREAM).backward()
    torch.cuda.synchronize()
    assert loss.dim() == 0 and loss.dtype == torch.float32
    grad = x.grad.reshape(-1, x.shape[-1])
    grad = torch.nn.functional.pad(grad, (0, t["ld"] - grad.shape[-1]))
    return L.check(dict(mean=loss.detach(), dlogits=grad), ref, t, what)


@pytest.mark.parametrize("form", ["off_grid", "strided", "batched", "padded_buffer"])
@pytest.mark.parametrize("regime", WRAPPER_REGIMES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_wrapper_forms(dev, dtype, regime, form):
    """off_grid: V = 2059, contiguous, re-homed by the wrapper's padding route.  strided: V = 2056 as a column slice of a wider
    poisoned block.  batched: logits [2, 3, V] with targets [2, 3].  padded_buffer: ops._SoftmaxCE on [T, ld = ceil8(V) + 256] with
    NaN in the padding, as the vocabulary GEMM hands it over.  The mean is over the rows that count: each case holds some that do not."""
    from meant_amd import ops
    tier = _tier(dtype)
    V = 2056 if form == "strided" else 2059
    T = 6 if form == "batched" else 5
    ld = L.ceil8(V) + 256 if form == "padded_buffer" else L.ceil8(V)
    t, ref = _wrapper_case(regime, T, V, ld, tier, pad=NAN)
    assert 0 < int(ref["counted"].sum()) < T
    tg = t["targets"].to(dev)
    if form == "padded_buffer":
        x = t["logits"].to(dtype).to(dev)
        fig = _through(lambda v: ops._SoftmaxCE.apply(v, tg, V, t["ignore_index"]), x, t, ref, f"{form} {regime} {tier}")
        assert bool((x.grad[:, V:] == 0).all())
    elif form == "strided":
        block = torch.full((T, V + 24), NAN, device=dev, dtype=dtype)
        block[:, 8:8 + V] = t["logits"][:, :V].to(dtype).to(dev)
        block.requires_grad_(True)
        view = block[:, 8:8 + V]
        assert not view.is_contiguous()
        loss = ops.softmax_cross_entropy(view, tg)
        (loss * UPSTREAM).backward()
        g = block.grad
        assert bool((g[:, :8] == 0).all()) and bool((g[:, 8 + V:] == 0).all())
        fig = L.check(dict(mean=loss.detach(), dlogits=g[:, 8:8 + V]), ref, t, f"{form} {regime} {tier}")
    else:
        x = t["logits"][:, :V].to(dtype).to(dev).contiguous()
        if form == "batched":
            x, tg = x.view(2, 3, V), tg.view(2, 3)
        fig = _through(lambda v: ops.softmax_cross_entropy(v, tg), x, t, ref, f"{form} {regime} {tier}")
    L.report("wrapper_" + form, t, fig)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_wrapper_with_every_row_ignored(dev, dtype):
    """pinned: a batch in which no row counts gives loss 0 and a gradient of zeros (the mean divides by max(1, rows that count)),
    where torch.nn.functional.cross_entropy returns NaN (0 / 0).  A pretraining step whose micro-batch drew no label then adds
    nothing instead of poisoning the parameters."""
    from meant_amd import ops
    V = 2059
    x = torch.randn(4, V, generator=torch.Generator().manual_seed(SEED)).to(dtype)
    tg = torch.tensor([-100, -100, V, -1])
    assert bool(torch.isnan(torch.nn.functional.cross_entropy(x.float(), torch.full((4,), -100))))
    xd = x.to(dev).requires_grad_(True)
    loss = ops.softmax_cross_entropy(xd, tg.to(dev))
    loss.backward()
    assert loss.item() == 0.0 and bool((xd.grad == 0).all())


# ------------------------------------------------------------------------------------------------------------------------------
# meant_ce_probs
def _ce_probs(p, tg, dev, preload=0.0, with_grad=True):
    from meant_amd import _lib, ops
    B, C = p.shape
    pd, td = p.to(dev).contiguous(), tg.to(dev)
    loss = torch.full((1,), preload, device=dev, dtype=torch.float32)
    dp = torch.full((B, C), NAN, device=dev) if with_grad else None
    _lib.check(_lib.lib.meant_ce_probs(pd.data_ptr(), td.data_ptr(), loss.data_ptr(), ops._p(dp), B, C, ops._stream()), "ce_probs")
    torch.cuda.synchronize()
    return loss[0].cpu(), dp


@pytest.mark.parametrize("kind", L.CE_PROBS_KINDS)
@pytest.mark.parametrize("B,C", L.CE_PROBS_SHAPES, ids=[f"{b}x{c}" for b, c in L.CE_PROBS_SHAPES])
def test_ce_probs_against_float64(dev, B, C, kind):
    """rand rows and rows of exact 0 and 1 within the gates of loss_ref.  rand + 1000 lies outside the entry's contract of
    probabilities, and the kernel keeps logsumexp = max + log sum in ONE float there (unlike meant_softmax_ce_fwd): near 1008 that
    float has an ulp of 2^-14, so loss and dprobs * B may be off by half of it, 2^-15 = 3.05e-5, on top of the gate (x - lse itself is
    exact: both are multiples of 2^-14 below 2^10).  Measured on an MI355X at this shift: loss 2.5e-5, dprobs * B 2.1e-5, 3.7 x and
    49 x the gates of the shift-invariant form, so the case is held to the one-float bound and not to those gates; the kernel was left
    as it is because the other form moves every gradient of a fine-tuning step by an ulp.
    The entry ADDS to loss_accum: a pre-loaded 1.5 comes back as 1.5 + loss to the rounding of that sum and of the adds of the
    ceil(B / 64) waves; without dprobs the loss is the same."""
    p, tg = L.ce_probs_inputs(kind, B, C, SEED)
    ref_loss, ref_d = L.ce_probs_reference(p, tg)
    loss, dp = _ce_probs(p, tg, dev)
    gates = {k: v + 2.0 ** -15 for k, v in L.CE_PROBS_GATES.items()} if kind == "shifted" else None
    fig = L.ce_probs_check(loss, dp, ref_loss, ref_d, f"ce_probs {kind} [{B}, {C}]", gates)
    loss_only, none = _ce_probs(p, tg, dev, with_grad=False)
    assert none is None
    L.ce_probs_check(loss_only, None, ref_loss, ref_d, f"ce_probs {kind} [{B}, {C}] without dprobs", gates)
    added, _ = _ce_probs(p, tg, dev, preload=1.5, with_grad=False)
    waves = -(-B // 64)
    assert abs(added.double().item() - (1.5 + loss.double().item())) <= (1 + waves) * 2.0 ** -24 * (1.5 + abs(loss.item()))
    print(f"loss-regime-errors entry=ce_probs regime={kind} tier=f32 V={C} B={B} " + " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
