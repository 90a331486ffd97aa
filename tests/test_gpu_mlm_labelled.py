"""The MLM vocabulary head on the labelled rows alone (utils/custom_datasets.py:46-54 labels 15 % of the positions; pretrain_mlm.py:160,178
ignores the rest): meant_select_rows at the C ABI against numpy, the differentiable row gather, the loss on the gathered rows against
F.cross_entropy and against the all-rows route, and the pretrainer's loss() on both routes."""
import numpy as np
import pytest
import torch

from tests.util import assert_grad_close

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]

# spans of the implementation (select.hip): a wave owns 256 rows, a workgroup 1024, one pass of the count scan 256 workgroups
WAVE_SPAN, WG_SPAN, SCAN_SPAN = 256, 1024, 256 * 1024
SELECT_T = [1, 63, 64, 65, WAVE_SPAN - 1, WAVE_SPAN, WAVE_SPAN + 1, WG_SPAN - 1, WG_SPAN, WG_SPAN + 1, 200003,
            SCAN_SPAN - 1, SCAN_SPAN, SCAN_SPAN + 1]
V_SEL = 1000


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture()
def L():
    from meant_amd import _lib
    saved = _lib.get_option("deterministic")
    _lib.set_option("deterministic", 0)
    _lib.route_reset()
    yield _lib
    _lib.set_option("deterministic", saved)


def _select_ref(t, V, ign):
    lab = (t != ign) & (t >= 0) & (t < V)
    rows = np.nonzero(lab)[0]
    n, T = len(rows), len(t)
    idx = np.full(T, -1, np.int32); idx[:n] = rows
    inv = np.full(T, -1, np.int32); inv[rows] = np.arange(n, dtype=np.int32)
    tsel = np.full(T, ign, np.int64); tsel[:n] = t[rows]
    return idx, inv, tsel, n


def _label_patterns(rs, T, V, ign):
    """(name, targets): every target that is not meant to be a label carries `ign`"""
    def valid(k):                                        # k labels in [0, V) other than `ign`
        v = rs.randint(0, V - 1, size=k).astype(np.int64)
        return v + (v >= ign) if 0 <= ign < V else v
    none = np.full(T, ign, np.int64)
    yield "none", none
    yield "all", valid(T)
    first = none.copy(); first[0] = valid(1)[0]
    yield "row0", first
    last = none.copy(); last[T - 1] = valid(1)[0]
    yield "rowT-1", last
    some = none.copy(); pick = rs.rand(T) < 0.15; some[pick] = valid(int(pick.sum()))
    yield "15%", some
    mixed = some.copy(); bad = rs.rand(T) < 0.1; mixed[bad] = rs.choice(np.array([-1, V, V + 5], np.int64), size=int(bad.sum()))
    yield "15% + out of range", mixed


def _select_raw(L, t_dev, V, ign):
    """one meant_select_rows call through the raw ABI into poisoned buffers"""
    T = t_dev.numel()
    dev = t_dev.device
    idx = torch.full((T,), 0x55555555, device=dev, dtype=torch.int32)
    inv = torch.full((T,), 0x55555555, device=dev, dtype=torch.int32)
    tsel = torch.full((T,), 0x5555555555, device=dev, dtype=torch.int64)
    count = torch.full((1,), 0x55555555, device=dev, dtype=torch.int32)
    wsb = L.lib.meant_select_rows_ws(T)
    ws = torch.full((wsb,), 0x55, device=dev, dtype=torch.uint8)
    L.check(L.lib.meant_select_rows(t_dev.data_ptr(), T, V, ign, idx.data_ptr(), inv.data_ptr(), tsel.data_ptr(), count.data_ptr(),
                                    ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream), "select_rows")
    torch.cuda.synchronize()
    return idx.cpu().numpy(), inv.cpu().numpy(), tsel.cpu().numpy(), int(count.item())


@pytest.mark.parametrize("T", SELECT_T)
def test_select_rows_matches_numpy(L, dev, T):
    """all four outputs, tails included, equal numpy's; a second run gives the same bits; every call counts once"""
    rs = np.random.RandomState(T % 9973)
    calls = 0
    for ign in (-100, 1):
        for name, t in _label_patterns(rs, T, V_SEL, ign):
            t_dev = torch.from_numpy(t).to(dev)
            ref = _select_ref(t, V_SEL, ign)
            got = _select_raw(L, t_dev, V_SEL, ign)
            again = _select_raw(L, t_dev, V_SEL, ign)
            calls += 2
            assert L.route_count("select_rows") == calls
            for k, what in enumerate(("idx", "inv", "target_sel")):
                assert np.array_equal(got[k], ref[k]), (T, ign, name, what)
                assert np.array_equal(again[k], got[k]), (T, ign, name, what, "second run")
            assert got[3] == ref[3] == again[3], (T, ign, name, "count")


def test_select_rows_wrapper_host_and_device_labels(L, dev):
    """ops.select_rows: labels on the host give the count without reading anything back, labels on the device by one read; the
    lists are the same tensors either way"""
    from meant_amd import ops
    rs = np.random.RandomState(5)
    t = np.full(3000, -100, np.int64)
    pick = rs.rand(3000) < 0.15
    t[pick] = rs.randint(0, V_SEL, int(pick.sum()))
    ref = _select_ref(t, V_SEL, -100)
    a = ops.select_rows(torch.from_numpy(t).view(3, 1000), V_SEL)
    b = ops.select_rows(torch.from_numpy(t).to(dev), V_SEL)
    assert a.n == b.n == ref[3] == int(a.count.item()) == int(b.count.item())
    for got in (a, b):
        assert got.idx.is_cuda and np.array_equal(got.idx.cpu().numpy(), ref[0]) and np.array_equal(got.inv.cpu().numpy(), ref[1])
        assert np.array_equal(got.target_sel.cpu().numpy(), ref[2])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("W", [128, 768])
def test_take_rows_forward_and_backward_are_exact(dev, dtype, W):
    from meant_amd import ops
    T = 300
    g = torch.Generator().manual_seed(W)
    tgt = torch.full((T,), -100, dtype=torch.int64)
    pick = torch.rand(T, generator=g) < 0.15
    tgt[pick] = torch.randint(0, 50, (int(pick.sum()),), generator=g)
    rows = torch.nonzero(pick).flatten()
    n = rows.numel()
    assert n % 8 != 0
    x = torch.randn(T, W, generator=g).to(dtype)
    sel = ops.select_rows(tgt, 50)
    m = ops.padded_rows(sel.n)
    assert sel.n == n and m == (n + 7) // 8 * 8
    xh = x.to(dev).requires_grad_()
    y = ops.take_rows(xh, sel.idx, sel.inv, m)
    assert y.shape == (m, W) and y.dtype == dtype
    assert torch.equal(y[:n].cpu(), x.index_select(0, rows)) and y[n:].abs().max().item() == 0
    dy = torch.randn(m, W, generator=g).to(dtype)
    y.backward(dy.to(dev))
    ref = torch.zeros(T, W, dtype=dtype)
    ref[rows] = dy[:n]
    assert torch.equal(xh.grad.cpu(), ref)


def _ce_case(dev, dtype, labelled):
    """T = 300, d = 64, V = 1001: (x, w, b, target) on the host, 15 % labelled (or none)"""
    T, d, V = 300, 64, 1001
    rs = np.random.RandomState(11)
    x = torch.from_numpy(rs.standard_normal((T, d)).astype("float32"))
    w = torch.from_numpy((rs.standard_normal((V, d)) / 8).astype("float32"))
    b = torch.from_numpy((rs.standard_normal(V) * 0.1).astype("float32"))
    tgt = torch.full((T,), -100, dtype=torch.int64)
    if labelled:
        pick = torch.from_numpy(rs.rand(T) < 0.15)
        tgt[pick] = torch.from_numpy(rs.randint(0, V, int(pick.sum())))
        tgt[int(torch.nonzero(pick)[0])] = V - 1         # the last real row of W next to the padding
        assert int(pick.sum()) % 8 != 0
    if dtype == BF:
        x, w = x.to(BF).float(), w.to(BF).float()        # the operands as the bf16 tier sees them
    return x, w, b, tgt


def _ce_run(dev, dtype, case, rows):
    from meant_amd import ops
    x, w, b, tgt = case
    xh = x.to(dev).to(dtype).requires_grad_()
    wh, bh = torch.nn.Parameter(w.to(dev)), torch.nn.Parameter(b.to(dev))
    loss = ops.vocab_linear_cross_entropy(xh, wh, bh, tgt.to(dev), rows=rows)
    loss.backward()
    return loss.item(), xh.grad, wh.grad, bh.grad


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_vocab_cross_entropy_on_labelled_rows(L, dev, dtype):
    case = _ce_case(dev, dtype, True)
    x, w, b, tgt = case
    xr, wr, br = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    lr = torch.nn.functional.cross_entropy(torch.nn.functional.linear(xr, wr, br), tgt, ignore_index=-100)
    lr.backward()
    lab = _ce_run(dev, dtype, case, "labelled")
    assert L.route_count("select_rows") == 1
    full = _ce_run(dev, dtype, case, "all")
    assert L.route_count("select_rows") == 1
    print(f"loss: labelled {lab[0]:.7f} all {full[0]:.7f} cpu {lr.item():.7f}")
    assert abs(lab[0] - lr.item()) <= 1e-2 * abs(lr.item()), (lab[0], lr.item())
    for got, ref, what in zip(lab[1:], (xr.grad, wr.grad, br.grad), ("dx", "dW", "db")):
        assert got.shape == ref.shape
        assert_grad_close(got, ref, 2e-2, what + " against the CPU")
    # the two routes consume identical operands and differ in the order of fp32 sums alone
    gate = 1e-5 if dtype == torch.float32 else 2e-2
    assert abs(lab[0] - full[0]) <= gate * abs(full[0]), (lab[0], full[0])
    for got, ref, what in zip(lab[1:], full[1:], ("dx", "dW", "db")):
        assert_grad_close(got, ref, gate, what + " against the all-rows route")
    ignored = (tgt == -100).to(dev)
    assert lab[1][ignored].abs().max().item() == 0       # rows the loss ignores: exact zeros, as on the all-rows route


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_vocab_cross_entropy_with_no_labelled_row(L, dev, dtype):
    """n = 0: one padded block of zero rows; the loss is 0 and every gradient is a tensor of zeros, not None"""
    case = _ce_case(dev, dtype, False)
    loss, dx, dw, db = _ce_run(dev, dtype, case, "labelled")
    assert L.route_count("select_rows") == 1
    assert loss == 0.0
    for g, ref in zip((dx, dw, db), case[:3]):
        assert g is not None and g.shape == ref.shape and g.abs().max().item() == 0


# ---- the pretrainer ------------------------------------------------------------------------------------------------------
def _golden_model(dev, dtype):
    import meant_amd as M
    from oracle import meant_oracle as O
    torch.manual_seed(0)
    emb, head = O.mlm_parts()
    m = M.meant_language_pretrainer(2, 128, emb, head, text_dim=128, num_heads=2)
    O.fill_weights_(m, 2468)
    m = m.to(dev).eval()
    m.compute_dtype = dtype
    return m


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_mlm_pretrainer_golden_on_labelled_rows(dev, golden, dtype):
    """test_mlm_pretrainer_golden's loss mode with labelled_only = True: the reference's recorded loss, gradient norms and slices at
    that test's tolerances; 17 of the 72 rows carry a label, so the head runs on 24; labels on the host and on the device give
    the same bits"""
    g = golden("mlm_pretrainer_tiny")
    ids, mask = (torch.from_numpy(g[k]).to(dev) for k in ("ids", "mask"))
    labels = torch.from_numpy(g["labels"])
    T = labels.numel()
    assert T == 72 and int((labels != -100).sum()) == 17
    tol_loss, tol_g = (2e-5, 2e-3) if dtype == torch.float32 else (2e-2, 6e-2)
    losses = []
    for lab in (labels, labels.to(dev)):
        m = _golden_model(dev, dtype)
        loss = m.loss(ids, mask, lab, labelled_only=True)
        assert m.last_head_rows == 24 < T
        losses.append(loss.detach().clone())
        assert abs(loss.item() - float(g["loss"])) < tol_loss * max(1.0, float(g["loss"])), (loss.item(), float(g["loss"]))
        loss.backward()
        params = dict(m.named_parameters())
        floor = 1e-3 * float(np.max(g["grad_norms"]))
        for nm, refn in zip(g["grad_names"], g["grad_norms"]):
            got = params[str(nm)].grad.double().norm().item()
            assert abs(got - refn) <= tol_g * max(refn, floor), (str(nm), got, refn)
        for k in g.files:
            if k.startswith("grad__"):
                p_ = params[k[6:]]
                ref = torch.from_numpy(g[k])
                got = (p_.grad if p_.grad.numel() <= 4096 else p_.grad[:4]).float().cpu()
                assert (got - ref).abs().max().item() <= tol_g * max(ref.abs().max().item(), floor), k
    assert torch.equal(losses[0], losses[1])
    m = _golden_model(dev, dtype)
    m.loss(ids, mask, labels.to(dev), labelled_only=False)
    assert m.last_head_rows == T
    import os
    assert m.labelled_only == (os.environ.get("MEANT_MLM_LABELLED_ONLY", "1") != "0")      # the initial value
    m.labelled_only = True                                # None takes the attribute
    m.loss(ids, mask, labels.to(dev))
    assert m.last_head_rows == 24
    m.labelled_only = False
    m.loss(ids, mask, labels.to(dev))
    assert m.last_head_rows == T
    dense = torch.randint(0, 120, (3, 24))                # every row labelled (causal-LM style): nothing to save, the all-rows route
    m.loss(ids, mask, dense, labelled_only=True)
    assert m.last_head_rows == T


class _StandInHead(torch.nn.Module):
    """the three attributes of a RobertaLMHead, decoder tied to the word embedding (pretrain_mlm.py:318-319)"""

    def __init__(self, emb, d, V):
        super().__init__()
        self.dense = torch.nn.Linear(d, d)
        self.layer_norm = torch.nn.LayerNorm(d, eps=1e-5)
        self.decoder = torch.nn.Linear(d, V)
        self.decoder.weight = emb.weight


def _stand_in_model(dev, dtype):
    import meant_amd as M
    torch.manual_seed(3)
    d, V = 128, 120
    emb = torch.nn.Embedding(V, d)
    m = M.meant_language_pretrainer(1, d, emb, _StandInHead(emb, d, V), text_dim=d, num_heads=2).to(dev).eval()
    m.compute_dtype = dtype
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, V, (3, 24), generator=g)
    mask = torch.ones(3, 24)
    mask[1, 20:] = 0
    labels = torch.full((3, 24), -100, dtype=torch.int64)
    pick = torch.rand(3, 24, generator=g) < 0.15
    labels[pick] = ids[pick]
    assert 0 < int(pick.sum()) and int(pick.sum()) % 8 != 0
    return m, ids.to(dev), mask.to(dev), labels


def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_mlm_pretrainer_stand_in_head_without_hf(L, dev, dtype):
    """nn.Embedding + a three-attribute head: the labelled route against the all-rows route of the same module"""
    m, ids, mask, labels = _stand_in_model(dev, dtype)
    n = int((labels != -100).sum())
    out = {}
    for only in (True, False):
        m.zero_grad(set_to_none=True)
        loss = m.loss(ids, mask, labels.to(dev), labelled_only=only)
        assert m.last_head_rows == ((n + 7) // 8 * 8 if only else 72)
        loss.backward()
        out[only] = (loss.item(), _grads(m))
    assert L.route_count("select_rows") == 1
    gate = 1e-5 if dtype == torch.float32 else 2e-2
    print(f"loss: labelled {out[True][0]:.7f} all {out[False][0]:.7f}")
    assert abs(out[True][0] - out[False][0]) <= gate * abs(out[False][0])
    assert set(out[True][1]) == set(out[False][1]) == {k for k, p in m.named_parameters() if p.requires_grad}
    for k, ref in out[False][1].items():
        assert_grad_close(out[True][1][k], ref, gate, k)
    m.zero_grad(set_to_none=True)
    host = m.loss(ids, mask, labels, labelled_only=True)  # labels left on the host
    assert host.item() == out[True][0]


def test_labelled_route_is_bit_reproducible_under_deterministic(L, dev):
    m, ids, mask, labels = _stand_in_model(dev, BF)
    L.set_option("deterministic", 1)
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        m.loss(ids, mask, labels.to(dev), labelled_only=True).backward()
        assert m.last_head_rows < 72
        runs.append(_grads(m))
    assert runs[0] and set(runs[0]) == set(runs[1])
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_tied_embedding_under_direct_grads_on_labelled_rows(L, dev):
    """a word embedding tied to the vocabulary decoder under GradReducer(direct_grads=True) (the single-process half of
    test_tied_embedding_and_vocab_decoder_reduce_both_contributions): the reduced gradients of a step on the labelled route equal
    the all-rows route's"""
    from meant_amd import ops
    from meant_amd.parallel import GradReducer
    torch.manual_seed(0)
    V, d, T = 1000, 128, 4096
    emb = torch.nn.Embedding(V, d).to(dev)
    lin = torch.nn.Linear(d, d).to(dev)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, V, (T,), generator=g).to(dev)
    tgt = torch.randint(0, V, (T,), generator=g)
    tgt[torch.rand(T, generator=g) >= 0.15] = -100
    n = int((tgt != -100).sum())
    assert n % 8 != 0
    tgt = tgt.to(dev)
    red = GradReducer(list(emb.parameters()) + list(lin.parameters()), direct_grads=True)
    got = {}
    for rows in ("all", "labelled"):
        red.prepare()
        x = ops.embedding(ids, emb.weight, BF)
        h = ops.linear(x, lin.weight, lin.bias)
        loss = ops.vocab_linear_cross_entropy(h, emb.weight, None, tgt, rows=rows)
        loss.backward()
        red.wait()
        torch.cuda.synchronize()
        got[rows] = (loss.item(), emb.weight.grad.detach().clone(), lin.weight.grad.detach().clone(), lin.bias.grad.detach().clone())
    red.close()
    assert L.route_count("select_rows") == 1
    assert abs(got["labelled"][0] - got["all"][0]) <= 2e-2 * abs(got["all"][0])
    for a, b, what in zip(got["labelled"][1:], got["all"][1:], ("embedding", "linear weight", "linear bias")):
        assert b.abs().max().item() > 0
        assert_grad_close(a, b, 2e-2, what)
