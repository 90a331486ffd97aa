"""The device collators against tests/collate_ref.py, the numpy restatement of their masking rule.

Everything integer -- masked ids, labels, counts, the positions a patch row is masked at -- is compared at zero tolerance.  The masked
patch rows are compared bit for bit with ops.patchify of the host-built masked image (same fp32 arithmetic, then a select; the bf16 tier
against the bf16 rounding of that fp32 result).  The L1 loss is compared with torch in float64 on the host-built labels within the
project's own MIM gate (tests/test_gpu_models.py: 1e-5 relative in fp32, 1e-2 in bf16), its gradient with sign(out - label) / N within
1 ulp of fp32 (its bf16 rounding in the bf16 tier)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import collate_ref as R

pytestmark = pytest.mark.gpu

V, MASK_ID = 64001, 64000
SPECIAL = (0, 1, 2, 3, 64000)                          # BERTweet's all_special_ids
SEED = 1234
MEAN, STD = 0.3, 1.7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- MLM ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mlm_case(B, S):
    """ids in [0, 64001) with <s> first, </s> last and <pad> behind a per-row length; the padding-tail attention mask (never written to)"""
    rs = np.random.RandomState(B * 1000 + S)
    ids = rs.randint(0, V, size=(B, S)).astype(np.int64)
    mask = np.ones((B, S), dtype=np.float32)
    for b in range(B):
        n = S if b == 0 else rs.randint(max(1, S // 2), S + 1)
        ids[b, 0] = 0
        ids[b, n - 1] = 2
        ids[b, n:] = 1
        mask[b, n:] = 0
    if S > 8:
        ids[:, 3] = MASK_ID                            # a special id in the middle of the row, and one the random draw could also hit
        mask[B - 1, 5] = 0                             # a hole that is no padding: an ordinary id under a zero of the mask
    return ids, mask


def _mlm_device(dev, ids, mask, sample_ids=None, mask_dtype=torch.float32, **kw):
    from meant_amd import ops
    t_ids = torch.from_numpy(ids).to(dev)
    t_mask = None if mask is None else torch.from_numpy(mask).to(dev).to(mask_dtype)
    t_sid = None if sample_ids is None else torch.from_numpy(np.asarray(sample_ids, dtype=np.int64)).to(dev)
    out, labels = ops.mlm_mask(t_ids, t_mask, t_sid, mask_id=MASK_ID, special_ids=SPECIAL, vocab_size=V, seed=SEED, **kw)
    assert torch.equal(t_ids.cpu(), torch.from_numpy(ids))                       # the input is left alone
    return out.cpu().numpy(), labels.cpu().numpy()


def _mlm_check(ids, mask, got_out, got_labels, exp):
    exp_out, exp_labels, ch = exp
    assert np.array_equal(got_out, exp_out) and np.array_equal(got_labels, exp_labels)
    special = np.isin(ids, np.array(SPECIAL))
    assert not (ch & special).any() and not (ch & (mask == 0)).any()            # no special or padded position is ever chosen
    assert (got_labels[~ch] == -100).all() and (got_out[~ch] == ids[~ch]).all()  # every unchosen position keeps its id
    assert (got_labels[ch] == ids[ch]).all()


@pytest.mark.parametrize("mask_dtype", [torch.float32, torch.int64, torch.bfloat16, torch.int32, torch.uint8, torch.bool],
                         ids=["f32mask", "i64mask", "bf16mask", "i32mask", "u8mask", "boolmask"])
@pytest.mark.parametrize("shape", [(1, 1), (3, 17), (8, 128), (64, 512)], ids=lambda s: "x".join(map(str, s)))
def test_mlm_mask_outputs(dev, shape, mask_dtype):
    ids, mask = mlm_case(*shape)
    sid = np.arange(shape[0])
    exp = R.mlm_expected(ids, mask, sid, SPECIAL, SEED, 0.15, MASK_ID, V)
    got_out, got_labels = _mlm_device(dev, ids, mask, p=0.15, mask_dtype=mask_dtype)
    _mlm_check(ids, mask, got_out, got_labels, exp)
    assert (got_out[exp[2]] == MASK_ID).all()                                    # the reference's recipe: every chosen id becomes <mask>
    if ids.size >= 1024:
        assert exp[2].any()


@pytest.mark.parametrize("shape", [(3, 17), (8, 128), (64, 512)], ids=lambda s: "x".join(map(str, s)))
def test_mlm_mask_bert_recipe(dev, shape):
    ids, mask = mlm_case(*shape)
    exp = R.mlm_expected(ids, mask, np.arange(shape[0]), SPECIAL, SEED, 0.15, MASK_ID, V, replace=0.8, random=0.1)
    got_out, got_labels = _mlm_device(dev, ids, mask, p=0.15, replace=0.8, random=0.1)
    _mlm_check(ids, mask, got_out, got_labels, exp)
    if shape == (64, 512):                                                        # all three outcomes occur
        ch = exp[2]
        kept = ch & (got_out == ids)
        rand = ch & (got_out != ids) & (got_out != MASK_ID)
        assert kept.any() and rand.any() and (ch & (got_out == MASK_ID)).any()
        assert (got_out[rand] >= 0).all() and (got_out[rand] < V).all()


def test_mlm_mask_without_a_mask_and_in_place(dev):
    from meant_amd import ops
    ids, mask = mlm_case(8, 128)
    exp = R.mlm_expected(ids, None, np.arange(8), SPECIAL, SEED, 0.15, MASK_ID, V, replace=0.8, random=0.1)
    got_out, got_labels = _mlm_device(dev, ids, None, p=0.15, replace=0.8, random=0.1)
    assert np.array_equal(got_out, exp[0]) and np.array_equal(got_labels, exp[1])
    t = torch.from_numpy(ids).to(dev)                                            # ids_out aliasing ids
    out, labels = ops.mlm_mask(t, None, None, mask_id=MASK_ID, special_ids=SPECIAL, vocab_size=V, seed=SEED, p=0.15, replace=0.8, random=0.1, out=t)
    assert out is t
    assert np.array_equal(t.cpu().numpy(), exp[0]) and np.array_equal(labels.cpu().numpy(), exp[1])


def test_mlm_mask_is_keyed_by_the_sample(dev):
    """rows 0..7 in one call = two calls of four = a call on a row permutation with the permuted sample ids"""
    ids, mask = mlm_case(8, 128)
    kw = dict(p=0.15, replace=0.8, random=0.1)
    whole_out, whole_labels = _mlm_device(dev, ids, mask, **kw)
    for lo in (0, 4):
        o, l = _mlm_device(dev, ids[lo:lo + 4].copy(), mask[lo:lo + 4].copy(), sample_base=lo, **kw)
        assert np.array_equal(o, whole_out[lo:lo + 4]) and np.array_equal(l, whole_labels[lo:lo + 4])
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    o, l = _mlm_device(dev, ids[perm].copy(), mask[perm].copy(), sample_ids=perm, **kw)
    assert np.array_equal(o, whole_out[perm]) and np.array_equal(l, whole_labels[perm])
    far = np.arange(8) + (1 << 40)                                               # dataset indices past 2^31 * S
    exp = R.mlm_expected(ids, mask, far, SPECIAL, SEED, 0.15, MASK_ID, V, replace=0.8, random=0.1)
    o, l = _mlm_device(dev, ids, mask, sample_ids=far, id_bound=1 << 41, **kw)
    assert np.array_equal(o, exp[0]) and np.array_equal(l, exp[1])


def test_mlm_mask_special_ids_as_a_tensor(dev):
    """a device tensor of special ids gives the sequence's result; a host tensor raises before anything is launched"""
    from meant_amd import ops
    ids, mask = mlm_case(8, 128)
    exp = R.mlm_expected(ids, mask, np.arange(8), SPECIAL, SEED, 0.15, MASK_ID, V)
    t_ids, t_mask = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
    kw = dict(mask_id=MASK_ID, vocab_size=V, seed=SEED, p=0.15)
    out, labels = ops.mlm_mask(t_ids, t_mask, special_ids=torch.tensor(SPECIAL, device=dev), **kw)
    assert np.array_equal(out.cpu().numpy(), exp[0]) and np.array_equal(labels.cpu().numpy(), exp[1])
    with pytest.raises(RuntimeError, match="no CPU fallback|There is no CPU fallback"):
        ops.mlm_mask(t_ids, t_mask, special_ids=torch.tensor(SPECIAL), **kw)
    with pytest.raises(ValueError, match="int64"):
        ops.mlm_mask(t_ids, t_mask, special_ids=torch.tensor(SPECIAL, device=dev, dtype=torch.int32), **kw)
    torch.cuda.synchronize()


@pytest.mark.parametrize("pin", [0, 1], ids=["staged", "page_locked"])
@pytest.mark.parametrize("shuffle", [False, True], ids=["in_order", "shuffled"])
def test_loader_appends_the_dataset_indices_on_the_device(dev, shuffle, pin):
    """DeviceBatchLoader(with_index=True) on the GPU: the index tensor of every batch is the slice of shard_indices the batch was cut
    from, it travels with the batch's rows (both double-buffer slots are reused over seven batches, across two epochs), and the
    collator keyed by it masks every sample as a call on the whole data set does"""
    from meant_amd import data, ops
    n, bs, S = 29, 4, 16
    ids_all, _ = mlm_case(n, S)
    rows = np.arange(n * 3, dtype=np.float64).reshape(n, 3)
    whole = R.mlm_expected(ids_all, None, np.arange(n), SPECIAL, SEED, 0.15, MASK_ID, V)
    ld = data.DeviceBatchLoader(rows, ids_all, batch_size=bs, device=dev, shuffle=shuffle, seed=5, with_index=True, pin_source_bytes=pin)
    for epoch in (0, 1):
        want = data.shard_indices(n, 0, 1, bs, shuffle, 5, epoch)
        seen = 0
        for b, (r, ids, idx) in enumerate(ld):
            assert idx.is_cuda and idx.dtype == torch.int64 and idx.shape == (bs,)
            sl = want[b * bs:(b + 1) * bs]
            assert idx.cpu().tolist() == sl.tolist()
            assert torch.equal(r.cpu(), torch.from_numpy(rows[sl])) and torch.equal(ids.cpu(), torch.from_numpy(ids_all[sl]))
            out, labels = ops.mlm_mask(ids, None, idx, mask_id=MASK_ID, special_ids=SPECIAL, vocab_size=V, seed=SEED, p=0.15)
            assert np.array_equal(out.cpu().numpy(), whole[0][sl]) and np.array_equal(labels.cpu().numpy(), whole[1][sl])
            seen += 1
        assert seen == len(ld) == n // bs
    ld.close()
    plain = next(iter(data.DeviceBatchLoader(rows, ids_all, batch_size=bs, device=dev)))
    assert len(plain) == 2                                                        # the old tuple


def test_mlm_labels_feed_select_rows(dev):
    from meant_amd import data, ops
    ids, mask = mlm_case(64, 512)
    coll = data.MLMCollator(mask_id=MASK_ID, special_ids=SPECIAL, vocab_size=V, seed=SEED)
    coll.set_epoch(2)
    exp = R.mlm_expected(ids, mask, np.arange(64), SPECIAL, R.collate_seed(SEED, 2), 0.15, MASK_ID, V)
    out, labels = coll(torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev))
    assert np.array_equal(out.cpu().numpy(), exp[0]) and np.array_equal(labels.cpu().numpy(), exp[1])
    sel = ops.select_rows(labels, V)
    assert sel.n == int(exp[2].sum()) == int(sel.count.item())
    assert np.array_equal(sel.idx[:sel.n].cpu().numpy(), np.flatnonzero(exp[2].reshape(-1)))


# ---- MIM: the masked patch rows ---------------------------------------------------------------------------------------------------
RAW = {"f64": torch.float64, "f32": torch.float32, "u8": torch.uint8, "bf16": torch.bfloat16}


def raw_images(kind, shape, seed):
    """(torch tensor in its storage type, the same values as a numpy array)"""
    rs = np.random.RandomState(seed)
    if kind == "u8":
        a = rs.randint(0, 256, size=shape).astype(np.uint8)
        return torch.from_numpy(a), a
    a = rs.standard_normal(shape) * 2.0 + 0.3
    if kind == "f64":
        return torch.from_numpy(a), a
    t = torch.from_numpy(a.astype(np.float32))
    if kind == "bf16":
        t = t.to(torch.bfloat16)
        return t, t.float().numpy()
    return t, t.numpy()


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["f64", "f32", "u8", "bf16"])
def test_patchify_masked(dev, kind, out_dtype):
    from meant_amd import ops
    G = 3
    sid = np.array([7, 2, 11])                                                    # shuffled dataset indices
    t_sid = torch.from_numpy(sid).to(dev)
    for C in (3, 4):
        for Hh, Ww, p in ((32, 32, 16), (32, 48, 16), (24, 40, 8)):
            img, img_np = raw_images(kind, (G, C, Hh, Ww), seed=C * 100 + Ww)
            inputs, _, mask = R.mim_inputs_labels(img_np, sid, SEED, 0.15, MEAN, STD, mask_value=0.25)
            assert mask.any() and not mask.all()
            want32 = ops.patchify(torch.from_numpy(inputs).to(dev), p, torch.float32)
            want = want32 if out_dtype == torch.float32 else want32.to(torch.bfloat16)
            got = ops.patchify_masked(img.to(dev), p, out_dtype, MEAN, STD, prob=0.15, seed=SEED, sample_ids=t_sid, mask_value=0.25)
            assert got.dtype == out_dtype and got.shape == want.shape
            assert torch.equal(got, want), (kind, C, Hh, Ww, p)
            # p = 0 is the unmasked pipeline itself
            assert torch.equal(ops.patchify_masked(img.to(dev), p, out_dtype, MEAN, STD, prob=0.0, seed=SEED, sample_ids=t_sid),
                               ops.patchify(img.to(dev), p, out_dtype, MEAN, STD))
    base = ops.patchify_masked(img.to(dev), p, out_dtype, MEAN, STD, prob=0.15, seed=SEED, sample_base=5)       # base + row
    inputs, _, _ = R.mim_inputs_labels(img_np, np.arange(5, 5 + G), SEED, 0.15, MEAN, STD)
    assert torch.equal(base, ops.patchify(torch.from_numpy(inputs).to(dev), p, torch.float32).to(out_dtype))


# ---- MIM: the loss ------------------------------------------------------------------------------------------------------------------
L1_CASES = {"one_partial": ((1, 1, 8, 8), 1, "f32"), "co_below_c": ((2, 3, 32, 32), 4, "f64"), "ragged": ((5, 3, 40, 56), 3, "u8"),
            "ragged_bf16raw": ((5, 3, 40, 56), 4, "bf16")}


@functools.lru_cache(maxsize=None)
def l1_case(name, tier):
    """inputs and the float64 reference of one case (never written to): out is random, with a few elements planted equal to their labels"""
    (B, Co, Hh, Ww), C, kind = L1_CASES[name]
    img, img_np = raw_images(kind, (B, C, Hh, Ww), seed=len(name) + C)
    sid = np.random.RandomState(3).permutation(50)[:B]
    _, labels, mask = R.mim_inputs_labels(img_np, sid, SEED, 0.15, MEAN, STD)
    labels, mask = np.ascontiguousarray(labels[:, :Co]), np.ascontiguousarray(mask[:, :Co])
    rs = np.random.RandomState(17)
    out = torch.from_numpy((rs.standard_normal(labels.shape) * 3.0).astype(np.float32))
    flat, lab = out.view(-1), torch.from_numpy(labels).view(-1)
    unchosen = np.flatnonzero(~mask.reshape(-1))[:3]
    flat[unchosen] = lab[unchosen]                                                # -100 is exact in bf16 too
    planted = list(unchosen)
    if tier == torch.float32 and mask.any():
        chosen = np.flatnonzero(mask.reshape(-1))[:2]
        flat[chosen] = lab[chosen]
        planted += list(chosen)
    out = out.to(tier)
    od, ld = out.double(), torch.from_numpy(labels).double()
    return dict(img=img, sid=sid, out=out, labels=labels, mask=mask, planted=np.array(planted), Co=Co,
                loss=F.l1_loss(od, ld).item(), sign=torch.sign(od - ld).numpy(),
                masked_loss=((od - ld).abs() * torch.from_numpy(mask)).sum().item() / max(int(mask.sum()), 1))


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32)))


def _l1_run(dev, c, on_masked=False):
    from meant_amd import ops
    out = c["out"].to(dev).requires_grad_()
    loss, count = ops.mim_l1_loss(out, c["img"].to(dev), prob=0.15, seed=SEED, sample_ids=torch.from_numpy(c["sid"]).to(dev), mean=MEAN, std=STD,
                                  on_masked=on_masked, return_count=True)
    loss.backward()
    return loss.detach(), count, out.grad


@pytest.mark.parametrize("tier", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(L1_CASES))
@pytest.mark.parametrize("on_masked", [False, True], ids=["all", "masked"])
def test_mim_l1_loss(dev, name, tier, on_masked):
    c = l1_case(name, tier)
    loss, count, dout = _l1_run(dev, c, on_masked)
    n_chosen = int(c["mask"].sum())
    assert loss.dtype == torch.float32 and loss.dim() == 0 and dout.dtype == tier
    assert count.dtype == torch.int64 and int(count.item()) == n_chosen
    ref = c["masked_loss"] if on_masked else c["loss"]
    tol = 1e-5 if tier == torch.float32 else 1e-2
    print(f"{name} {tier} on_masked={on_masked}: loss {loss.item():.9g} ref {ref:.9g} chosen {n_chosen}")
    assert abs(loss.item() - ref) <= tol * abs(ref), (loss.item(), ref)
    div = max(n_chosen, 1) if on_masked else c["mask"].size
    want = (c["sign"] * (c["mask"] if on_masked else 1.0)) / div                  # float64
    want32 = want.astype(np.float32)
    got = dout.float().cpu().numpy()
    if tier == torch.float32:
        assert (np.abs(got.astype(np.float64) - want) <= _ulp32(want32)).all()
    else:
        assert np.array_equal(got, torch.from_numpy(want32).to(torch.bfloat16).float().numpy())
    assert (got.reshape(-1)[c["planted"]] == 0).all()                             # out == label: exactly 0, as L1Loss
    if on_masked:
        assert (got[~c["mask"]] == 0).all()
    again = _l1_run(dev, c, on_masked)                                            # ordered sums: the same bits
    assert torch.equal(again[0], loss) and torch.equal(again[2], dout) and torch.equal(again[1], count)


def test_mim_l1_loss_scales_its_gradient_on_the_device_and_takes_base_ids(dev):
    from meant_amd import ops
    c = l1_case("co_below_c", torch.float32)
    B = c["out"].shape[0]
    img_np = c["img"].numpy()
    _, labels, mask = R.mim_inputs_labels(img_np, np.arange(9, 9 + B), SEED, 0.15, MEAN, STD)
    labels = labels[:, :c["Co"]]
    out = c["out"].to(dev).requires_grad_()
    loss = ops.mim_l1_loss(out, c["img"].to(dev), prob=0.15, seed=SEED, sample_base=9, mean=MEAN, std=STD)
    ref = F.l1_loss(c["out"].double(), torch.from_numpy(labels).double()).item()
    assert abs(loss.item() - ref) <= 1e-5 * ref
    (loss * 3.0).backward()
    want = np.sign(c["out"].double().numpy() - labels.astype(np.float64)) * 3.0 / labels.size
    assert (np.abs(out.grad.cpu().numpy().astype(np.float64) - want) <= _ulp32(want.astype(np.float32))).all()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_masked", [False, True], ids=["all", "masked"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_mim_pretrainer_loss_end_to_end(dev, dtype, on_masked):
    """m.loss(raw images, collator) = L1Loss(m(host-masked image), host labels[:, :3]): loss and every parameter's gradient norm within the
    gates of test_mim_pretrainer_golden"""
    import meant_amd as M
    from meant_amd import data
    from oracle import meant_oracle as O
    torch.manual_seed(0)
    m = M.meant_vision_pretrainer(1, O.mim_decoder(), 128, patch_res=16, channels=4, height=32, width=32, image_dim=128, num_heads=2)
    O.fill_weights_(m, 1357)
    m = m.to(dev).eval()
    m.compute_dtype = dtype
    img, img_np = raw_images("f64", (3, 4, 32, 32), seed=77)
    sid = np.array([12, 3, 40])
    coll = data.MIMCollator(p=0.15, on_masked=on_masked, seed=SEED)
    coll.set_epoch(1)
    inputs, labels, mask = R.mim_inputs_labels(img_np, sid, R.collate_seed(SEED, 1), 0.15, MEAN, STD)
    # the reference's way: masked image and labels built on the host, both uploaded, L1Loss from ATen
    out = m(torch.from_numpy(inputs).to(dev))
    lab = torch.from_numpy(labels).to(dev)[:, 0:3]
    if on_masked:
        mk = torch.from_numpy(mask).to(dev)[:, 0:3]
        ref = ((out.float() - lab).abs() * mk).sum() / mk.sum().clamp(min=1)
    else:
        ref = F.l1_loss(out.float(), lab)
    ref.backward()
    ref_norms = {k: p.grad.double().norm().item() for k, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    # the device's way: raw float64 pixels and the dataset indices
    m.patchEmbed[0].set_normalization(MEAN, STD)
    loss = m.loss(img.to(dev), coll, torch.from_numpy(sid).to(dev))
    loss.backward()
    tol_loss, tol_g = (1e-5, 2e-3) if dtype == torch.float32 else (1e-2, 6e-2)
    print(f"{dtype} on_masked={on_masked}: loss {loss.item():.9g} ref {ref.item():.9g}")
    assert abs(loss.item() - ref.item()) <= tol_loss * abs(ref.item()), (loss.item(), ref.item())
    floor = 1e-3 * max(ref_norms.values())
    got_norms = {k: p.grad.double().norm().item() for k, p in m.named_parameters() if p.grad is not None}
    assert set(got_norms) == set(ref_norms) and len(ref_norms) > 10
    for k, refn in ref_norms.items():
        assert abs(got_norms[k] - refn) <= tol_g * max(refn, floor), (k, got_norms[k], refn)


def test_one_mlm_step_with_the_device_collator(dev, golden):
    """meant_language_pretrainer.loss on the collator's two outputs = the same call on the restatement's (ids, labels) uploaded from the
    host, bit for bit under option deterministic = 1"""
    import meant_amd as M
    from meant_amd import _lib, data
    from oracle import meant_oracle as O
    g = golden("mlm_pretrainer_tiny")
    ids, mask = g["ids"].astype(np.int64), g["mask"]
    special, mask_id, vocab = (0, 1, 2, 3), 4, 120
    coll = data.MLMCollator(0.3, mask_id=mask_id, special_ids=special, vocab_size=vocab, replace=0.8, random=0.1, seed=SEED)
    sid = np.array([9, 1, 4])
    exp_ids, exp_labels, ch = R.mlm_expected(ids, mask, sid, special, R.collate_seed(SEED, 0), 0.3, mask_id, vocab, replace=0.8, random=0.1)
    assert ch.sum() >= 4
    torch.manual_seed(0)
    emb, head = O.mlm_parts()
    m = M.meant_language_pretrainer(2, 128, emb, head, text_dim=128, num_heads=2)
    O.fill_weights_(m, 2468)
    m = m.to(dev).eval()
    t_mask = torch.from_numpy(mask).to(dev)
    before = _lib.get_option("deterministic")
    _lib.set_option("deterministic", 1)
    try:
        got_ids, got_labels = coll(torch.from_numpy(ids).to(dev), t_mask, torch.from_numpy(sid).to(dev))
        assert np.array_equal(got_ids.cpu().numpy(), exp_ids) and np.array_equal(got_labels.cpu().numpy(), exp_labels)
        loss_dev = m.loss(got_ids, t_mask, got_labels)
        loss_dev.backward()
        assert m.last_head_rows < ids.size                                        # the labelled-rows route, fed from the device
        m.zero_grad(set_to_none=True)
        loss_host = m.loss(torch.from_numpy(exp_ids).to(dev), t_mask, torch.from_numpy(exp_labels).to(dev))
        loss_host.backward()
    finally:
        _lib.set_option("deterministic", before)
    assert torch.isfinite(loss_dev) and torch.equal(loss_dev, loss_host)
