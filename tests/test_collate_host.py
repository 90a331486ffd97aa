"""Host-side facts of the device collators (no GPU): the masking rule as tests/collate_ref.py restates it chooses at the rate it is
asked for and its per-epoch seeds are independent; data.collate_seed is that restatement's; DeviceBatchLoader(with_index=True) appends
the slice of shard_indices each batch was cut from; the new symbols are in the header, the ctypes table and the library, and refuse bad
arguments before any launch (the pointers below are made-up addresses that are never dereferenced); the three ops and the collators
raise the package's "no CPU fallback" error on CPU tensors.

The rate cap is a condition, not a measurement: the count of chosen elements among n lies within 4 standard deviations of
Binomial(n, q), q = floor(p 2^24) / 2^24, around n q."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import collate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, -1, -2, -4
SPAN = 1 << 40
A, B_, C_, D_, E_, F_ = (SPAN * (i + 1) for i in range(6))
SEED = 1234
NEW_SYMBOLS = ("meant_mlm_mask", "meant_patchify_raw_masked", "meant_mim_l1_ws", "meant_mim_l1_fwd", "meant_mim_l1_bwd")


def _within_cap(count, n, q):
    return abs(count - n * q) <= 4.0 * math.sqrt(n * q * (1.0 - q))


# ---- the rule -----------------------------------------------------------------------------------------------------------------
def test_rule_matches_a_scalar_evaluation_in_python_integers():
    """the numpy restatement against the rule written out once more with Python's unbounded integers"""
    M = (1 << 64) - 1

    def bits(seed, stream, idx):
        z = (seed + (idx | stream << 60) * 0x9E3779B97F4A7C15) & M
        z = ((z ^ z >> 30) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ z >> 27) * 0x94D049BB133111EB) & M
        return z ^ z >> 31
    for seed in (0, SEED, M, 0xDEADBEEFCAFEF00D):
        for stream in (0, 1, 2, 3):
            idx = np.array([0, 1, 2, 12345, (1 << 31) + 7, (1 << 60) - 1], dtype=np.uint64)
            got = R.bits(seed, stream, idx)
            assert [int(v) for v in got] == [bits(seed, stream, int(i)) for i in idx]
            assert [int(v) for v in R.draw24(seed, stream, idx)] == [bits(seed, stream, int(i)) >> 40 for i in idx]
    assert R.threshold(0.15) == 2516582 and R.threshold(1.0) == 1 << 24 and R.threshold(0.0) == 0


@pytest.mark.parametrize("shape,p", [((8, 128), 0.15), ((64, 512), 0.15), ((2, 4 * 32 * 32), 0.15), ((2, 4 * 224 * 224), 0.15), ((64, 512), 0.5)])
def test_rate_of_the_rule(shape, p):
    rows, E = shape
    ch = R.chosen(SEED, np.arange(rows), E, p)
    q = R.threshold(p) / 2.0 ** 24
    assert _within_cap(int(ch.sum()), ch.size, q), (int(ch.sum()), ch.size * q)


@pytest.mark.parametrize("stream", [1, 2])
def test_rate_of_the_other_streams(stream):
    """streams 1 (replace or not) and 2 (the random id) at 64 x 512: the top 24 bits of either fall below a threshold at its rate, and
    stream 2's ids modulo a vocabulary spread evenly over its halves"""
    idx = R.element_index(np.arange(64), 512)
    for p in (0.8, 0.1):
        q = R.threshold(p) / 2.0 ** 24
        n = int((R.draw24(SEED, stream, idx) < np.uint64(R.threshold(p))).sum())
        assert _within_cap(n, idx.size, q), (stream, p, n)
    low = int(((R.bits(SEED, stream, idx) % np.uint64(64001)) < np.uint64(32000)).sum())
    assert _within_cap(low, idx.size, 32000 / 64001.0)


def test_streams_are_independent_of_each_other():
    idx = R.element_index(np.arange(64), 512)
    a = R.draw24(SEED, 0, idx) < np.uint64(R.threshold(0.5))
    b = R.draw24(SEED, 1, idx) < np.uint64(R.threshold(0.5))
    assert _within_cap(int((a & b).sum()), idx.size, 0.25)


def test_epoch_seeds_are_distinct_and_independent():
    from meant_amd import data
    seeds = [data.collate_seed(SEED, e) for e in range(16)]
    assert seeds == [R.collate_seed(SEED, e) for e in range(16)]
    assert len(set(seeds)) == 16 and all(0 <= s < 1 << 64 for s in seeds)
    assert all(s != SEED + e for e, s in enumerate(seeds))
    assert data.collate_seed(SEED, 0) != data.collate_seed(SEED + 1, 0)
    # epochs 0 and 1 overlap as two independent masks of rate q do: q^2 of the positions, within the same cap
    q = R.threshold(0.15) / 2.0 ** 24
    m0 = R.chosen(seeds[0], np.arange(64), 512, 0.15)
    m1 = R.chosen(seeds[1], np.arange(64), 512, 0.15)
    assert _within_cap(int((m0 & m1).sum()), m0.size, q * q), int((m0 & m1).sum())
    with pytest.raises(ValueError):
        data.collate_seed(SEED, -1)


def test_mask_is_keyed_by_the_sample_not_by_the_batch():
    """a sample's mask is the same whichever rows it shares a call with"""
    whole = R.chosen(SEED, np.arange(8), 128, 0.15)
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    assert (R.chosen(SEED, perm, 128, 0.15) == whole[perm]).all()
    assert (R.chosen(SEED, np.arange(4, 8), 128, 0.15) == whole[4:]).all()


def test_collators_hold_the_rule():
    from meant_amd import data
    c = data.MLMCollator(mask_id=64000, special_ids=(0, 1, 2, 3, 64000), vocab_size=64001, seed=SEED)
    assert (c.p, c.replace, c.random, c.ignore_index) == (0.15, 1.0, 0.0, -100)
    assert c.epoch_seed == R.collate_seed(SEED, 0)
    c.set_epoch(3)
    assert c.epoch_seed == R.collate_seed(SEED, 3)
    m = data.MIMCollator(seed=SEED)
    assert (m.p, m.mask_value, m.unmasked_label, m.on_masked) == (0.15, 0.0, -100.0, False)
    m.set_epoch(2)
    assert m.epoch_seed == R.collate_seed(SEED, 2)
    with pytest.raises(ValueError):
        data.MLMCollator(mask_id=1, special_ids=range(17), vocab_size=10)
    with pytest.raises(ValueError):
        data.MIMCollator(p=1.5)


# ---- the loader's indices -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("world", [1, 2])
def test_loader_appends_the_dataset_indices(shuffle, world):
    from meant_amd import data
    n, bs = 37, 4
    a = np.arange(n * 3, dtype=np.float32).reshape(n, 3)
    b = np.arange(n, dtype=np.int64)
    for rank in range(world):
        for epoch in (0, 1):
            ld = data.DeviceBatchLoader(a, None, b, batch_size=bs, device="cpu", shuffle=shuffle, seed=5, rank=rank, world=world, with_index=True)
            ld.set_epoch(epoch)
            want = data.shard_indices(n, rank, world, bs, shuffle, 5, epoch)
            batches = [tuple(None if t is None else t.clone() for t in batch) for batch in ld]
            assert len(batches) == len(ld) == n // (bs * world)
            for i, batch in enumerate(batches):
                assert len(batch) == 4 and batch[1] is None
                idx = batch[-1]
                assert idx.dtype == torch.int64 and idx.shape == (bs,)
                assert idx.tolist() == want[i * bs:(i + 1) * bs].tolist()
                assert batch[2].tolist() == idx.tolist()                     # the rows really are those samples
                assert torch.equal(batch[0], torch.from_numpy(a[idx.numpy()]))
    plain = data.DeviceBatchLoader(a, None, b, batch_size=bs, device="cpu", shuffle=shuffle, seed=5)
    first = next(iter(plain))
    assert len(first) == 3 and first[1] is None                             # the old tuple


# ---- symbols and argument checks -------------------------------------------------------------------------------------------------
def test_symbols_in_header_table_and_library():
    from meant_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "meant_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES
        assert re.search(r" T %s$" % name, out, flags=re.M), name


def _mlm(lib, ids=A, am=None, mdt=0, sids=None, base=0, bound=1 << 31, spec=D_, ns=5, B=4, S=8, thr=100, trep=1 << 24, trand=0, V=64001,
         out=B_, labels=C_):
    return lib.meant_mlm_mask(ids, am, mdt, sids, base, bound, spec, ns, B, S, SEED, thr, trep, trand, 64000, V, -100, out, labels, None)


@pytest.mark.parametrize("kw", [dict(ids=None), dict(out=None), dict(labels=None), dict(B=0), dict(S=0), dict(V=0), dict(ns=17), dict(ns=-1),
                                dict(spec=None), dict(thr=(1 << 24) + 1), dict(trep=(1 << 24) + 1), dict(trand=(1 << 24) + 1), dict(mdt=5),
                                dict(mdt=-1), dict(ids=A + 4), dict(labels=C_ + 4), dict(am=E_ + 2, mdt=0), dict(am=E_ + 4, mdt=2),
                                dict(sids=F_ + 4), dict(labels=A), dict(labels=B_), dict(out=A + 8), dict(labels=A + 8 * 31)])
def test_mlm_mask_rejects_bad_arguments_before_any_launch(kw):
    from meant_amd import _lib
    assert _mlm(_lib.lib, **kw) == ERR_ARG, kw
    assert b"mlm_mask" in _lib.lib.meant_last_error()


def test_index_limit_of_the_rule():
    """sample id * elements per sample stays below 2^60: refused on the host, with the caller's bound where the ids are on the device"""
    from meant_amd import _lib
    lib = _lib.lib
    assert _mlm(lib, base=(1 << 60) // 8, B=1) == ERR_UNSUPPORTED            # (base + 1) * 8 > 2^60
    assert b"2^60" in lib.meant_last_error()
    assert _mlm(lib, base=-1) == ERR_UNSUPPORTED
    assert _mlm(lib, sids=F_, bound=(1 << 57) + 1) == ERR_UNSUPPORTED
    assert lib.meant_patchify_raw_masked(A, 0, 0.0, 1.0, B_, 2, 4, 32, 32, 16, 0, SEED, 100, None, 1 << 48, 0, 0.0, None) == ERR_UNSUPPORTED
    assert b"2^60" in lib.meant_last_error()
    assert lib.meant_mim_l1_fwd(A, 0, B_, 0, 0.0, 1.0, 2, 4, 3, 32, 32, SEED, 100, F_, 0, (1 << 48) + 1, -100.0, 0, C_, D_, E_, 1 << 20, None) == ERR_UNSUPPORTED
    assert b"2^60" in lib.meant_last_error()


def test_mim_entries_reject_bad_arguments_before_any_launch():
    from meant_amd import _lib
    lib = _lib.lib

    def pm(images=A, raw=0, patches=B_, G=2, C=4, Hh=32, Ww=32, p=16, dtype=0, thr=100, sids=None):
        return lib.meant_patchify_raw_masked(images, raw, 0.0, 1.0, patches, G, C, Hh, Ww, p, dtype, SEED, thr, sids, 0, 1 << 31, 0.0, None)
    for kw in (dict(images=None), dict(patches=None), dict(G=0), dict(C=0), dict(p=0), dict(p=24), dict(Ww=40), dict(dtype=2), dict(raw=4), dict(raw=-1),
               dict(thr=(1 << 24) + 1), dict(images=A + 2), dict(raw=2, images=A + 4), dict(patches=B_ + 2), dict(sids=F_ + 1)):
        assert pm(**kw) == ERR_ARG, kw
        assert b"patchify_raw_masked" in lib.meant_last_error()

    def fwd(out=A, dtype=0, images=B_, raw=0, B=2, C=4, Co=3, thr=100, loss=C_, count=D_, ws=E_, wsb=1 << 20, sids=None):
        return lib.meant_mim_l1_fwd(out, dtype, images, raw, 0.0, 1.0, B, C, Co, 32, 32, SEED, thr, sids, 0, 1 << 31, -100.0, 0, loss, count, ws, wsb, None)
    for kw in (dict(out=None), dict(images=None), dict(loss=None), dict(count=None), dict(B=0), dict(Co=0), dict(Co=5), dict(dtype=2), dict(raw=7),
               dict(thr=(1 << 24) + 1), dict(out=A + 2), dict(images=B_ + 1), dict(count=D_ + 4), dict(loss=C_ + 2), dict(sids=F_ + 4)):
        assert fwd(**kw) == ERR_ARG, kw
        assert b"mim_l1_fwd" in lib.meant_last_error()
    assert fwd(ws=None) == ERR_WORKSPACE and fwd(wsb=8) == ERR_WORKSPACE

    def bwd(out=A, dtype=0, images=B_, raw=0, Co=3, on_masked=0, g=C_, count=D_, dout=E_):
        return lib.meant_mim_l1_bwd(out, dtype, images, raw, 0.0, 1.0, 2, 4, Co, 32, 32, SEED, 100, None, 0, 1 << 31, -100.0, on_masked, g, count, dout, None)
    for kw in (dict(out=None), dict(g=None), dict(dout=None), dict(Co=5), dict(on_masked=1, count=None), dict(dout=A), dict(g=C_ + 2),
               dict(dtype=1, dout=E_ + 1)):
        assert bwd(**kw) == ERR_ARG, kw
        assert b"mim_l1_bwd" in lib.meant_last_error()


def test_workspace_size():
    """one float partial and one 32-bit count per 4096 elements, each array rounded up to 256 bytes"""
    from meant_amd import _lib
    ws = _lib.lib.meant_mim_l1_ws
    assert ws(0) == 0 and ws(-1) == 0 and ws((1 << 40) + 1) == 0
    assert ws(1) == 512 and ws(4096 * 64) == 512 and ws(4096 * 64 + 1) == 1024
    assert ws(128 * 3 * 224 * 224) == 2 * ((4704 * 4 + 255) // 256 * 256)


# ---- no CPU fallback ----------------------------------------------------------------------------------------------------------------
def test_no_cpu_fallback():
    import meant_amd
    from meant_amd import data, ops
    err = "no CPU fallback|There is no CPU fallback"
    ids = torch.randint(5, 100, (2, 8))
    img = torch.rand(2, 4, 32, 32)
    with pytest.raises(RuntimeError, match=err):
        ops.mlm_mask(ids, mask_id=4, special_ids=(0, 1), vocab_size=100)
    # the special-token list is an operand like the others: a host tensor never reaches the kernel, whatever the other tensors are
    with pytest.raises(RuntimeError, match=err):
        ops._special_ids(torch.tensor([0, 1, 2, 3, 64000]), torch.device("cpu"))
    with pytest.raises(RuntimeError, match=err):
        ops.mlm_mask(ids, mask_id=4, special_ids=torch.tensor([0, 1]), vocab_size=100)
    with pytest.raises(ValueError, match="int64"):                               # argument checks need no device
        ops._special_ids(torch.tensor([0, 1], dtype=torch.int32), torch.device("cpu"))
    with pytest.raises(ValueError, match="at most 16"):
        ops._special_ids(torch.arange(17), torch.device("cpu"))
    with pytest.raises(ValueError, match="at most 16"):
        ops._special_ids(range(17), torch.device("cpu"))
    assert ops._special_ids((), torch.device("cpu")) == (None, 0) and ops._special_ids(None, torch.device("cpu")) == (None, 0)
    with pytest.raises(RuntimeError, match=err):
        ops.patchify_masked(img, 16, torch.float32)
    with pytest.raises(RuntimeError, match=err):
        ops.mim_l1_loss(torch.rand(2, 3, 32, 32), img)
    with pytest.raises(RuntimeError, match=err):
        data.MLMCollator(mask_id=4, special_ids=(0, 1), vocab_size=100)(ids, torch.ones(2, 8))
    m = meant_amd.meant_vision_pretrainer(1, torch.nn.Identity(), 128, patch_res=16, channels=4, height=32, width=32, image_dim=128, num_heads=2)
    with pytest.raises(RuntimeError, match=err):
        m.loss(img, data.MIMCollator())
