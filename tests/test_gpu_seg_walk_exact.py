"""The per-id summation kernels on integers, at zero tolerance: meant_embedding_bwd_sorted[_range], meant_embedding_bwd_seg and the
segmented sum of meant_qkv_embed_bwd_by_id, which share one walk over the sorted ids (seg_walk, csrc/seg_sum.h).

With integer-valued gradients in [-4, 4] every sum these kernels form is an integer below 2^24 in magnitude, so fp32 holds it
exactly whatever the order of the additions (float atomics included), and the result must equal an int64 reference with torch.equal:
a row that is dropped, doubled or added to the wrong id shows.  n <= 4864 keeps a run's sum within 4 * 4864 = 19 456, which the
hi | lo bf16 split of the by-id route holds exactly too (bf16(s) + bf16(s - bf16(s)) == s for every integer |s| <= 40 000); each
test asserts that bound on its reference.

Ids over V = 300, shuffled over the token rows.  At n = 4864 = 19 stretches of 256 sorted entries, in sorted order: id 0 (3 entries)
and id 3 (100) inside stretch 0; id 5 (200) across exactly one stretch end; id 7 (4400) from stretch 1 to stretch 18 -- it covers 16
whole stretches (open on both sides: the "from the left" slot) and its 18 partial sums are a long list of seg_long_kernel; then ids
that occur a few times each, and id V - 1.  Ids 100 .. 149 never occur: their rows stay exactly zero.  The smaller n carry id 7 on
half the tokens and ids 0 and V - 1; at n = 257 the two entries of V - 1 sit on either side of the only stretch end.
Widths: 8 (one chunk, lanes 1 .. 63 idle), 520 (65 chunks: the second chunk on lane 0 only), 1024 (both chunks on every lane, the
sorted kernel's limit), 1032 (129 chunks in two column blocks of 65 and 64; meant_embedding_bwd_seg only)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V = 300
BOUND = 19456
NS = [1, 255, 256, 257, 4864]
EPS = 1e-8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture()
def option():
    from meant_amd import _lib
    saved = _lib.get_option("deterministic")
    yield _lib.set_option
    _lib.set_option("deterministic", saved)


def _ids(n):
    rs = np.random.RandomState(n)
    few = np.concatenate([np.arange(8, 100), np.arange(150, V - 1)])
    if n == 4864:
        ids = np.concatenate([np.full(3, 0), np.full(100, 3), np.full(200, 5), np.full(4400, 7), rs.choice(few, 159), np.full(2, V - 1)])
    else:
        ids = np.concatenate([np.full(2, V - 1), np.full(1, 0), np.full(n // 2, 7), rs.choice(few, n)])[:n]
    assert ids.size == n
    return rs.permutation(ids).astype(np.int64)


def _ints(rs, *shape):
    return torch.from_numpy(rs.randint(-4, 5, shape).astype(np.float32))


def _sum_by_id(ids, rows):
    """int64 [V, width]: the reference, with the value bound the exactness argument needs"""
    ref = torch.zeros(V, rows.shape[1], dtype=torch.int64).index_add_(0, torch.from_numpy(ids), rows.long())
    assert ref.abs().max().item() <= BOUND
    return ref


_cache = {}


def _case(dev, n, d):
    """(ids, dout fp32 on the host, int64 reference, sorted ids, order), made once per (n, d) and left unchanged"""
    from meant_amd import ops
    if (n, d) not in _cache:
        ids = _ids(n)
        dout = _ints(np.random.RandomState(1000 * n + d), n, d)
        _cache[(n, d)] = (ids, dout, _sum_by_id(ids, dout)) + tuple(ops._sort_ids(torch.from_numpy(ids).to(dev), V))
    return _cache[(n, d)]


def _sorted(dout, sorted_ids, order, dtab, lo=None, hi=None):
    from meant_amd import ops, _lib
    lib, p = _lib.lib, ops._p
    n, d = dout.shape
    dt = _lib.F32 if dout.dtype == torch.float32 else _lib.BF16
    if lo is None:
        _lib.check(lib.meant_embedding_bwd_sorted(p(dout), p(sorted_ids), p(order), p(dtab), n, d, V, dt, ops._stream()), "embedding_bwd_sorted")
    else:
        _lib.check(lib.meant_embedding_bwd_sorted_range(p(dout), p(sorted_ids), p(order), p(dtab), n, d, V, lo, hi, dt, ops._stream()),
                   "embedding_bwd_sorted_range")
    torch.cuda.synchronize()


def _seg(dout, sorted_ids, order, dtab, lo=0, hi=V):
    from meant_amd import ops, _lib
    lib, p = _lib.lib, ops._p
    n, d = dout.shape
    wsb = lib.meant_embedding_bwd_seg_ws(n, d)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dout.device)
    _lib.check(lib.meant_embedding_bwd_seg(p(dout), p(sorted_ids), p(order), p(dtab), n, d, V, lo, hi,
                                           _lib.F32 if dout.dtype == torch.float32 else _lib.BF16, p(ws), wsb, ops._stream()), "embedding_bwd_seg")
    torch.cuda.synchronize()


def _check_rows(got, ref, what):
    assert torch.equal(got.cpu(), ref.float()), what
    assert got[100:150].abs().max().item() == 0, what            # ids that never occur


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("det", [0, 1], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("n", NS)
def test_sorted_kernel_is_exact_on_integers(dev, option, n, det, dtype):
    option("deterministic", det)
    for d in (8, 520, 1024):
        ids, dout, ref, sorted_ids, order = _case(dev, n, d)
        got = torch.zeros(V, d, device=dev)
        _sorted(dout.to(dev).to(dtype), sorted_ids, order, got)
        _check_rows(got, ref, (n, d))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", NS)
def test_seg_kernels_are_exact_on_integers(dev, n, dtype):
    for d in (8, 520, 1024, 1032):
        ids, dout, ref, sorted_ids, order = _case(dev, n, d)
        got = torch.zeros(V, d, device=dev)
        _seg(dout.to(dev).to(dtype), sorted_ids, order, got)
        _check_rows(got, ref, (n, d))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", NS)
def test_row_slices_into_a_nonzero_table_equal_one_call(dev, n, dtype):
    """[id_lo, id_hi) cut as (0, 7), (7, 8), (8, V): the hot id alone in its slice; the table starts as integers and is accumulated into"""
    for entry, d in ((_sorted, 520), (_sorted, 1024), (_seg, 520), (_seg, 1032)):
        ids, dout, ref, sorted_ids, order = _case(dev, n, d)
        start = _ints(np.random.RandomState(d), V, d)
        x = dout.to(dev).to(dtype)
        one, many = start.to(dev), start.to(dev)
        entry(x, sorted_ids, order, one, 0, V)
        for lo, hi in ((0, 7), (7, 8), (8, V)):
            entry(x, sorted_ids, order, many, lo, hi)
        want = (ref + start.long()).float()
        assert torch.equal(one.cpu(), want), (entry.__name__, n, d)
        assert torch.equal(many.cpu(), want), (entry.__name__, n, d)


# ---- the by-id backward, exact through its GEMMs -------------------------------------------------------------------------------------
# V = 300, d = 256, H = 4 heads of 64.  The table image holds +1 / -1 and the gain is 1: a row's rms is exactly 1, eps = 1e-8 vanishes
# beside it in fp32 and the normed table, rounded to bf16, is the table image.  Then dW = dqkv^T table[ids] and db = colsum(dqkv) are
# integer sums, and the hi | lo images carry the per-id sums exactly, so both must come out exactly.  dtable and dgain pass through the
# norm backward and are no integers; the other suites hold them.  Key padding as in tests/test_gpu_qkv_by_id.py: rows 448 .. 511 (a
# 64-row block) and 512 .. 767 (a 256-row panel) are dead, their k | v columns NaN, which must never be read.
D_MODEL, HEADS = 256, 4
N3 = 3 * HEADS * 64


@pytest.mark.parametrize("T", [768, 4864])
def test_by_id_bias_and_weight_gradients_are_exact_on_integers(dev, T):
    from meant_amd import ops, _lib
    lib, p = _lib.lib, ops._p
    rs = np.random.RandomState(T)
    ids = _ids(T)
    table = torch.from_numpy(rs.choice([-1.0, 1.0], (V, D_MODEL)).astype(np.float32))
    dqkv, dres = _ints(rs, T, N3), _ints(rs, T, D_MODEL)
    live = torch.ones(T, dtype=torch.bool)
    live[448:768] = False
    dqkv_live = dqkv.clone()
    dqkv_live[~live, N3 // 3:] = 0
    D = _sum_by_id(ids, dqkv_live)
    want_db = dqkv_live.long().sum(0)
    want_dw = dqkv_live.long().t() @ table.long()[torch.from_numpy(ids)]
    assert torch.equal(want_dw, D.t() @ table.long())
    assert max(want_db.abs().max().item(), want_dw.abs().max().item()) <= BOUND

    mask = torch.ones(1, T, device=dev)
    mask[0, 448:768] = 0
    lists = ops.kv_live_rows(mask, False)
    assert lists[:3].tolist() == [T // 64 - 5, T // 256 - 1, 1]
    poisoned = dqkv.clone()
    poisoned[~live, N3 // 3:] = float("nan")
    bf = lambda a: a.to(dev).to(torch.bfloat16)
    x, tb, wT = bf(poisoned), bf(table), bf(_ints(rs, D_MODEL, N3))
    gain = torch.ones(D_MODEL, device=dev)
    sorted_ids, order = ops._sort_ids(torch.from_numpy(ids).to(dev), V)
    dw, db = torch.zeros(N3, D_MODEL, device=dev), torch.zeros(N3, device=dev)
    dgain, dtab = torch.empty(D_MODEL, device=dev), torch.zeros(V, D_MODEL, device=dev)
    wsb = lib.meant_qkv_embed_bwd_by_id_ws(T, D_MODEL, N3, V)
    ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
    _lib.check(lib.meant_qkv_embed_bwd_by_id(p(x), p(bf(dres)), p(sorted_ids), p(order), p(tb), p(gain), EPS, p(wT), p(lists), p(dw), p(db),
                                             p(dgain), p(dtab), T, D_MODEL, N3, V, 0, V, _lib.BY_ID_SHARED | _lib.BY_ID_TABLE, p(ws), wsb,
                                             ops._stream()), "qkv_embed_bwd_by_id")
    torch.cuda.synchronize()
    assert torch.equal(db.cpu(), want_db.float())
    assert torch.equal(dw.cpu(), want_dw.float())
    assert torch.isfinite(dtab).all() and torch.isfinite(dgain).all()
    assert dtab[100:150].abs().max().item() == 0                 # ids that never occur
