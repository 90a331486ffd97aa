"""The sorted-id stretch walk (seg_walk of csrc/seg_sum.h) with its rows in flight in two register sets of four, through
meant_embedding_bwd_sorted_range on bf16 rows.  D = 8 rows are on their way at most, so the id lists are built to put a run's first
and last row into every slot of the two sets and across the 64-entry blocks and the 256-entry stretches:
  ladder    run lengths 1, 2, ..., 2 D + 1 following each other, again and again
  one       one id for all n: the run spans every stretch
  distinct  every id once
  outside   the ladder with ids below 0 and at / above V among them (sorted by a stable host sort: the library's sort would clamp them)
  range     the ladder, summed for the ids of a range cut out of the middle third of the sorted list only (the range's ends fall
            inside a stretch and a set, the runs next to them are dropped at the flush), and then for the rest in two more calls
Under option "deterministic" the result is compared bit for bit with a float32 sum taken row by row in the order the library's own
sort returns (a run starts from 0 and is added to the zeroed table once); under the default option, where the runs that cross a
stretch end go through float atomics, with a float64 sum within the bound of tests/test_gpu_embedding_wide.py (2e-3 of the largest
element for bf16 rows)."""
import numpy as np
import pytest
import torch

from tests.util import assert_grad_close

pytestmark = pytest.mark.gpu

V, D_FLIGHT, BF16 = 2000, 8, 1
KINDS = ("ladder", "one", "distinct", "outside", "range")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ids(kind, n):
    if kind == "one":
        return np.full(n, 11, dtype=np.int64)
    if kind == "distinct":
        return np.random.RandomState(n).permutation(V)[:n].astype(np.int64)
    lengths = np.tile(np.arange(1, 2 * D_FLIGHT + 2), n // 100 + 2)
    ids = np.repeat(3 + 5 * np.arange(len(lengths)), lengths)[:n].astype(np.int64)
    assert ids.max() < V
    if kind == "outside":
        ids[::7] = -3
        ids[3::11] = V
        ids[5::13] = V + 40
    return np.random.RandomState(n + 1).permutation(ids)     # the tokens come in any order; the sort makes the runs


def _sorted(kind, ids, dev):
    from meant_amd import ops
    if kind == "outside":
        s = torch.sort(torch.from_numpy(ids), stable=True)
        return s.values.to(dev), s.indices.to(dev)
    return ops._sort_ids(torch.from_numpy(ids).to(dev), V)


def _run(dout, sorted_ids, order, ranges, det):
    from meant_amd import _lib, ops
    n, d = dout.shape
    dtab = torch.zeros(V, d, device=dout.device)
    prev = _lib.get_option("deterministic")
    _lib.set_option("deterministic", det)
    try:
        for lo, hi in ranges:
            _lib.check(_lib.lib.meant_embedding_bwd_sorted_range(dout.data_ptr(), sorted_ids.data_ptr(), order.data_ptr(), dtab.data_ptr(), n, d, V,
                                                                 lo, hi, BF16, ops._stream()), "embedding_bwd_sorted_range")
        torch.cuda.synchronize()
    finally:
        _lib.set_option("deterministic", prev)
    return dtab.cpu()


def _reference(rows, sorted_ids, order, lo, hi):
    """(float32 in sorted order, float64) sums of the rows of the ids of [lo, hi) inside [0, V)"""
    f32 = np.zeros((V, rows.shape[1]), dtype=np.float32)
    f64 = np.zeros((V, rows.shape[1]), dtype=np.float64)
    for i, r in zip(sorted_ids, order):
        if 0 <= i < V and lo <= i < hi:
            f32[i] = f32[i] + rows[r]
            f64[i] += rows[r]
    return torch.from_numpy(f32), torch.from_numpy(f64)


@pytest.mark.parametrize("d", [8, 768, 1024])
@pytest.mark.parametrize("n", [1, 5, 255, 256, 257, 511, 513, 1027])
def test_sorted_sum_on_constructed_id_lists(dev, n, d):
    rs = np.random.RandomState(n * 3 + d)
    dout = torch.from_numpy(rs.standard_normal((n, d)).astype(np.float32)).to(torch.bfloat16)
    rows = dout.float().numpy()
    dout = dout.to(dev)
    for kind in KINDS:
        ids = _ids(kind, n)
        sorted_ids, order = _sorted(kind, ids, dev)
        s_np, o_np = sorted_ids.cpu().numpy(), order.cpu().numpy()
        assert np.array_equal(ids[o_np], s_np)
        # the cut is taken from the ids that occur, so that both of its ends fall inside the sorted list (inside a stretch, a 64-entry
        # block and a set of four rows, between two runs): the runs below, inside and above it are all there from three ids on
        cut = (int(s_np[n // 3]), max(int(s_np[2 * n // 3]), int(s_np[n // 3]) + 1))
        if kind == "range" and len(np.unique(s_np)) >= 3:
            inside = int(((s_np >= cut[0]) & (s_np < cut[1])).sum())
            assert 0 < inside < n and s_np[0] < cut[0] and s_np[-1] >= cut[1], (n, cut, inside)
        ranges = ((0, V),) if kind != "range" else (cut,)
        want32, want64 = _reference(rows, s_np, o_np, *ranges[0])
        got = _run(dout, sorted_ids, order, ranges, 1)
        assert torch.equal(got, want32), (kind, "deterministic")
        got = _run(dout, sorted_ids, order, ranges, 0)
        assert torch.equal(got == 0, want64 == 0), (kind, "rows of ids that are absent or outside the range stay zero")
        if want64.abs().max() > 0:
            assert_grad_close(got, want64, 2e-3, f"{kind}, default option")
        if kind == "range":                                  # the rest of the table in two more calls: the union is the whole sum
            want32, want64 = _reference(rows, s_np, o_np, 0, V)
            parts = (cut, (0, cut[0]), (cut[1], V))
            assert torch.equal(_run(dout, sorted_ids, order, parts, 1), want32), "three id ranges, deterministic"
            assert_grad_close(_run(dout, sorted_ids, order, parts, 0), want64, 2e-3, "three id ranges, default option")
