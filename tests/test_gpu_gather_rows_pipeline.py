"""meant_gather_rows in its 16-byte form at the row counts where a wave's share of the rows changes: 1 .. 9 rows and the first count at
which a wave of the largest grid (8192 blocks of four waves) takes a second row (4 * 8192 + 1); widths of one chunk, of a lane's second
chunk half filled (768) and of a chunk more (776); indices with repeats, -1 (zeros) and -2 (the fill row, or zeros without one).
Compared with torch.equal against index_select.  The cases hold for any row-to-wave map of the kernel."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BLOCKS = 8192                                                # the launcher's largest grid, four waves to a block
SRC_ROWS = 37


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _gather(src, idx, fill, n, W):
    from meant_amd import _lib, ops
    dst = torch.full((n, W), 7.0, device=src.device, dtype=src.dtype)
    _lib.check(_lib.lib.meant_gather_rows(src.data_ptr(), idx.data_ptr(), fill.data_ptr() if fill is not None else None, dst.data_ptr(), n, W,
                                          _lib.F32 if src.dtype == torch.float32 else _lib.BF16, ops._stream()), "gather_rows")
    torch.cuda.synchronize()
    return dst


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("W", [8, 768, 776])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 7, 8, 9, 4 * BLOCKS + 1])
def test_gather_rows_against_index_select(dev, dtype, W, n):
    g = torch.Generator().manual_seed(n + W)
    src = torch.randn(SRC_ROWS, W, generator=g).to(dtype).to(dev)
    fill = torch.randn(W, generator=g).to(dtype).to(dev)
    idx = torch.randint(0, SRC_ROWS, (n,), generator=g, dtype=torch.int32)          # repeats: n rows out of 37
    idx[::5] = -1
    idx[2::7] = -2
    if n > 1:
        idx[n - 1] = SRC_ROWS - 1
    idx = idx.to(dev)
    for f in (fill, None):
        table = torch.cat([src, torch.zeros(1, W, device=dev, dtype=dtype), (f if f is not None else torch.zeros_like(fill)).view(1, W)])
        want = table.index_select(0, torch.where(idx >= 0, idx, SRC_ROWS - 1 - idx).long())     # -1 -> the zero row, -2 -> the fill row
        assert torch.equal(_gather(src, idx, f, n, W), want), "fill" if f is not None else "no fill"
