"""Host-side facts of attention at any head count (no GPU): the head dims ops.qkv_attention and the TimeSformer pad to, and that
rotary tables padded to ceil8(R) with identity columns rotate to the same bits as the unpadded ones."""
import pytest
import torch

# what ops._padded_head_dim answered for every multiple of 8 up to 256 before heads off the 8-grid were padded: native dims stay,
# the others go to 128 below 128 and to the next native dim above
NATIVE = (64, 96, 128, 160, 192, 256)
MULT8 = {d: (None if d in NATIVE else 128 if d < 128 else next(n for n in NATIVE if n > d)) for d in range(8, 257, 8)}
OFF_GRID = {29: 64, 76: 96, 100: 128, 172: 192, 1: 64, 20: 64, 63: 64, 65: 96, 97: 128, 129: 160, 161: 192, 193: 256, 255: 256}


def test_padded_head_dim_table():
    from meant_amd import ops
    for d, want in MULT8.items():
        assert ops._padded_head_dim(d) == want, d
    for d, want in OFF_GRID.items():
        assert ops._padded_head_dim(d) == want, d
    assert ops._padded_head_dim(257) is None and ops._padded_head_dim(264) is None
    # every head dim up to 256 ends on a native dim that holds it
    for d in range(1, 257):
        p = ops._padded_head_dim(d) or d
        assert p in NATIVE and p >= d, d


def test_run_and_divided_head_dims():
    from meant_amd import ops
    bf, f32 = torch.bfloat16, torch.float32
    assert [ops.run_head_dim(d, bf) for d in (20, 40, 64, 76, 172)] == [64, 128, 64, 96, 192]
    assert [ops.run_head_dim(d, f32) for d in (20, 40, 64, 76, 172)] == [20, 40, 64, 76, 172]
    # TimeSformer: multiples of 8 run as they are in both tiers; the others at a native dim (bf16) or ceil8 (fp32)
    assert [ops.divided_head_dim(d, bf) for d in (12, 20, 50, 40, 64, 72)] == [64, 64, 64, 40, 64, 72]
    assert [ops.divided_head_dim(d, f32) for d in (12, 20, 50, 40, 64, 72)] == [16, 24, 56, 40, 64, 72]


def _tables(S, R, xpos, seed):
    g = torch.Generator().manual_seed(seed)
    ang = torch.repeat_interleave(torch.arange(S, dtype=torch.float32)[:, None] * torch.rand(R // 2, generator=g)[None, :], 2, dim=-1)
    cos, sin = ang.cos(), ang.sin()
    if not xpos:
        return (cos, sin, cos, sin)
    s = (0.9 + 0.2 * torch.rand(S, R, generator=g))
    return (cos * s, sin * s, cos / s, sin / s)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("Dh,R,xpos", [(8, 6, False), (24, 20, False), (40, 20, False), (64, 14, False), (96, 38, True), (192, 86, False),
                                       (128, 50, True), (64, 50, False)])
def test_padded_tables_rotate_to_the_same_bits(Dh, R, xpos, dtype):
    from meant_amd import ops
    from meant_amd.modules import _rotate_pairs
    G, S, H = 2, 5, 3
    tabs = _tables(S, R, xpos, 100 * Dh + R)
    padded = ops.pad_rotary_tables(tabs, Dh)
    R8 = (R + 7) & ~7
    assert all(p.shape == (S, R8) and p.is_contiguous() for p in padded)
    for i, (p, u) in enumerate(zip(padded, tabs)):
        assert torch.equal(p[:, :R], u)
        assert torch.equal(p[:, R:], torch.full((S, R8 - R), 1.0 if i % 2 == 0 else 0.0))
    assert (padded[0] is padded[2]) == (tabs[0] is tabs[2]) and (padded[1] is padded[3]) == (tabs[1] is tabs[3])
    x = torch.randn(G, S, H, Dh, generator=torch.Generator().manual_seed(R)).to(dtype)
    for (a, b), (ap, bp) in (((tabs[0], tabs[1]), (padded[0], padded[1])), ((tabs[2], tabs[3]), (padded[2], padded[3]))):
        want, got = _rotate_pairs(x, a, b), _rotate_pairs(x, ap, bp)
        assert want.dtype == got.dtype == dtype
        assert torch.equal(want.view(torch.int32 if dtype == torch.float32 else torch.int16),
                           got.view(torch.int32 if dtype == torch.float32 else torch.int16))


def test_tables_are_left_alone_without_room():
    from meant_amd import ops
    tabs = _tables(4, 14, False, 1)
    assert ops.pad_rotary_tables(tabs, 14) is tabs          # ceil8(14) = 16 columns do not fit a head of 14
    assert ops.pad_rotary_tables(tabs, 29) is tabs          # a head off the 8-grid runs the pair-by-pair rotary: no use for padding
    t16 = _tables(4, 16, False, 2)
    assert ops.pad_rotary_tables(t16, 64) is t16            # on the grid already
    assert ops.pad_rotary_tables(None, 64) is None


def test_rotary_embedding_caches_the_padded_tables():
    from meant_amd.modules import RotaryEmbedding
    rot = RotaryEmbedding(dim=10, freqs_for="pixel")        # visionEncoder(40, 2): R = 10
    plain = rot.tables(5, "cpu")
    padded = rot.tables(5, "cpu", head_dim=64)
    assert plain[0].shape == (5, 10) and padded[0].shape == (5, 16)
    assert rot.tables(5, "cpu", head_dim=64) is padded and rot.tables(5, "cpu") is plain
    assert rot.tables(5, "cpu", head_dim=20) is plain       # fp32 tier at Dh = 20: no room on the 8-grid, nothing padded
    rot48 = RotaryEmbedding(dim=48, use_xpos=True)
    t = rot48.tables(7, "cpu")
    assert rot48.tables(7, "cpu", head_dim=96) is t         # R = 48 is on the grid
