"""Host-side facts of "TimeSformer at any width and any video length" (no GPU): the bounds, workspace sizes and refusals of the
class-token attention over key segments, and the argument checks of the entries that now take any width -- all decided before any
launch, on pointers that are never dereferenced."""
import pytest

ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -4
LDS_FLOATS = (160 * 1024 - 1024) // 4


def _max_len(Dh, arrays):
    return (LDS_FLOATS - 4 - (256 // (Dh // 8)) * Dh) // arrays


@pytest.mark.parametrize("Dh", [8, 32, 64, 96, 256])
def test_cls_max_len_is_the_one_workgroup_bound(Dh):
    from meant_amd import _lib
    lib = _lib.lib
    assert lib.meant_attn_cls_max_len(Dh, 0) == _max_len(Dh, 1) and lib.meant_attn_cls_max_len(Dh, 1) == _max_len(Dh, 2)
    assert lib.meant_attn_cls_max_len(100, 0) == 0 and lib.meant_attn_cls_max_len(264, 1) == 0
    # the old entries refuse one key past it, as they always have
    L = _max_len(Dh, 1) + 1
    assert lib.meant_attn_cls_fwd(16, 32, 2 * Dh, 48, None, 2, L, 2, Dh, 0.1, _lib.F32, None) == ERR_UNSUPPORTED


def test_split_segment_count_workspace_and_refusals():
    from meant_amd import _lib
    lib = _lib.lib
    B, H, Dh = 2, 2, 64
    big = 1 << 24

    def fwd(L, nseg, wsb=big):
        return lib.meant_attn_cls_split_fwd(16, 32, H * Dh, 48, None, B, L, H, Dh, 0.1, nseg, _lib.F32, 64, wsb, None)

    def bwd(L, nseg, wsb=big):
        return lib.meant_attn_cls_split_bwd(16, 32, H * Dh, 48, H * Dh, 64, None, 80, B, L, H, Dh, 0.1, nseg, _lib.F32, 96, wsb, None)
    mf, mb = _max_len(Dh, 1), _max_len(Dh, 2)
    for L, nseg in ((mf + 1, 1), (2 * mf + 1, 2)):
        assert fwd(L, nseg) == ERR_UNSUPPORTED and b"attn_cls_split_fwd" in lib.meant_last_error()
    for L, nseg in ((mb + 1, 1), (2 * mb + 1, 2)):
        assert bwd(L, nseg) == ERR_UNSUPPORTED
    for L, nseg in ((5, 6), (5, -1), (0, 0), (1 << 31, 0)):
        assert fwd(L, nseg) == ERR_ARG and bwd(L, nseg) == ERR_ARG
    for L, nseg in ((5, 2), (257, 7), (mb + 1, 2)):
        wsb = lib.meant_attn_cls_split_ws(B, L, H, Dh, nseg)
        assert wsb == B * H * nseg * (Dh + 2) * 4
        assert fwd(L, nseg, wsb - 1) == ERR_WORKSPACE and bwd(L, nseg, wsb - 1) == ERR_WORKSPACE
    # nseg = 0: the smallest count that fits, the backward's (the larger) sizing the workspace
    for L, segs in ((mb, 1), (mb + 1, 2), (2 * mb, 2), (2 * mb + 1, 3), (100001, 6)):
        assert lib.meant_attn_cls_split_ws(B, L, H, Dh, 0) == B * H * segs * (Dh + 2) * 4, L
    assert fwd(2 * mf + 1, 0, B * H * 3 * (Dh + 2) * 4 - 1) == ERR_WORKSPACE          # three forward segments
    assert lib.meant_attn_cls_split_ws(B, 5, H, Dh, 6) == 0 and lib.meant_attn_cls_split_ws(B, 5, H, 100, 1) == 0
    assert lib.meant_attn_cls_split_fwd(16, 32, H * 100, 48, None, B, 5, H, 100, 0.1, 1, _lib.F32, 64, big, None) == ERR_UNSUPPORTED
    assert lib.meant_attn_cls_split_fwd(16, 32, H * Dh, 48, None, B, 5, H, Dh, 0.1, 1, 7, 64, big, None) == ERR_ARG      # unknown dtype
    assert lib.meant_attn_cls_split_fwd(16, 32, H * Dh, 48, None, B, 5, H, Dh, 0.1, 1, _lib.F32, 68, big, None) == ERR_ARG   # workspace alignment


def test_any_width_entries_reject_bad_geometry_and_alignment():
    """widths off the 8-grid pass the argument checks with element-aligned pointers only; a pointer off its element, a width of 0 and
    d < 3 for the shift are refused; multiples of 8 keep the 16-byte rule"""
    from meant_amd import _lib
    lib = _lib.lib
    F32, BF16 = _lib.F32, _lib.BF16
    assert lib.meant_gather_rows(16, 32, None, 48, 4, 0, F32, None) == ERR_ARG
    assert lib.meant_gather_rows(18, 32, None, 48, 4, 99, F32, None) == ERR_ARG and b"element alignment" in lib.meant_last_error()
    assert lib.meant_gather_rows(17, 32, None, 48, 4, 99, BF16, None) == ERR_ARG
    assert lib.meant_gather_rows(20, 32, None, 48, 4, 96, F32, None) == ERR_ARG and b"16-byte" in lib.meant_last_error()
    assert lib.meant_token_shift(16, 32, 1, 1, 1, 2, 0, F32, None) == ERR_ARG
    assert lib.meant_token_shift(18, 32, 1, 1, 1, 99, 0, F32, None) == ERR_ARG
    assert lib.meant_token_shift(20, 32, 1, 1, 1, 96, 0, F32, None) == ERR_ARG and b"16-byte" in lib.meant_last_error()
    assert lib.meant_dropout(16, 32, 0, 0.1, 1, F32, None) == ERR_ARG
    assert lib.meant_dropout(18, 32, 7, 0.1, 1, F32, None) == ERR_ARG and lib.meant_dropout(16, 32, 7, 1.0, 1, F32, None) == ERR_ARG
    assert lib.meant_dropout(20, 32, 8, 0.1, 1, F32, None) == ERR_ARG and b"16-byte" in lib.meant_last_error()
    assert lib.meant_geglu_fwd(16, 32, 4, 0, F32, None) == ERR_ARG and lib.meant_geglu_fwd(17, 32, 4, 99, BF16, None) == ERR_ARG
    assert lib.meant_geglu_bwd(16, 32, 50, 4, 99, F32, None) == ERR_ARG
    assert lib.meant_geglu_fwd(18, 32, 0, 99, BF16, None) == 0 and lib.meant_geglu_bwd(16, 32, 48, 0, 99, F32, None) == 0   # no rows: nothing to launch
    assert _lib.route_count("attn_cls_split") >= 0 and _lib.route_count("rows_elem") >= 0
