"""Host-side facts of the K-tail Linear path (no GPU): the two route counters exist and start at zero, and the copy kernel's entry
point rejects shapes that would make it read or write outside its operands before anything is launched."""
import pytest


def test_k_tail_route_counters_exist():
    from meant_amd import _lib
    _lib.route_reset()
    assert _lib.route_count("nt128k") == 0 and _lib.route_count("nt256k") == 0
    with pytest.raises(KeyError):
        _lib.route_count("nt512k")


@pytest.mark.parametrize("ld_src,cols_src,ld_dst,cols_dst,rows", [(7, 8, 8, 8, 4), (8, 8, 7, 8, 4), (8, 0, 8, 8, 4), (8, 8, 8, 0, 4), (8, 8, 8, 8, 0)])
def test_pad_copy2d_rejects_bad_geometry(ld_src, cols_src, ld_dst, cols_dst, rows):
    from meant_amd import _lib
    rc = _lib.lib.meant_pad_copy2d(16, ld_src, cols_src, _lib.F32, 32, ld_dst, cols_dst, _lib.F32, rows, None)   # never dereferenced
    assert rc != 0 and b"pad_copy2d" in _lib.lib.meant_last_error()
