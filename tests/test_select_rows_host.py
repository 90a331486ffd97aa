"""Host-side facts of meant_select_rows (no GPU): the two symbols are in the header, the ctypes table and the built library; the
workspace size is host arithmetic and monotone in T; bad arguments come back with their status before anything is launched (the
pointers below are made-up addresses that are never dereferenced)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -4
SPAN = 1 << 40                                         # distance between the made-up buffers: far more than any T below needs


def _bufs():
    """target, idx, inv, target_sel, count, workspace: disjoint, aligned, never touched"""
    return [(i + 1) * SPAN for i in range(6)]


def _call(lib, T, V=100, ignore_index=-100, bufs=None, ws_bytes=None):
    tgt, idx, inv, tsel, count, ws = bufs or _bufs()
    if ws_bytes is None:
        ws_bytes = lib.meant_select_rows_ws(T)
    return lib.meant_select_rows(tgt, T, V, ignore_index, idx, inv, tsel, count, ws, ws_bytes, None)


def test_symbols_in_header_table_and_library():
    from meant_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "meant_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("meant_select_rows_ws", "meant_select_rows"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES
        assert re.search(r" T %s$" % name, out, flags=re.M), name
    _lib.route_reset()
    assert _lib.route_count("select_rows") == 0


def test_workspace_is_monotone_in_T():
    from meant_amd import _lib
    ws = _lib.lib.meant_select_rows_ws
    sizes = [ws(T) for T in (1, 63, 64, 65, 1023, 1024, 1025, 131072, 262143, 262144, 262145, 200003 * 64, (1 << 31) - 1)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert ws(0) == 0 and ws(-5) == 0 and ws(1 << 31) == 0       # what the call itself rejects


@pytest.mark.parametrize("T", [0, -1])
def test_rejects_empty_input(T):
    from meant_amd import _lib
    assert _call(_lib.lib, T, ws_bytes=1 << 20) == ERR_ARG
    assert b"select_rows" in _lib.lib.meant_last_error()


@pytest.mark.parametrize("which", range(5))
def test_rejects_null_pointers(which):
    from meant_amd import _lib
    bufs = _bufs()
    bufs[which] = None
    assert _call(_lib.lib, 4096, bufs=bufs) == ERR_ARG


@pytest.mark.parametrize("a,b", [(0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (1, 3), (2, 3), (1, 4), (3, 4), (0, 5), (3, 5)])
def test_rejects_overlapping_buffers(a, b):
    """buffer b starts inside buffer a (its last four bytes, or exactly on it)"""
    from meant_amd import _lib
    T = 4096
    length = [8 * T, 4 * T, 4 * T, 8 * T, 4, _lib.lib.meant_select_rows_ws(T)]
    for shift in (0, length[a] - 4):
        bufs = _bufs()
        bufs[b] = bufs[a] + shift
        assert _call(_lib.lib, T, bufs=bufs) == ERR_ARG, (a, b, shift)
        assert b"overlap" in _lib.lib.meant_last_error()
    bufs = _bufs()
    bufs[b] = bufs[a] + (length[a] + 7) // 8 * 8        # back to back is fine for the argument check; it stops at the workspace size
    assert _call(_lib.lib, T, bufs=bufs, ws_bytes=0) == ERR_WORKSPACE


def test_rejects_T_beyond_int32_before_any_launch():
    from meant_amd import _lib
    _lib.route_reset()
    assert _call(_lib.lib, 1 << 31, ws_bytes=1 << 30) == ERR_UNSUPPORTED
    assert _call(_lib.lib, (1 << 31) + 5, ws_bytes=1 << 30) == ERR_UNSUPPORTED
    assert _lib.route_count("select_rows") == 0


def test_rejects_short_or_missing_workspace():
    from meant_amd import _lib
    T = 200003
    need = _lib.lib.meant_select_rows_ws(T)
    assert _call(_lib.lib, T, ws_bytes=need - 1) == ERR_WORKSPACE
    bufs = _bufs()
    bufs[5] = None
    assert _call(_lib.lib, T, bufs=bufs, ws_bytes=need) == ERR_WORKSPACE
    assert _lib.route_count("select_rows") == 0


def test_padded_rows_rule():
    """the row count the head runs on: multiples of 8 below 1024 labelled rows, of 256 from there on, never zero"""
    from meant_amd import ops
    assert [ops.padded_rows(n) for n in (0, 1, 8, 9, 17, 1016, 1017, 1023)] == [8, 8, 8, 16, 24, 1016, 1024, 1024]
    assert [ops.padded_rows(n) for n in (1024, 1025, 4915, 5120)] == [1024, 1280, 5120, 5120]
