"""Host-side rules of the embedding gradient's routes (no GPU): which shapes take the segmented reduction, that the sorted kernel's
predicate kept its meaning, the workspace arithmetic of the two new entry points, the route names."""
import pytest


@pytest.fixture()
def deterministic():
    from meant_amd import _lib
    prev = _lib.get_option("deterministic")

    def set_(v):
        _lib.set_option("deterministic", v)
    yield set_
    _lib.set_option("deterministic", prev)


def test_seg_predicate_and_routes(deterministic):
    from meant_amd import ops
    deterministic(0)
    assert ops._emb_seg_bwd_ok(786432, 2048) and ops._emb_seg_bwd_ok(786432, 1280) and ops._emb_seg_bwd_ok(4096, 768)
    assert not ops._emb_seg_bwd_ok(786432, 772)
    assert not ops._emb_seg_bwd_ok(4095, 2048)
    assert ops._emb_bwd_route(786432, 2048) == "seg" and ops._emb_bwd_route(786432, 1032) == "seg"
    assert ops._emb_bwd_route(786432, 768) == "sorted" and ops._emb_bwd_route(786432, 1024) == "sorted"   # the default route is unchanged
    assert ops._emb_bwd_route(4095, 2048) == "atomic" and ops._emb_bwd_route(786432, 772) == "atomic"
    deterministic(1)
    assert ops._emb_seg_bwd_ok(4095, 2048) and ops._emb_seg_bwd_ok(100, 768)
    assert not ops._emb_seg_bwd_ok(100, 772)
    assert ops._emb_bwd_route(100, 2048) == "seg"
    assert ops._emb_bwd_route(786432, 768) == "sorted" and ops._emb_bwd_route(100, 768) == "sorted"   # the follow-the-run branch stays
    assert ops._emb_bwd_route(100, 772) == "atomic"


def test_sorted_predicate_is_unchanged(deterministic):
    from meant_amd import ops
    deterministic(0)
    assert ops._emb_sorted_bwd_ok(786432, 768) and ops._emb_sorted_bwd_ok(4096, 768)
    assert not ops._emb_sorted_bwd_ok(4095, 768)
    assert not ops._emb_sorted_bwd_ok(786432, 2048) and not ops._emb_sorted_bwd_ok(786432, 772)
    deterministic(1)
    assert ops._emb_sorted_bwd_ok(4095, 768) and not ops._emb_sorted_bwd_ok(4095, 2048)


def test_workspace_sizes_are_host_arithmetic():
    from meant_amd import _lib
    lib = _lib.lib
    last = 0
    for n in (1, 255, 2048, 2049, 4099, 70001, 786432, 2**31 - 1):
        w = lib.meant_sort_ids_ws(n, 64001)
        assert w > 0 and w >= last
        last = w
    assert lib.meant_sort_ids_ws(786432, 2) < lib.meant_sort_ids_ws(786432, 64001) < lib.meant_sort_ids_ws(786432, 70000)   # 0, 1, 2 buffers
    assert lib.meant_sort_ids_ws(786432, 70000) == lib.meant_sort_ids_ws(786432, 2**31 - 1)
    assert lib.meant_sort_ids_ws(2**31, 64001) == 0 and lib.meant_sort_ids_ws(8, 2**31) == 0                               # unsupported
    last = 0
    for n in (1, 256, 257, 4099, 786432):
        w = lib.meant_embedding_bwd_seg_ws(n, 2048)
        assert w > 0 and w >= last and w % 16 == 0
        last = w
    assert lib.meant_embedding_bwd_seg_ws(786432, 2048) == 3072 * 2 * 2048 * 4 + 3072 * 4   # [stretch][first | last][d] floats, then one int per stretch
    assert lib.meant_embedding_bwd_seg_ws(786432, 1280) < lib.meant_embedding_bwd_seg_ws(786432, 2048)


def test_route_names_are_known():
    from meant_amd import _lib
    assert _lib.route_count("emb_seg") >= 0 and _lib.route_count("sort_ids") >= 0
    with pytest.raises(KeyError):
        _lib.route_count("emb_segx")
