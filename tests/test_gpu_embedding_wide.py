"""The embedding gradient at any width: meant_sort_ids (the stable device radix sort of the token ids) and meant_embedding_bwd_seg
(the segmented reduction without float atomics), through the raw C entry points and through ops.embedding.  References: torch.sort
(stable) and torch.nn.functional.embedding's backward on the CPU, with the tolerances of test_embedding_backward_sorted_path."""
import numpy as np
import pytest
import torch

from tests.util import DTYPES, IDS, t, assert_grad_close, pair, compare_param_grads

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _tol(dtype):
    return 1e-5 if dtype == torch.float32 else 2e-3


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _raw_sort(ids_dev, V):
    """meant_sort_ids through ctypes; the outputs start as -1 so that a slot nobody wrote shows"""
    from meant_amd import _lib
    lib = _lib.lib
    n = ids_dev.numel()
    sorted_ids = torch.full((n,), -1, dtype=torch.int64, device=ids_dev.device)
    order = torch.full((n,), -1, dtype=torch.int64, device=ids_dev.device)
    wsb = lib.meant_sort_ids_ws(n, V)
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=ids_dev.device)
    _lib.check(lib.meant_sort_ids(ids_dev.data_ptr(), n, V, sorted_ids.data_ptr(), order.data_ptr(), ws.data_ptr(), wsb, _stream()), "sort_ids")
    torch.cuda.synchronize()
    return sorted_ids, order


def _raw_seg(dout, sorted_ids, order, dtab, V, lo, hi):
    from meant_amd import _lib
    lib = _lib.lib
    n, d = dout.shape
    wsb = lib.meant_embedding_bwd_seg_ws(n, d)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dout.device)
    _lib.check(lib.meant_embedding_bwd_seg(dout.data_ptr(), sorted_ids.data_ptr(), order.data_ptr(), dtab.data_ptr(), n, d, V, lo, hi,
                                           F32 if dout.dtype == torch.float32 else BF16, ws.data_ptr(), wsb, _stream()), "embedding_bwd_seg")
    torch.cuda.synchronize()


def _sort_inputs(n, V, kind):
    g = torch.Generator().manual_seed(n * 7 + V % 1000 + len(kind))
    if kind == "random":
        return torch.randint(0, V, (n,), generator=g)
    if kind == "equal":
        return torch.full((n,), V // 2, dtype=torch.int64)
    if kind == "sorted":
        return torch.sort(torch.randint(0, V, (n,), generator=g)).values
    if kind == "reversed":
        return torch.sort(torch.randint(0, V, (n,), generator=g), descending=True).values
    assert kind == "outside"                                    # ids below 0 and at / above V: clamped as the forward clamps
    return torch.randint(-V // 2 - 3, V + V // 2 + 3, (n,), generator=g)


@pytest.mark.parametrize("V", [2, 300, 64001, 70000, 2**31 - 1])   # one, two, two, three and four digit passes
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099, 70001])
def test_sort_ids_matches_stable_torch_sort(dev, n, V):
    from meant_amd import _lib
    for kind in ("random", "equal", "sorted", "reversed", "outside"):
        ids = _sort_inputs(n, V, kind)
        want_ids, want_order = torch.sort(ids.clamp(0, V - 1), stable=True)
        before = _lib.route_count("sort_ids")
        got_ids, got_order = _raw_sort(ids.to(dev), V)
        assert _lib.route_count("sort_ids") == before + 1
        assert torch.equal(got_ids.cpu(), want_ids), (kind, n, V)
        assert torch.equal(got_order.cpu(), want_order), (kind, n, V)


def test_sort_ids_limits(dev):
    from meant_amd import _lib
    lib = _lib.lib
    x, a, b = (torch.zeros(8, dtype=torch.int64, device=dev) for _ in range(3))
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=dev)
    rc = lib.meant_sort_ids(x.data_ptr(), 8, 2**31, a.data_ptr(), b.data_ptr(), ws.data_ptr(), 1 << 16, _stream())
    assert rc == -2                                             # MEANT_ERR_UNSUPPORTED
    for outs in ((x, b), (a, x), (a, a)):                       # not in place, and two different outputs
        rc = lib.meant_sort_ids(x.data_ptr(), 8, 300, outs[0].data_ptr(), outs[1].data_ptr(), ws.data_ptr(), 1 << 16, _stream())
        assert rc == -1                                         # MEANT_ERR_ARG
    dout = torch.zeros(8, 12, device=dev)
    rc = lib.meant_embedding_bwd_seg(dout.data_ptr(), a.data_ptr(), b.data_ptr(), dout.data_ptr(), 8, 12, 4, 0, 4, F32, ws.data_ptr(), 1 << 16,
                                     _stream())
    assert rc == -2                                             # d % 8 != 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d", [8, 768])
def test_embedding_backward_seg_narrow_raw(dev, dtype, d):
    """the raw entry point at widths of one column block (d = 768: 96 chunks, d = 8: one chunk, one lane), fed by meant_sort_ids;
    the same sorted ids also drive the sorted kernel (meant_embedding_bwd_sorted), which reads the same layout"""
    from meant_amd import _lib
    V, B, S = 300, 3, 2048
    table, ids, ge = _case(V, d, B, S)
    want = _reference(table, ids, ge, dtype)
    dout = ge.view(-1, d).to(dev).to(dtype).contiguous()
    sorted_ids, order = _raw_sort(ids.view(-1).to(dev), V)
    seg = _lib.route_count("emb_seg")
    got = torch.zeros(V, d, device=dev)
    _raw_seg(dout, sorted_ids, order, got, V, 0, V)
    assert _lib.route_count("emb_seg") == seg + 1
    assert_grad_close(got, want, _tol(dtype), "d embedding (raw, narrow)")
    assert torch.equal(got.cpu() == 0, want == 0)
    again = torch.zeros(V, d, device=dev)
    _raw_seg(dout, sorted_ids, order, again, V, 0, V)
    assert torch.equal(again, got)
    old = torch.zeros(V, d, device=dev)
    _lib.check(_lib.lib.meant_embedding_bwd_sorted(dout.data_ptr(), sorted_ids.data_ptr(), order.data_ptr(), old.data_ptr(), B * S, d, V,
                                                   F32 if dtype == torch.float32 else BF16, _stream()), "embedding_bwd_sorted")
    torch.cuda.synchronize()
    assert_grad_close(old, want, _tol(dtype), "d embedding (sorted kernel on meant_sort_ids output)")


def _case(V, d, B, S):
    g = torch.Generator().manual_seed(3)
    table = torch.randn(V, d, generator=g)
    ids = torch.randint(0, V, (B, S), generator=g)
    ids[0, :1500] = 7                                           # a hot run over several stretches and more than one workgroup
    ge = torch.randn(B, S, d, generator=g)
    return table, ids, ge


def _reference(table, ids, ge, dtype):
    tr = table.clone().requires_grad_()
    torch.nn.functional.embedding(ids, tr).backward(ge.to(dtype).float())
    return tr.grad


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("V,d,B,S", [(300, 1032, 3, 2048), (64, 2048, 2, 4099), (5000, 1544, 1, 5003), (50, 4104, 1, 4100)])
def test_embedding_backward_wide(dev, dtype, V, d, B, S):
    """widths above the sorted kernel's 1024 take the device sort and the segmented reduction: a hot id, ids that occur once or never,
    token counts that are no multiple of the stretch, one to five column blocks"""
    from meant_amd import ops, _lib
    table, ids, ge = _case(V, d, B, S)
    th = table.to(dev).requires_grad_()
    seg, srt = _lib.route_count("emb_seg"), _lib.route_count("sort_ids")
    ops.embedding(ids.to(dev), th, dtype).backward(ge.to(dev).to(dtype))
    assert _lib.route_count("emb_seg") > seg and _lib.route_count("sort_ids") > srt
    want = _reference(table, ids, ge, dtype)
    assert_grad_close(th.grad, want, _tol(dtype), "d embedding (wide)")
    assert th.grad[8:].abs().sum() > 0 and torch.equal(th.grad.cpu() == 0, want == 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d", [768, 2048])
def test_embedding_backward_deterministic_is_bit_identical(dev, dtype, d):
    from meant_amd import ops, _lib
    V, B, S = 300, 3, 2048
    table, ids, ge = _case(V, d, B, S)
    want = _reference(table, ids, ge, dtype)
    prev = _lib.get_option("deterministic")
    _lib.set_option("deterministic", 1)
    try:
        grads = []
        for _ in range(2):
            t2 = table.to(dev).requires_grad_()
            ops.embedding(ids.to(dev), t2, dtype).backward(ge.to(dev).to(dtype))
            grads.append(t2.grad.clone())
    finally:
        _lib.set_option("deterministic", prev)
    assert torch.equal(grads[0], grads[1])
    for gr in grads:
        assert_grad_close(gr, want, _tol(dtype), "d embedding (deterministic)")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_embedding_backward_seg_row_slices_and_accumulate(dev, dtype):
    """the raw entry point: four id ranges that do not divide V = 301 evenly, into one zeroed table, equal one call bit for bit; and a
    table of ones comes back as ones plus the gradient"""
    V, d, B, S = 301, 1032, 2, 2500
    table, ids, ge = _case(V, d, B, S)
    want = _reference(table, ids, ge, dtype)
    dout = ge.view(-1, d).to(dev).to(dtype).contiguous()
    sorted_ids, order = _raw_sort(ids.view(-1).to(dev), V)
    whole = torch.zeros(V, d, device=dev)
    _raw_seg(dout, sorted_ids, order, whole, V, 0, V)
    assert_grad_close(whole, want, _tol(dtype), "d embedding (raw, whole)")
    assert torch.equal(whole.cpu() == 0, want == 0)
    sliced = torch.zeros(V, d, device=dev)
    for c in range(4):
        _raw_seg(dout, sorted_ids, order, sliced, V, V * c // 4, V * (c + 1) // 4)
    assert torch.equal(sliced, whole)
    ones = torch.ones(V, d, device=dev)
    _raw_seg(dout, sorted_ids, order, ones, V, 0, V)
    assert torch.equal(ones, whole + 1.0)                       # every row is one add of its sum to what was there


def test_embedding_backward_few_tokens_route(dev):
    """n = 100 at d = 2048: the atomics kernel as before, unless option "deterministic" asks for ordered sums"""
    from meant_amd import ops, _lib
    V, d = 40, 2048
    g = torch.Generator().manual_seed(5)
    table = torch.randn(V, d, generator=g)
    ids = torch.randint(0, V, (1, 100), generator=g)
    ge = torch.randn(1, 100, d, generator=g)
    want = _reference(table, ids, ge, torch.float32)
    th = table.to(dev).requires_grad_()
    seg = _lib.route_count("emb_seg")
    ops.embedding(ids.to(dev), th, torch.float32).backward(ge.to(dev))
    assert _lib.route_count("emb_seg") == seg
    assert_grad_close(th.grad, want, 1e-5, "d embedding (few tokens)")
    prev = _lib.get_option("deterministic")
    _lib.set_option("deterministic", 1)
    try:
        t2 = table.to(dev).requires_grad_()
        ops.embedding(ids.to(dev), t2, torch.float32).backward(ge.to(dev))
        assert _lib.route_count("emb_seg") == seg + 1
    finally:
        _lib.set_option("deterministic", prev)
    assert_grad_close(t2.grad, want, 1e-5, "d embedding (few tokens, deterministic)")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_meant_text_1280_embedding_gradient(dev, dtype):
    """meant(text_dim=1280) at lag 2, S = 16 under option "deterministic" (64 tokens): the table's gradient comes from the segmented
    reduction and agrees with the CPU oracle like every other parameter's"""
    import meant_amd
    from meant_amd import _lib
    from oracle import meant_oracle as O
    args, kw = (1280, 320, 4, 32, 32, 16, 2, 3), dict(num_heads=20, num_encoders=1, channels=4)
    ref, hip = pair(O.meant(*args, torch.nn.Embedding(100, 1280), **kw), meant_amd.meant(*args, torch.nn.Embedding(100, 1280), **kw), 1234, dev)
    r = np.random.RandomState(11)
    ids = t(r.randint(0, 100, (2, 2, 16)).astype("int64"))
    ids[0, 0, :9] = 1                                           # padding-like repeats
    img = t(r.standard_normal((2, 2, 4, 32, 32)).astype("float32"))
    mask = torch.ones(2, 2, 16)
    mask[1, :, 11:] = 0
    tgt = torch.tensor([2, 0])
    torch.nn.functional.cross_entropy(ref(ids, img, mask), tgt).backward()
    hip.compute_dtype = dtype
    prev = _lib.get_option("deterministic")
    _lib.set_option("deterministic", 1)
    try:
        seg = _lib.route_count("emb_seg")
        torch.nn.functional.cross_entropy(hip(ids.to(dev), img.to(dev), mask.to(dev)), tgt.to(dev)).backward()
        torch.cuda.synchronize()
        assert _lib.route_count("emb_seg") > seg
    finally:
        _lib.set_option("deterministic", prev)
    compare_param_grads(ref, hip, dtype, "meant_text_1280")
    from tests.util import TOL
    gw, rw = hip.embedding[0].weight.grad, ref.embedding[0].weight.grad
    assert rw is not None and rw.abs().max() > 0
    assert_grad_close(gw, rw, TOL[dtype]["gelem"], "meant_text_1280: embedding table")


class _StubReducer:
    """stands in for a GradReducer: asks for the table's gradient in `slices` row slices and records what is reported"""

    def __init__(self, slices):
        self.slices, self.rows, self.whole = slices, [], 0

    def _row_slices(self, p):
        return self.slices

    def _sink_report_rows(self, p, lo, hi, last):
        self.rows.append((lo, hi, last))

    def _sink_report(self, p):
        self.whole += 1


@pytest.mark.parametrize("slices", [1, 4])
def test_embedding_backward_wide_into_a_gradient_sink(dev, slices):
    """ops.embedding at d > 1024 with a gradient sink: the rows are added straight into the sink's view (pre-filled with ones), in one
    call or in four id ranges with one workspace, each range reported; same bits as the gradient autograd returns without a sink"""
    from meant_amd import ops, _lib
    V, d, B, S = 301, 1032, 2, 2500
    table, ids, ge = _case(V, d, B, S)
    t0 = table.to(dev).requires_grad_()
    ops.embedding(ids.to(dev), t0, torch.bfloat16).backward(ge.to(dev).to(torch.bfloat16))
    th = table.to(dev).requires_grad_()
    view = torch.ones(V, d, device=dev)
    red = _StubReducer(slices)
    ops.grad_sinks[id(th)] = ops.GradSink(th, view, red)
    try:
        seg = _lib.route_count("emb_seg")
        ops.embedding(ids.to(dev), th, torch.bfloat16).backward(ge.to(dev).to(torch.bfloat16))
        torch.cuda.synchronize()
        assert _lib.route_count("emb_seg") == seg + slices
    finally:
        ops.grad_sinks.pop(id(th), None)
    assert th.grad is None
    if slices > 1:
        assert red.rows == [(V * c // 4, V * (c + 1) // 4, c == 3) for c in range(4)] and red.whole == 0
    else:
        assert red.rows == [] and red.whole == 1
    assert torch.equal(view, t0.grad + 1.0)
