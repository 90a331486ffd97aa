"""The two kernels that move whole token rows by vocabulary id around the first text layer -- qkv_gather_kernel (the forward's gather,
two register sets of tokens in flight) and qkv_seg_kernel (the backward's sum by id: seg_walk with two sets of four rows in flight)
-- at the route's smallest admitted shape, the one of tests/test_gpu_qkv_fwd_by_id.py: V = 4100 table rows, 12 sequences of 512
tokens, 12 heads of 64 (N3 = 2304), R = 48, its pad lengths.  The id lists are built to put a run's first and last token into
every slot of the sets and across the 64-entry blocks and the 256-entry stretches: run lengths 1, 2, ..., 17 following each other
(`ladder`), one id on every token (`one`), and as many distinct ids as the table has (`distinct`).
Op level, ops.embed_qkv_attention, option "deterministic" on, with the forward bit of option kv_skip on and off:
  qkv_fwd_by_id 0 against 2 (qkv_by_id = 2 in both): the packed projection, the outputs and every gradient with torch.equal
C ABI, meant_qkv_embed_bwd_by_id against the per-token sequence on the same id lists, with and without the key-padding lists: the two
routes' gradients are different sums by design and cannot be compared bit for bit (ops.embed_qkv_attention is the by-id node itself),
so they are held to the check of tests/test_gpu_qkv_by_id.py: against fp64, the by-id error within twice the per-token route's.  What
can be bit for bit is: lists against no lists, one call against row slices, two runs (all under "deterministic"), and the bias gradient
against a host float32 sum taken in the order of qkv_seg_kernel's walk."""
import numpy as np
import pytest
import torch

from tests.test_gpu_qkv_fwd_by_id import V, S, G, D_MODEL, DH, R, T, PADS, EPS, _mask

pytestmark = pytest.mark.gpu

H = 12


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ids(kind):
    if kind == "one":
        return np.full(T, 9, dtype=np.int64)
    if kind == "distinct":
        return (np.random.RandomState(1).permutation(T) % V).astype(np.int64)    # every id once or twice, the whole table used
    lengths = np.tile(np.arange(1, 18), T // 153 + 1)
    ids = np.repeat((7 * np.arange(len(lengths))) % V, lengths)[:T].astype(np.int64)
    return np.random.RandomState(2).permutation(ids)


_cache = {}


def _operands(dev, kind):
    if kind not in _cache:
        rs = np.random.RandomState(len(kind))
        N3 = 3 * H * DH
        f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dev)
        _cache[kind] = dict(
            ids=torch.from_numpy(_ids(kind)).to(dev).view(G, S),
            table=f(rs.standard_normal((V, D_MODEL))), gain=f(1 + 0.2 * rs.standard_normal(D_MODEL)),
            w=f(rs.standard_normal((N3, D_MODEL)) / np.sqrt(D_MODEL)), b=f(0.1 * rs.standard_normal(N3)),
            tables=tuple(f(rs.uniform(-1, 1, (S, R))) for _ in range(4)), mask=_mask(dev, PADS),
            do=f(rs.standard_normal((G, S, H * DH))).to(torch.bfloat16), dx=f(rs.standard_normal((G, S, D_MODEL))).to(torch.bfloat16))
    return _cache[kind]


def _op(dev, kind, fwd_opt, bwd_opt):
    """one forward + backward of the node under the two options: (qkv, o, lse, x), gradients, route hits"""
    from meant_amd import ops, _lib
    c = _operands(dev, kind)
    saved_opts = {k: _lib.get_option(k) for k in ("qkv_by_id", "qkv_fwd_by_id", "deterministic")}
    _lib.set_option("qkv_by_id", bwd_opt)
    _lib.set_option("qkv_fwd_by_id", fwd_opt)
    _lib.set_option("deterministic", 1)
    leaves = {k: c[k].clone().requires_grad_() for k in ("table", "gain", "w", "b")}
    saved = {}
    orig = ops._attn_fwd_raw

    def spy(qkv, *a, **k):                                   # the packed projection as the attention core reads it
        o, lse = orig(qkv, *a, **k)
        saved.update(qkv=qkv, lse=lse)
        return o, lse
    ops._attn_fwd_raw = spy
    try:
        _lib.route_reset()
        o, x = ops.embed_qkv_attention(c["ids"], leaves["table"], leaves["gain"], EPS, leaves["w"], leaves["b"], c["tables"], c["mask"], True, H)
        torch.autograd.backward((o, x), (c["do"], c["dx"]))
        torch.cuda.synchronize()
        hits = {r: _lib.route_count(r) for r in ("qkv_fwd_by_id", "qkv_by_id")}
    finally:
        ops._attn_fwd_raw = orig
        for k, v in saved_opts.items():
            _lib.set_option(k, v)
    return dict(qkv=saved["qkv"], o=o.detach(), lse=saved["lse"], x=x.detach()), {k: v.grad for k, v in leaves.items()}, hits


@pytest.fixture(params=[3, 1], ids=["kv_skip_on", "kv_skip_forward_off"])
def kv_skip(request):
    from meant_amd import _lib
    saved = _lib.get_option("kv_skip")
    _lib.set_option("kv_skip", request.param)
    yield request.param
    _lib.set_option("kv_skip", saved)


@pytest.mark.parametrize("kind", ["ladder", "one", "distinct"])
def test_forward_by_id_equals_per_token_bit_for_bit(dev, kv_skip, kind):
    from meant_amd import _lib
    if _lib.lib.meant_qkv_embed_fwd_by_id_ok(T, D_MODEL, 3 * H * DH, V) != 1:
        pytest.fail(f"the test's shape does not reach the streaming kernel on this part ({_lib.lib.meant_num_cus()} CUs)")
    f0, g0, h0 = _op(dev, kind, 0, 2)
    f2, g2, h2 = _op(dev, kind, 2, 2)
    assert h0["qkv_fwd_by_id"] == 0 and h2["qkv_fwd_by_id"] == 1
    for k in f0:
        assert torch.equal(f0[k], f2[k]), k
    for k in g0:
        assert torch.isfinite(g2[k]).all() and torch.equal(g0[k], g2[k]), k


def _abi_case(dev, kind):
    """the operands of meant_qkv_embed_bwd_by_id at the C ABI, as tests/test_gpu_qkv_by_id.py lays them out: the rows as one run of T keys"""
    from meant_amd import ops
    if ("abi", kind) not in _cache:
        rs = np.random.RandomState(10 + len(kind))
        N3 = 3 * H * DH
        bf = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev).to(torch.bfloat16)
        c = dict(d=D_MODEL, N3=N3, ids=torch.from_numpy(_ids(kind)).to(dev))
        c["tb"] = bf(rs.standard_normal((V, D_MODEL)))
        c["gain"] = torch.from_numpy((1 + 0.2 * rs.standard_normal(D_MODEL)).astype(np.float32)).to(dev)
        c["wT"] = bf(rs.standard_normal((D_MODEL, N3)) / np.sqrt(D_MODEL))
        c["dres"] = bf(rs.standard_normal((T, D_MODEL)))
        mask = _mask(dev, PADS).view(1, T)
        dead = (mask.view(-1, 64).sum(1) == 0).repeat_interleave(64).cpu().numpy()
        dqkv = rs.standard_normal((T, N3))
        dqkv[dead, N3 // 3:] = 0                             # k | v of the dead 64-row blocks: exact zeros by the kv-skip contract
        c["dqkv"] = bf(dqkv)
        c["lists"] = ops.kv_live_rows(mask, False)
        _cache[("abi", kind)] = c
    return _cache[("abi", kind)]


@pytest.mark.parametrize("lists", [True, False], ids=["kv_skip_on", "kv_skip_off"])
@pytest.mark.parametrize("kind", ["ladder", "one", "distinct"])
def test_backward_by_id_against_fp64_within_twice_the_per_token_error(dev, monkeypatch, kind, lists):
    """qkv_by_id's two routes at the C ABI on the constructed id lists, with the reference, the per-token sequence and the bound of
    tests/test_gpu_qkv_by_id.py (its helpers, at this file's shape): the gradients of the two routes are different sums by design, so
    they meet in fp64, the by-id error within twice the per-token route's.  With and without the key-padding lists."""
    from tests import test_gpu_qkv_by_id as B
    from meant_amd import _lib
    monkeypatch.setattr(B, "V", V)
    monkeypatch.setattr(B, "T", T)
    c = _abi_case(dev, kind)
    saved = _lib.get_option("deterministic")
    _lib.set_option("deterministic", 0)
    try:
        _lib.route_reset()
        by_id = B._by_id(c, parts=((0, V),), lists=lists)
        assert _lib.route_count("qkv_by_id") == 1
        if ("ref", kind) not in _cache:
            _cache[("ref", kind)] = (B._per_token(c), B._fp64(c))
        tok, ref = _cache[("ref", kind)]
    finally:
        _lib.set_option("deterministic", saved)
    e_id, e_tok = B._err(by_id, ref), B._err(tok, ref)
    for k in ref:
        print(f"by-id rows {kind} lists={lists} {k}: by-id {e_id[k]:.3e} per-token {e_tok[k]:.3e}")
    for k in ref:
        assert torch.isfinite(by_id[k]).all(), k
        assert e_id[k] <= 2 * e_tok[k], (k, e_id[k], e_tok[k])


def _db_in_walk_order(c):
    """db as the library sums it, in float32 on the host: the column sums of each stretch of 256 sorted entries, row after row in sorted
    order (qkv_seg_kernel's walk), then 16 equal pieces of the stretch axis summed in order and added as a binary tree (qkv_colsum_kernel)"""
    from meant_amd import ops
    _, order = ops._sort_ids(c["ids"], V)
    rows = c["dqkv"].float().cpu().numpy()[order.cpu().numpy()]
    nst = (T + 255) // 256
    cpart = np.zeros((nst, rows.shape[1]), dtype=np.float32)
    for j in range(T):
        cpart[j // 256] = cpart[j // 256] + rows[j]
    piece = (nst + 15) // 16
    red = np.zeros((16, rows.shape[1]), dtype=np.float32)
    for p in range(16):
        for k in range(p * piece, min(p * piece + piece, nst)):
            red[p] = red[p] + cpart[k]
    for h in (8, 4, 2, 1):
        for p in range(h):
            red[p] = red[p] + red[p + h]
    return torch.from_numpy(red[0])


@pytest.mark.parametrize("kind", ["ladder", "one", "distinct"])
def test_backward_by_id_bit_for_bit(dev, monkeypatch, kind):
    """what of meant_qkv_embed_bwd_by_id can be held bit for bit on the constructed id lists, under option "deterministic" (dw then has
    one summation order): with the key-padding lists against without (the dead rows' k | v are zeros: the walk's per-lane live flags
    must drop exactly those chunks), one call against row slices whose ends are ids that occur, two runs, and the bias gradient against
    a host float32 sum in the walk's order (the column sums of qkv_seg_kernel: a shifted flag or a row added out of turn shows here)"""
    from tests import test_gpu_qkv_by_id as B
    from meant_amd import _lib
    monkeypatch.setattr(B, "V", V)
    monkeypatch.setattr(B, "T", T)
    c = _abi_case(dev, kind)
    saved = _lib.get_option("deterministic")
    _lib.set_option("deterministic", 1)
    try:
        one = B._by_id(c, parts=((0, V),), lists=True)
        again = B._by_id(c, parts=((0, V),), lists=True)
        no_lists = B._by_id(c, parts=((0, V),), lists=False)
        present = np.unique(_ids(kind))
        mid = int(present[len(present) // 2])
        sliced = B._by_id(c, parts=((0, mid), (mid, mid + 1), (mid + 1, V)), lists=True)
    finally:
        _lib.set_option("deterministic", saved)
    for k in one:
        assert torch.isfinite(one[k]).all(), k
        assert torch.equal(one[k], again[k]), ("two runs", k)
        assert torch.equal(one[k], no_lists[k]), ("lists against no lists", k)
        assert torch.equal(one[k], sliced[k]), ("one call against three row slices", k)
    assert torch.equal(one["db"].cpu(), _db_in_walk_order(c)), "db against the host sum in the walk's order"
