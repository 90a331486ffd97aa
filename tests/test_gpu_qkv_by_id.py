"""Option "qkv_by_id": the first text layer's backward (q|k|v projection, RMSNorm, embedding) once per vocabulary id
(meant_qkv_embed_bwd_by_id, ops.embed_qkv_attention) against the per-token route on the same inputs.

Shapes, the smallest that can still go wrong: V = 300 table rows (not a multiple of 64 or of the GEMMs' 256-row padding), d = 256
with 4 heads of 64 (and one case at d = 768 with 12 heads), T = 768 token rows = three stretches of the segmented sum.
Ids: id 7 on ~30 % of the tokens (a run that crosses two stretch ends), ids 0 and V - 1, ids 100 .. 149 never drawn, and ids outside
[0, V) that must be clamped as meant_embedding_fwd clamps them.
Key padding at the C ABI (rows as one run of 768 keys): rows 0 .. 447 live, the 64-row block 448 .. 511 dead, the 256-row panel
512 .. 767 dead; the by-id call gets NaN in the k | v columns of the dead rows, which it must never read.  At the model level (G = 3
sequences of S = 256): one unpadded sequence, one with a dead 64-key block, one with three.

The gradients are compared with an fp64 evaluation from the same bf16 operands (dqkv, dres, table image, W') and the fp32 gain; the
worst error of by-id, relative to the largest reference element, has to stay within twice that of the per-token route on the same
inputs -- the margin tests/test_gpu_kv_skip.py uses for a reordered reduction."""
import numpy as np
import pytest
import torch

from util import TOL

pytestmark = pytest.mark.gpu

V, S, G = 300, 256, 3
T = G * S
EPS = 1e-8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture()
def option():
    from meant_amd import _lib
    saved = {k: _lib.get_option(k) for k in ("qkv_by_id", "deterministic")}
    yield _lib.set_option
    for k, v in saved.items():
        _lib.set_option(k, v)


def _ids(rs):
    ids = rs.randint(0, V, T)
    ids[(ids >= 100) & (ids < 150)] += 100                   # 100 .. 149 never occur
    ids[rs.rand(T) < 0.3] = 7                                # the hot id
    ids[:4] = (0, V - 1, -5, V + 10)                         # the ends, and two ids to clamp (to 0 and V - 1)
    ids[-2:] = (V - 1, 0)
    return ids.astype(np.int64)


def _case(dev, d, H, seed=0):
    """every operand of the C-ABI comparison, made once per shape"""
    from meant_amd import ops
    rs = np.random.RandomState(seed)
    N3 = 3 * H * 64
    bf = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev).to(torch.bfloat16)
    c = dict(d=d, N3=N3)
    c["ids"] = torch.from_numpy(_ids(rs)).to(dev)
    c["tb"] = bf(rs.standard_normal((V, d)))
    c["gain"] = torch.from_numpy((1 + 0.2 * rs.standard_normal(d)).astype(np.float32)).to(dev)
    c["wT"] = bf(rs.standard_normal((d, N3)) / np.sqrt(d))
    c["dres"] = bf(rs.standard_normal((T, d)))
    dqkv = rs.standard_normal((T, N3))
    dqkv[c["ids"].cpu().numpy() == 7] += 0.5                 # the hot id's gradients agree in sign: its sum is large, its rounding coherent
    dqkv[448:, N3 // 3:] = 0                                 # k | v of the dead rows: exact zeros by the kv-skip contract
    c["dqkv"] = bf(dqkv)
    mask = torch.ones(1, T, device=dev)
    mask[0, 448:] = 0
    c["lists"] = ops.kv_live_rows(mask, False)
    assert c["lists"][:3].tolist() == [7, 2, 1]
    return c


def _by_id(c, parts=((0, V),), lists=True, poison=False):
    from meant_amd import ops, _lib
    lib, p = _lib.lib, ops._p
    d, N3 = c["d"], c["N3"]
    dev = c["ids"].device
    sorted_ids, order = ops._sort_ids(c["ids"], V)
    dqkv = c["dqkv"]
    if poison:
        dqkv = dqkv.clone()
        dqkv[448:, N3 // 3:] = float("nan")
    dw, db = torch.zeros(N3, d, device=dev), torch.zeros(N3, device=dev)
    dgain, dtab = torch.empty(d, device=dev), torch.zeros(V, d, device=dev)
    wsb = lib.meant_qkv_embed_bwd_by_id_ws(T, d, N3, V)
    ws = torch.empty(wsb, device=dev, dtype=torch.uint8)

    def call(lo, hi, stage):
        _lib.check(lib.meant_qkv_embed_bwd_by_id(p(dqkv), p(c["dres"]), p(sorted_ids), p(order), p(c["tb"]), p(c["gain"]), EPS, p(c["wT"]),
                                                 p(c["lists"]) if lists else None, p(dw), p(db), p(dgain), p(dtab), T, d, N3, V, lo, hi, stage,
                                                 p(ws), wsb, ops._stream()), "qkv_embed_bwd_by_id")
    if len(parts) == 1:
        call(*parts[0], _lib.BY_ID_SHARED | _lib.BY_ID_TABLE)
    else:
        call(0, 0, _lib.BY_ID_SHARED)
        for lo, hi in parts:
            call(lo, hi, _lib.BY_ID_TABLE)
    torch.cuda.synchronize()
    return dict(dw=dw, db=db, dgain=dgain, dtable=dtab)


def _per_token(c):
    """today's sequence on the same operands: dX GEMM, dW over q and over the live k|v rows, RMSNorm backward with the residual
    gradient, sorted embedding sum"""
    from meant_amd import ops, _lib
    lib, p = _lib.lib, ops._p
    d, N3 = c["d"], c["N3"]
    D = N3 // 3
    dev = c["ids"].device
    x = c["tb"][c["ids"].clamp(0, V - 1)].contiguous()
    n, sc, rinv = ops._rmsnorm_fwd_raw(x, c["gain"], EPS, 0.0, 0)
    dn = torch.empty(T, d, device=dev, dtype=torch.bfloat16)
    _lib.check(lib.meant_linear_bwd_dx(p(c["dqkv"]), N3, p(c["wT"]), p(dn), d, T, N3, d, _lib.BF16, ops._stream()), "linear_bwd_dx")
    dw, db = torch.zeros(N3, d, device=dev), torch.zeros(N3, device=dev)
    ops._bwd_dw(c["dqkv"][:, :D], n, dw[:D], db[:D])
    ops._bwd_dw_rows(c["dqkv"][:, D:], n, dw[D:], db[D:], c["lists"])
    dx, dgain = ops._rmsnorm_bwd_raw(dn, x, sc, rinv, EPS, 0.0, 0, dres=c["dres"])
    dtab = torch.zeros(V, d, device=dev)
    sorted_ids, order = ops._sort_ids(c["ids"], V)
    _lib.check(lib.meant_embedding_bwd_sorted(p(dx), p(sorted_ids), p(order), p(dtab), T, d, V, _lib.BF16, ops._stream()), "embedding_bwd_sorted")
    torch.cuda.synchronize()
    return dict(dw=dw, db=db, dgain=dgain, dtable=dtab)


def _fp64(c):
    d = c["d"]
    tab = c["tb"].double().cpu().requires_grad_()
    g = c["gain"].double().cpu().requires_grad_()
    W = c["wT"].double().cpu().t().contiguous().requires_grad_()
    b = torch.zeros(c["N3"], dtype=torch.float64, requires_grad=True)
    x = tab[c["ids"].cpu().clamp(0, V - 1)]
    n = g * x / (x.norm(dim=-1, keepdim=True) * d ** -0.5 + EPS)            # utils/rms_norm.py:40-57
    loss = ((n @ W.t() + b) * c["dqkv"].double().cpu()).sum() + (x * c["dres"].double().cpu()).sum()
    dW, db, dg, dt = torch.autograd.grad(loss, (W, b, g, tab))
    return dict(dw=dW, db=db, dgain=dg, dtable=dt)


def _err(got, ref):
    return {k: ((got[k].double().cpu() - ref[k]).abs().max() / ref[k].abs().max()).item() for k in ref}


_cache = {}


def _results(dev, d, H):
    """(case, by-id, per-token, fp64): computed once per shape and left unchanged"""
    if (d, H) not in _cache:
        c = _case(dev, d, H)
        _cache[(d, H)] = (c, _by_id(c, poison=True), _per_token(c), _fp64(c))
    return _cache[(d, H)]


@pytest.mark.parametrize("d,H", [(256, 4), (768, 12)], ids=["d256", "d768"])
def test_gradients_against_fp64_within_twice_the_per_token_error(dev, option, d, H):
    """measured on MI355X (profiles/qkv_by_id_errors.txt holds both routes' figures)"""
    from meant_amd import _lib
    option("deterministic", 0)
    _lib.route_reset()
    c, by_id, tok, ref = _results(dev, d, H)
    e_id, e_tok = _err(by_id, ref), _err(tok, ref)
    for k in ref:
        print(f"qkv_by_id d={d} {k}: by-id {e_id[k]:.3e} per-token {e_tok[k]:.3e}")
    for k in ref:
        assert torch.isfinite(by_id[k]).all(), k             # the NaNs in the dead k | v rows were never read
        assert e_id[k] <= 2 * e_tok[k], (k, e_id[k], e_tok[k])


def test_route_counter_counts_the_shared_stage(dev):
    from meant_amd import _lib
    c = _results(dev, 256, 4)[0]
    _lib.route_reset()
    _by_id(c)
    assert _lib.route_count("qkv_by_id") == 1
    _by_id(c, parts=((0, 100), (100, V)))
    assert _lib.route_count("qkv_by_id") == 2


def test_rows_of_unused_ids_are_exactly_zero(dev):
    c, by_id = _results(dev, 256, 4)[:2]
    used = torch.zeros(V, dtype=torch.bool)
    used[c["ids"].cpu().clamp(0, V - 1).unique()] = True
    assert (~used).sum() >= 50 and not used[100:150].any()
    assert by_id["dtable"][~used.to(dev)].abs().max().item() == 0
    assert by_id["dtable"][used.to(dev)].abs().amax(dim=1).min().item() > 0


def test_without_lists_every_row_is_read_and_the_sums_are_the_same(dev, option):
    """the dead rows' k | v are zeros: reading them adds nothing.  Deterministic, so that dW has one summation order"""
    option("deterministic", 1)
    c = _results(dev, 256, 4)[0]
    a, b = _by_id(c), _by_id(c, lists=False)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("det", [0, 1])
def test_row_slices_equal_one_call_bit_for_bit(dev, option, det):
    """dw goes through float atomics without the deterministic option (as meant_linear_bwd_dw's): the slices are compared on what
    the slicing touches (dtable, and dgain / db, which are ordered sums in either mode), dw as well under the option"""
    option("deterministic", det)
    c = _results(dev, 256, 4)[0]
    one = _by_id(c)
    for parts in (((0, 150), (150, V)), ((0, 7), (7, 8), (8, 299), (299, V)), ((0, V), (V, V))):
        many = _by_id(c, parts=parts)
        for k in ("dtable", "dgain", "db") + (("dw",) if det else ()):
            assert torch.equal(one[k], many[k]), (parts, k)


def test_two_deterministic_runs_are_bit_identical(dev, option):
    option("deterministic", 1)
    for d, H in ((256, 4), (768, 12)):
        c = _results(dev, d, H)[0]
        a, b = _by_id(c), _by_id(c)
        for k in a:
            assert torch.equal(a[k], b[k]), (d, k)


def test_op_forward_is_the_per_token_kernels_bit_for_bit(dev):
    """(o, x) of ops.embed_qkv_attention against ops.embedding -> rmsnorm_fork -> compose -> qkv_attention on the same parameters"""
    from meant_amd import ops
    import meant_amd.modules as mm
    torch.manual_seed(3)
    d, H = 256, 4
    enc = mm.languageEncoder(d, H).to(dev)
    table = torch.nn.Parameter(torch.randn(V, d, device=dev))
    ids = torch.from_numpy(_ids(np.random.RandomState(1))).to(dev).view(G, S)
    mask = _model_mask(dev)
    e, att = enc.encode, enc.encode[2]
    tables = att.xPos.tables(S, dev, ops.run_head_dim(att.Dh, torch.bfloat16))
    with torch.no_grad():
        x0 = ops.embedding(ids, table, torch.bfloat16)
        n0, _ = ops.rmsnorm_fork(x0, e[0].scale, e[0].eps)
        o0 = ops.qkv_attention(n0, att.q.weight, att.q.bias, att.v.weight, att.v.bias, att.k.weight, att.k.bias, tables, mask, True, H,
                               pre=(e[1].weight, e[1].bias))
        o1, x1 = mm._TokenIds(ids, table, torch.bfloat16).attend(e, mask)
    assert torch.equal(x0, x1) and torch.equal(o0, o1)


def _model_mask(dev):
    mask = torch.ones(G, S, device=dev)
    mask[1, S - 64:] = 0                                     # one dead 64-key block
    mask[2, S - 200:] = 0                                    # three dead blocks and a partly padded one
    return mask


def _model(cls, dev, d=256, H=4, embedding=None):
    import meant_amd as M
    torch.manual_seed(5)
    emb = embedding if embedding is not None else torch.nn.Embedding(V, d)
    if cls == "meant":
        m = M.meant(d, d, 4, 32, 64, 16, G, 3, emb, num_heads=H, num_encoders=2, channels=4)
    else:
        m = M.meant_tweet(d, 4, G, 3, emb, num_heads=H, num_encoders=2)
    m = m.to(dev).train()
    m.compute_dtype = torch.bfloat16
    rs = np.random.RandomState(8)
    ids = torch.from_numpy(_ids(rs)).to(dev).view(1, G, S)
    img = torch.from_numpy(rs.standard_normal((1, G, 4, 32, 64)).astype("float32")).to(dev)
    mask = _model_mask(dev).view(1, G, S)
    return m, ((ids, img, mask) if cls == "meant" else (ids, mask))


def _step(m, args, seed=77):
    m.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    out = m(*args)
    (out * torch.arange(1, out.numel() + 1, device=out.device).view_as(out)).sum().backward()
    torch.cuda.synchronize()
    return out.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("cls", ["meant", "meant_tweet"])
def test_model_train_mode_by_id_against_per_token(dev, option, cls):
    """option 0 / 2, one torch.manual_seed per arm: equal outputs (the forward is the same kernels), every parameter gradient within
    the bf16 tier's gradient-norm tolerance, and the route counter proves which arm ran what"""
    from meant_amd import _lib
    m, args = _model(cls, dev)
    res = []
    for opt, hits in ((0, 0), (2, 1)):
        option("qkv_by_id", opt)
        _lib.route_reset()
        res.append(_step(m, args))
        assert _lib.route_count("qkv_by_id") == hits, opt
    assert torch.equal(res[0][0], res[1][0])
    assert res[0][1].keys() == res[1][1].keys()
    big = max(g.norm().item() for g in res[0][1].values())
    tol = TOL[torch.bfloat16]["gnorm"]
    for k, g0 in res[0][1].items():
        g1 = res[1][1][k]
        assert torch.isfinite(g1).all(), k
        assert (g0 - g1).norm().item() <= tol * max(g0.norm().item(), 2e-2 * big), (k, (g0 - g1).norm().item(), g0.norm().item())


class _Wrapped(torch.nn.Module):
    """an embedding module that is not a plain nn.Embedding"""

    def __init__(self, d):
        super().__init__()
        self.inner = torch.nn.Embedding(V, d)

    def forward(self, ids):
        return self.inner(ids.clamp(0, V - 1))


@pytest.mark.parametrize("how", ["recompute", "module", "fp32", "auto_few_tokens"])
def test_route_not_taken(dev, option, how):
    """forced, the route still leaves layer 0 under recomputation, a non-nn.Embedding module and the fp32 tier alone; on automatic,
    T = 768 tokens on a table of V = 300 rows stay per token"""
    from meant_amd import _lib
    option("qkv_by_id", 1 if how == "auto_few_tokens" else 2)
    m, args = _model("meant" if how == "recompute" else "meant_tweet", dev, embedding=_Wrapped(256) if how == "module" else None)
    if how == "fp32":
        m.compute_dtype = torch.float32
    if how == "recompute":
        m.activation_checkpointing = True
    _lib.route_reset()
    _step(m, args)
    assert _lib.route_count("qkv_by_id") == 0


# ---- gradient sinks: the reducer's bucket views, whole and in row slices, and a tied table ------------------------------------------------
def _close(a, b, what):
    """two backward passes of one route: equal up to the float atomics of the dW sums and of the sorted embedding sum"""
    assert (a - b).abs().max().item() <= 1e-3 * max(b.abs().max().item(), 1e-6), what


def _reducer_step(m, args, red, seed=77):
    red.prepare()
    torch.manual_seed(seed)
    out = m(*args)
    (out * torch.arange(1, out.numel() + 1, device=out.device).view_as(out)).sum().backward()
    red.wait()
    torch.cuda.synchronize()
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("cls", ["meant", "meant_tweet"])
def test_model_under_a_gradient_reducer_whole_sink(dev, option, cls):
    """GradReducer(direct_grads=True) on a one-process run (one slice): the table's gradient goes into its bucket view through the sink
    and is reported once -- in `meant` from the language stream -- and every gradient equals the run without a reducer and, within the
    tier's tolerance, the per-token run under the same reducer"""
    from meant_amd import _lib
    from meant_amd.parallel import GradReducer
    m, args = _model(cls, dev)
    table = m.embedding[0].weight
    option("qkv_by_id", 2)
    plain = _step(m, args)[1]
    m.zero_grad(set_to_none=True)
    red = GradReducer(m.parameters(), bucket_mb=0.05, direct_grads=True)
    try:
        res = {}
        for opt in (2, 0):
            option("qkv_by_id", opt)
            _lib.route_reset()
            res[opt] = _reducer_step(m, args, red)
            assert _lib.route_count("qkv_by_id") == (1 if opt else 0)
            assert id(table) in red._reported                # delivered through the sink, not through autograd's accumulation
            assert red._owner[id(table)].pending == 0         # ... and counted exactly once
    finally:
        red.close()
        m.zero_grad(set_to_none=True)
    assert res[2].keys() == plain.keys()
    for k in plain:
        _close(res[2][k], plain[k], k)
    big = max(g.norm().item() for g in res[0].values())
    for k, g0 in res[0].items():
        assert (g0 - res[2][k]).norm().item() <= TOL[torch.bfloat16]["gnorm"] * max(g0.norm().item(), 2e-2 * big), k


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


@pytest.mark.parametrize("slices", [1, 3])
def test_model_table_gradient_into_a_sliced_sink(dev, option, slices):
    """the table's sink asks for `slices` row slices: the shared stage once, the table rows slice by slice into the sink's view, each
    slice reported in order; the view is the gradient of the run without a sink"""
    from meant_amd import ops, _lib
    option("qkv_by_id", 2)
    m, args = _model("meant_tweet", dev)
    table = m.embedding[0].weight
    plain = _step(m, args)[1]["embedding.0.weight"]
    view = torch.zeros(V, 256, device=dev)
    red = _StubReducer(slices)
    ops.grad_sinks[id(table)] = ops.GradSink(table, view, red)
    try:
        _lib.route_reset()
        _step(m, args)
        assert _lib.route_count("qkv_by_id") == 1
    finally:
        ops.grad_sinks.pop(id(table), None)
    assert table.grad is None
    if slices > 1:
        assert red.rows == [(V * c // slices, V * (c + 1) // slices, c == slices - 1) for c in range(slices)] and red.whole == 0
    else:
        assert red.rows == [] and red.whole == 1
    _close(view, plain, "table")


def test_tied_table_falls_back_to_the_returned_gradient(dev, option):
    """a table that a second kind of op reads in the same step (a vocabulary decoder tied to the word embedding) must not use its sink:
    the by-id backward returns the gradient, autograd adds both contributions, the reducer counts the parameter once"""
    from meant_amd import ops, _lib
    from meant_amd.parallel import GradReducer
    import meant_amd.modules as mm
    torch.manual_seed(3)
    d, H = 256, 4
    enc = mm.languageEncoder(d, H).to(dev)
    table = torch.nn.Parameter(torch.randn(V, d, device=dev))
    ids = torch.from_numpy(_ids(np.random.RandomState(1))).to(dev).view(G, S)
    mask = _model_mask(dev)
    params = [table] + list(enc.parameters())

    def run():
        o, x = mm._TokenIds(ids, table, torch.bfloat16).attend(enc.encode, mask)
        logits = ops.linear((o + x).view(G * S, d), table)   # the decoder reads the same parameter
        (logits.float() * 1e-2).sum().backward()
        torch.cuda.synchronize()

    _lib.route_reset()
    run()
    plain = table.grad.detach().clone()
    for p in params:
        p.grad = None
    red = GradReducer(params, bucket_mb=0.05, direct_grads=True)
    try:
        red.prepare()
        run()
        red.wait()
        torch.cuda.synchronize()
        assert _lib.route_count("qkv_by_id") == 2
        assert id(table) not in red._reported
        assert red._owner[id(table)].pending == 0
        _close(table.grad, plain, "tied table")
    finally:
        red.close()


_RCCL_SLICES = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.environ["MEANT_REPO"])
sys.path.insert(0, os.path.join(os.environ["MEANT_REPO"], "tests"))
torch.cuda.set_device(0)
dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
import test_gpu_qkv_by_id as T
from meant_amd import _lib
from meant_amd.parallel import GradReducer
dev = torch.device("cuda:0")
_lib.set_option("qkv_by_id", 2)
m, args = T._model("meant", dev)
table = m.embedding[0].weight
plain = T._step(m, args)[1]
m.zero_grad(set_to_none=True)
def sliced(slices):
    red = GradReducer(m.parameters(), bucket_mb=0.05, direct_grads=True, row_slices=slices)
    assert red.active
    red.row_slice_min_bytes = 0
    _lib.route_reset()
    g = T._reducer_step(m, args, red)
    n = len(red._owner[id(table)].slice_handles)
    assert _lib.route_count("qkv_by_id") == 1 and id(table) in red._reported
    red.close()
    m.zero_grad(set_to_none=True)
    return g, n
g3, n3 = sliced(3)
g1, n1 = sliced(1)
assert (n3, n1) == (3, 0), (n3, n1)
for k in plain:
    T._close(g3[k], plain[k], k)
    T._close(g1[k], plain[k], k)
dist.destroy_process_group()
print("RCCL_SLICES_OK")
"""


def test_model_table_gradient_in_row_slices_over_rccl_one_rank(dev):
    """the real call sequence of a data-parallel step on the by-id route -- the table alone in its bucket, its gradient delivered in three
    row slices from the language stream, one all-reduce per slice from the reducer's launch stream, joined in wait() -- on a one-rank
    group, in a child process so that the process group does not leak into the other tests (as tests/test_gpu_train.py does)"""
    import os
    import subprocess
    import sys
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29537", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MEANT_REDUCE_ALWAYS="1",
               MEANT_REPO=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", _RCCL_SLICES], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RCCL_SLICES_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
