"""Option "kv_skip": the GEMMs around a key-masked bf16 attention leave out the token rows of padded key blocks -- the rows whose K / V
the attention kernels never read and whose dK / dV they write as exact zeros (csrc/attn_bf16.hip, key_tile_skippable).

Shape: G = 24 sequences of S = 512 tokens, d = 768, 12 heads, bf16: M = 12288 token rows = 48 row panels of 256, the smallest M at
which the N = 1536 and N = 768 launches of the projection take the streaming GEMM.  Every comparison runs the same inputs with the
option on and off in one process:
  * the live-row lists equal a numpy evaluation of the rule on the mask;
  * qkv out of the projection is bit-equal on q and on every live k|v row, and exactly zero on the k|v rows of dead panels;
  * o and dx are bit-equal (nothing they are made of changes; the rows left out add exact zeros);
  * dw / db against an fp64 product of the very bf16 operands the kernels read (dqkv, captured, and x): only the order of the fp32
    sums differs between on and off, so the worst error of `on`, relative to the largest reference element, stays within twice that of
    `off` on the same inputs.  fp32 sums of ~12288 bf16 products land near 1e-6 relative to the largest element either way; the
    factor 2 is the room two different summation orders need (no figure measured from the code went into it).
The masks cover every count of dead 64-key blocks per sequence from 0 to 7 (mask "sweep" has each of them)."""
import numpy as np
import pytest
import torch

from util import TOL

pytestmark = pytest.mark.gpu

G, S, D_MODEL, HEADS = 24, 512, 768, 12
PADS_B = (0, 1, 63, 64, 65, 255, 256, 257, 383, 448)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _trailing(pads, n=G, s=S):
    m = np.ones((n, s), dtype=np.float32)
    for g in range(n):
        p = pads[g % len(pads)]
        if p:
            m[g, s - p:] = 0
    return m


def _mask(name):
    if name == "none":                                       # (a) no padding: the lists are full
        return np.ones((G, S), dtype=np.float32)
    if name == "trailing":                                   # (b)
        return _trailing(PADS_B)
    if name == "trailing_plus":                              # (c) (b) + one sequence padded entirely + one with key 0 padded
        m = _trailing(PADS_B)
        m[5, :] = 0
        m[8, 0] = 0                                          # sequence 8 has 383 trailing pads: dead blocks that a causal run must keep
        return m
    if name == "hole":                                       # (d) 128 padded keys in the middle: two whole blocks, or one and two halves
        m = np.ones((G, S), dtype=np.float32)
        for g in range(G):
            lo = 192 if g % 2 == 0 else 200
            m[g, lo:lo + 128] = 0
        return m
    if name == "upper_half":                                 # (e) the maximum: every upper half dead
        return _trailing((256,))
    if name == "sweep":                                      # 0 .. 7 dead blocks per sequence
        return _trailing(tuple(64 * i for i in range(8)))
    raise KeyError(name)


def _dead_blocks(mask, causal):
    """the rule of key_tile_skippable on a 0 / 1 mask: [G, S / 64] bool"""
    g, s = mask.shape
    dead = (mask.reshape(g, s // 64, 64) == 0).all(axis=2)
    has_live = (mask[:, 0] == 1) if causal else (mask == 1).any(axis=1)
    return dead & has_live[:, None]


def _expected_lists(mask, causal):
    dead = _dead_blocks(mask, causal).reshape(-1)
    blocks = np.nonzero(~dead)[0]
    pdead = dead.reshape(-1, 4).all(axis=1)
    P, Q = mask.shape[1] // 256, mask.shape[0]
    walk = [q * P + r for r in range(P) for q in range(Q)]   # panels of one position range after the other
    return blocks, np.array([p for p in walk if not pdead[p]], dtype=np.int64), np.array([p for p in walk if pdead[p]], dtype=np.int64)


CASES = [("none", True), ("trailing", True), ("trailing_plus", True), ("hole", True), ("upper_half", True), ("sweep", True),
         ("none", False), ("trailing", False), ("trailing_plus", False), ("hole", False), ("upper_half", False), ("sweep", False)]
IDS = [f"{n}-{'causal' if c else 'full'}" for n, c in CASES]


def test_masks_cover_every_dead_block_count():
    seen = set()
    for name, causal in CASES:
        seen |= set(_dead_blocks(_mask(name), causal).sum(axis=1).tolist())
    assert seen >= set(range(8)), seen
    assert _dead_blocks(_mask("trailing_plus"), True)[[5, 8]].sum() == 0      # nothing of those two may be skipped under the causal mask
    assert _dead_blocks(_mask("trailing_plus"), False)[5].sum() == 0 and _dead_blocks(_mask("trailing_plus"), False)[8].sum() == 5


@pytest.mark.parametrize("name,causal", CASES, ids=IDS)
def test_live_row_lists_equal_the_rule_on_the_mask(dev, name, causal):
    from meant_amd import ops
    mask = _mask(name)
    lists = ops.kv_live_rows(torch.from_numpy(mask).to(dev), causal).cpu().numpy()
    blocks, panels, dead = _expected_lists(mask, causal)
    nblk, npan = G * S // 64, G * S // 256
    hdr = ops.KV_LIST_HEADER
    assert lists[:3].tolist() == [len(blocks), len(panels), len(dead)]
    assert np.array_equal(lists[hdr:hdr + len(blocks)], blocks)
    assert np.array_equal(lists[hdr + nblk:hdr + nblk + len(panels)], panels)
    assert np.array_equal(lists[hdr + nblk + npan:hdr + nblk + npan + len(dead)], dead)


def test_live_row_lists_of_one_long_sequence(dev):
    """more blocks than the compaction has threads, panels of four position ranges, nothing a multiple of anything"""
    from meant_amd import ops
    g, s = 70, 1024
    rs = np.random.RandomState(3)
    mask = _trailing(tuple(int(v) for v in rs.randint(0, 1000, 37)), g, s)
    mask[11, 0] = 0
    for causal in (True, False):
        lists = ops.kv_live_rows(torch.from_numpy(mask).to(dev), causal).cpu().numpy()
        blocks, panels, dead = _expected_lists(mask, causal)
        nblk, npan, hdr = g * s // 64, g * s // 256, ops.KV_LIST_HEADER
        assert lists[:3].tolist() == [len(blocks), len(panels), len(dead)]
        assert np.array_equal(lists[hdr:hdr + len(blocks)], blocks)
        assert np.array_equal(lists[hdr + nblk:hdr + nblk + len(panels)], panels)
        assert np.array_equal(lists[hdr + nblk + npan:hdr + nblk + npan + len(dead)], dead)


@pytest.fixture(scope="module")
def operands(dev):
    import meant_amd
    gen = torch.Generator().manual_seed(2024)
    x = (torch.randn(G, S, D_MODEL, generator=gen)).to(dev).to(torch.bfloat16)
    w = (torch.randn(3 * D_MODEL, D_MODEL, generator=gen) / D_MODEL ** 0.5).to(dev)
    b = (torch.randn(3 * D_MODEL, generator=gen) * 0.1).to(dev)
    do = torch.randn(G, S, D_MODEL, generator=gen).to(dev).to(torch.bfloat16)
    tables = meant_amd.RotaryEmbedding(dim=48, use_xpos=True).tables(S, dev)
    return x, w, b, do, tables


def _run(operands, mask, causal, kv_skip, monkeypatch):
    """one forward + backward of the fused op under `kv_skip`: (o, dx, dw, db, dqkv as the weight-gradient GEMMs saw it)"""
    from meant_amd import _lib, ops
    x, w, b, do, tables = operands
    seen = []
    plain, rows = ops._bwd_dw, ops._bwd_dw_rows
    monkeypatch.setattr(ops, "_bwd_dw", lambda dy, *a: (seen.append(dy), plain(dy, *a))[1])
    monkeypatch.setattr(ops, "_bwd_dw_rows", lambda dy, *a: (seen.append(dy), rows(dy, *a))[1])
    old = _lib.get_option("kv_skip")
    _lib.set_option("kv_skip", kv_skip)
    try:
        xg, wg, bg = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
        o = ops._QKVAttention.apply(xg, wg, bg, tables, mask, causal, HEADS)
        o.backward(do)
        torch.cuda.synchronize()
    finally:
        _lib.set_option("kv_skip", old)
        monkeypatch.undo()
    dqkv = seen[0]._base if seen[0]._base is not None else seen[0]            # the column slices are views of the one dqkv
    assert dqkv.shape == (G * S, 3 * D_MODEL)
    return o.detach(), xg.grad, wg.grad, bg.grad, dqkv.detach()


@pytest.mark.parametrize("name,causal", CASES, ids=IDS)
def test_projection_leaves_out_dead_panels_only(dev, operands, name, causal):
    """meant_qkv_proj_fwd_live with the lists against meant_qkv_proj_fwd at the C ABI: two streaming launches (q over all panels, k|v
    over the live ones) and the zero fill"""
    from meant_amd import _lib, ops
    from meant_amd._lib import lib, check, BF16
    x, w, b, _, (qa, qb, ka, kb) = operands
    np_mask = _mask(name)
    lists = ops.kv_live_rows(torch.from_numpy(np_mask).to(dev), causal)
    M, N, Dh = G * S, 3 * D_MODEL, D_MODEL // HEADS
    wc = w.to(torch.bfloat16).contiguous()
    st = torch.cuda.current_stream().cuda_stream
    ref = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    check(lib.meant_qkv_proj_fwd(x.data_ptr(), D_MODEL, wc.data_ptr(), b.data_ptr(), ref.data_ptr(), M, D_MODEL, S, HEADS, Dh, qa.shape[1],
                                 qa.data_ptr(), qb.data_ptr(), ka.data_ptr(), kb.data_ptr(), BF16, st), "qkv_proj_fwd")
    out = torch.full((M, N), float("nan"), device=dev, dtype=torch.bfloat16)
    before = _lib.route_count("nt256s_rot")
    check(lib.meant_qkv_proj_fwd_live(x.data_ptr(), D_MODEL, wc.data_ptr(), b.data_ptr(), out.data_ptr(), M, D_MODEL, S, HEADS, Dh, qa.shape[1],
                                      qa.data_ptr(), qb.data_ptr(), ka.data_ptr(), kb.data_ptr(), lists.data_ptr(), BF16, st), "qkv_proj_fwd_live")
    torch.cuda.synchronize()
    assert _lib.route_count("nt256s_rot") == before + 2      # both sections on the streaming kernel
    pdead = _dead_blocks(np_mask, causal).reshape(-1, 4).all(axis=1)
    dead_rows = torch.from_numpy(np.repeat(pdead, 256)).to(dev)
    assert torch.equal(out[:, :D_MODEL], ref[:, :D_MODEL])
    assert torch.equal(out[~dead_rows][:, D_MODEL:], ref[~dead_rows][:, D_MODEL:])
    assert (out[dead_rows][:, D_MODEL:] == 0).all()
    assert pdead.sum() == {"none": 0, "upper_half": G}.get(name, pdead.sum())


@pytest.mark.parametrize("name,causal", CASES, ids=IDS)
def test_fused_attention_equal_with_the_option_on_and_off(dev, operands, monkeypatch, name, causal):
    from meant_amd import _lib, ops
    np_mask = _mask(name)
    mask = torch.from_numpy(np_mask).to(dev)
    x = operands[0]
    o0, dx0, dw0, db0, dqkv0 = _run(operands, mask, causal, 0, monkeypatch)
    before = _lib.route_count("tn256_rows")
    o1, dx1, dw1, db1, dqkv1 = _run(operands, mask, causal, _lib.get_option("kv_skip") or (ops.KV_SKIP_DW | ops.KV_SKIP_FWD), monkeypatch)
    assert _lib.route_count("tn256_rows") == before + 1      # the list form of the dW kernel really ran
    assert torch.equal(o0, o1)
    assert torch.equal(dqkv0, dqkv1)
    assert torch.equal(dx0, dx1)
    # the premise: the dk / dv rows of every dead block are exact zeros
    dead = torch.from_numpy(np.repeat(_dead_blocks(np_mask, causal).reshape(-1), 64)).to(dev)
    assert dead.sum().item() == 64 * int(_dead_blocks(np_mask, causal).sum())
    assert (dqkv0[dead][:, D_MODEL:] == 0).all()
    # dw, db against fp64 on the same bf16 operands
    x2 = x.view(G * S, D_MODEL).double()
    dw_ref = dqkv0.double().t() @ x2
    db_ref = dqkv0.double().sum(dim=0)
    errs = {}
    for tag, dw, db in (("off", dw0, db0), ("on", dw1, db1)):
        errs[tag] = ((dw.double() - dw_ref).abs().max().item() / dw_ref.abs().max().item(),
                     (db.double() - db_ref).abs().max().item() / db_ref.abs().max().item())
    print(f"kv_skip {name} {'causal' if causal else 'full'}: dw rel err off {errs['off'][0]:.3e} on {errs['on'][0]:.3e}; "
          f"db rel err off {errs['off'][1]:.3e} on {errs['on'][1]:.3e}")
    assert errs["on"][0] <= 2 * errs["off"][0], errs
    assert errs["on"][1] <= 2 * errs["off"][1], errs


def test_whole_model_train_step_equal_with_the_option_on_and_off(dev):
    """a 2-sample, lag-2 meant in train mode, trailing pads of mask (b) cycled over its four text sequences (1024 tokens each, so that
    the projection's weight gradient has the 4096 token rows the 256 x 256 dW kernel starts at): loss and every parameter gradient,
    under the tolerance tests/test_gpu_bench_path.py uses for two bf16 evaluations of one model"""
    import meant_amd as M
    from meant_amd import _lib
    from meant_amd.train import cross_entropy_on_probs
    torch.manual_seed(5)
    dim, s = 256, 1024
    m = M.meant(dim, dim, 4, 32, 64, 16, 2, 3, torch.nn.Embedding(50, dim), num_heads=4, num_encoders=1, channels=4).to(dev).train()
    m.compute_dtype = torch.bfloat16
    rs = np.random.RandomState(8)
    ids = torch.from_numpy(rs.randint(0, 50, (2, 2, s))).to(dev)
    img = torch.from_numpy(rs.standard_normal((2, 2, 4, 32, 64)).astype("float32")).to(dev)
    mask = torch.from_numpy(_trailing(PADS_B, 4, s).reshape(2, 2, s)).to(dev)
    target = torch.tensor([0, 2], device=dev)
    res = []
    old = _lib.get_option("kv_skip")
    try:
        for v in (0, old or 3):
            _lib.set_option("kv_skip", v)
            m.zero_grad(set_to_none=True)
            torch.manual_seed(77)
            before = _lib.route_count("tn256_rows")
            loss = cross_entropy_on_probs(m(ids, img, mask), target)
            loss.backward()
            torch.cuda.synchronize()
            assert (_lib.route_count("tn256_rows") > before) == bool(v)
            res.append((loss.item(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}))
    finally:
        _lib.set_option("kv_skip", old)
    tol = TOL[torch.bfloat16]
    assert abs(res[0][0] - res[1][0]) <= tol["out"]
    assert res[0][1].keys() == res[1][1].keys()
    big = max(g.norm().item() for g in res[0][1].values())
    for k, g0 in res[0][1].items():
        g1 = res[1][1][k]
        assert torch.isfinite(g1).all(), k
        assert (g0 - g1).norm().item() <= tol["gnorm"] * max(g0.norm().item(), 2e-2 * big), k
