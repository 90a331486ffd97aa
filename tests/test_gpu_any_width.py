"""MEANT models at widths that are no multiple of 8, end to end: the four model classes and the encoder layers against the CPU oracle
(setup and tolerances of tests/test_gpu_models.py), the element forms of meant_add_rowvec / meant_meanpool_fwd / meant_meanpool_bwd
at the C ABI against float64, and the bf16 Linear backward at output widths N % 8 != 0, which moves from the exact-f32 engine to the
MFMA kernels (conventions and tolerances of tests/test_gpu_linear_tail.py).

Tolerances of the C-ABI kernel tests, from the number formats (unit roundoffs u32 = 2^-24 of float's 24 and u16 = 2^-8 of bfloat16's 8
significand bits: the relative error of one rounding to nearest):
  * add_rowvec: one float add of two exactly representable operands, rounded once to the storage type: |err| <= u |y|, plus one more
    u32 |y| for the add itself in the bf16 tier.
  * mean-pool forward: S float adds in a fixed order, one multiply by the rounded 1 / S, one rounding to the output type:
    |err| <= (S + 2) u32 max|x| + u_out |mean|.
  * mean-pool backward: one multiply by the rounded 1 / S and one rounding: |err| <= (2 u32 + u_out) |dout| / S.
The route assertions of the Linear cases: the weight gradient hands whole 64-row tiles to the MFMA kernel and the M % 64 trailing rows
to the exact kernel ("tn_tail", which counts one "gemm_f32" launch: tests/test_gpu_linear_tail.py's docstring), so "tn128" + "tn256"
is 1 from M = 64 on and 0 at M = 1 (no whole tile), "tn_tail" is 1 where M % 64 != 0, and nothing else may count under "gemm_f32"."""
import math

import numpy as np
import pytest
import torch

from tests.util import DTYPES, IDS, TOL, t, assert_close, assert_grad_close, pair, compare_param_grads

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
U32, U16 = 2.0 ** -24, 2.0 ** -8
ROUTES = ("nt128", "nt256", "nt256s", "nt_split", "nt_overlap", "nt128k", "nt256k", "gemm_f32", "tn128", "tn256", "tn_tail")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture()
def L():
    from meant_amd import _lib
    saved = {k: _lib.get_option(k) for k in ("nt_dynamic", "nt_grid_cap", "nt_stream", "deterministic", "nt_ragged")}
    for k, v in (("nt_dynamic", 1), ("nt_grid_cap", 0), ("nt_stream", 1), ("deterministic", 0), ("nt_ragged", 1)):
        _lib.set_option(k, v)
    _lib.route_reset()
    yield _lib
    for k, v in saved.items():
        _lib.set_option(k, v)


@pytest.fixture()
def deterministic():
    from meant_amd import _lib
    old = _lib.get_option("deterministic")
    _lib.set_option("deterministic", 1)
    yield _lib
    _lib.set_option("deterministic", old)


def _st():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the model classes against the CPU oracle
B_, LAG, S_, V_ = 2, 2, 24, 60
IMG = dict(h=32, w=32, p=4, c=3)                           # 64 patches of 4 x 4 x 3: the tiled attention kernels


def _mk(cls_name, args, kw, emb, dev):
    import meant_amd
    from oracle import meant_oracle as O
    a = list(args)
    ref = getattr(O, cls_name)(*(a + ([torch.nn.Embedding(*emb)] if emb else [])), **kw)
    hip = getattr(meant_amd, cls_name)(*(a + ([torch.nn.Embedding(*emb)] if emb else [])), **kw)
    return pair(ref, hip, 1234, dev)


def _inputs(seed, lag=True):
    """ids, images, mask with a random tail of padding per sequence, targets"""
    r = np.random.RandomState(seed)
    lead = (B_, LAG) if lag else (B_,)
    ids = t(r.randint(0, V_, lead + (S_,)).astype("int64"))
    img = t(r.standard_normal(lead + (IMG["c"], IMG["h"], IMG["w"])).astype("float32"))
    keep = r.randint(S_ // 2, S_ + 1, lead)
    mask = t((np.arange(S_)[None, :] < keep.reshape(-1, 1)).astype("float32")).reshape(lead + (S_,))
    return ids, img, mask, torch.tensor([2, 0])


def _build(cls, td, idim, heads, dev):
    kw = dict(num_heads=heads, num_encoders=1, channels=IMG["c"])
    geo = (IMG["h"], IMG["w"], IMG["p"])
    if cls == "meant":
        return _mk(cls, (td, idim, 4) + geo + (LAG, 3), kw, (V_, td), dev)
    if cls == "meant_vqa":
        return _mk(cls, (td, idim, 4) + geo + (1, 3), kw, (V_, td), dev)
    if cls == "meant_tweet":
        return _mk(cls, (td, 4, LAG, 3), dict(num_heads=heads, num_encoders=1), (V_, td), dev)
    return _mk(cls, (idim, 4) + geo + (LAG, 3), kw, None, dev)


def _args_of(cls, ids, img, mask):
    return {"meant": (ids, img, mask), "meant_vqa": (ids, img, mask), "meant_tweet": (ids, mask), "meant_vision": (img,)}[cls]


def _model_case(cls, td, idim, heads, dtype, dev):
    ref, hip = _build(cls, td, idim, heads, dev)
    ids, img, mask, tgt = _inputs(td + idim, lag=cls != "meant_vqa")
    out_r = ref(*_args_of(cls, ids, img, mask))
    loss_r = torch.nn.functional.cross_entropy(out_r, tgt)
    loss_r.backward()
    hip.compute_dtype = dtype
    out = hip(*[x.to(dev) for x in _args_of(cls, ids, img, mask)])
    assert out.dtype == torch.float32 and out.shape == out_r.shape
    loss = torch.nn.functional.cross_entropy(out, tgt.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    assert_close(out, out_r, TOL[dtype]["out"], "out")
    assert abs(loss.item() - loss_r.item()) <= TOL[dtype]["out"]
    compare_param_grads(ref, hip, dtype, f"{cls}_{td}_{idim}")
    return hip


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("td,idim", [(100, 50), (99, 51)], ids=["100_50", "99_51"])
@pytest.mark.parametrize("cls", ["meant", "meant_tweet", "meant_vision", "meant_vqa"])
def test_models_at_widths_off_the_grid(dev, cls, td, idim, dtype):
    """(100, 50): d = 4 mod 8, the concat writes the image means at col_off = 100 of rows of 150; (99, 51): odd widths, bf16 rows on
    2-byte boundaries, int(dim / heads) * heads < dim.  Every one of these raised MeantHipError in its first forward before."""
    _model_case(cls, td, idim, 2, dtype, dev)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_vision_model_at_260(dev, dtype):
    """d above 256: the mean-pool's second column block runs, with a ragged end (4 of its 256 columns)"""
    _model_case("meant_vision", 0, 260, 4, dtype, dev)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the encoder layers alone
def _layer_case(ref, hip, x, w, dtype, dev, what, *extra):
    xr = x.to(dtype).float().clone().requires_grad_()            # a copy: in the fp32 tier the conversions return x itself
    out_r = ref(xr, *extra)
    (out_r * w).sum().backward()
    xh = x.to(dev).to(dtype).requires_grad_()
    out = hip(xh, *[e.to(dev) for e in extra])
    (out.float() * w.to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert out.dtype == dtype and out.shape == out_r.shape
    tol = TOL[dtype]
    assert_close(out, out_r, tol["out"] * max(1.0, out_r.abs().max().item()), what)
    assert_grad_close(xh.grad, xr.grad, tol["gelem"], what + " dx")
    compare_param_grads(ref, hip, dtype, what)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_encoder_layers_at_width_100(dev, dtype):
    import meant_amd
    from oracle import meant_oracle as O
    gen = torch.Generator().manual_seed(100)
    x, w = torch.randn(3, 64, 100, generator=gen), torch.randn(3, 64, 100, generator=gen)
    ref, hip = pair(O.visionEncoder(100, 2), meant_amd.visionEncoder(100, 2), 1234, dev)
    _layer_case(ref, hip, x, w, dtype, dev, "visionEncoder_100")
    x, w = torch.randn(3, S_, 100, generator=gen), torch.randn(3, S_, 100, generator=gen)
    mask = torch.ones(3, S_)
    mask[1, 17:] = 0
    mask[2, 5:] = 0
    ref, hip = pair(O.languageEncoder(100, 2), meant_amd.languageEncoder(100, 2), 1234, dev)
    _layer_case(ref, hip, x, w, dtype, dev, "languageEncoder_100", mask)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("norms", [True, False], ids=["norms", "no_norms"])
def test_temporal_encoder_at_width_150(dev, dtype, norms):
    import meant_amd
    from oracle import meant_oracle as O
    gen = torch.Generator().manual_seed(150)
    x, w = torch.randn(5, 3, 150, generator=gen), torch.randn(5, 1, 150, generator=gen)
    ref, hip = pair(O.temporalEncoder(150, 2, 3, norms=norms), meant_amd.temporalEncoder(150, 2, 3, norms=norms), 1234, dev)
    _layer_case(ref, hip, x, w, dtype, dev, f"temporalEncoder_150_{norms}")


def _drop_mask(rows, d, p, seed, dev):
    """keep / (1 - p) factors of the norm kernels' dropout at this [rows, d] shape and seed (tests/test_gpu_bench_path.py::_mask_of,
    with the opt-in for the width)"""
    from meant_amd import ops
    y = ops.rmsnorm(torch.ones(rows, d, device=dev), torch.ones(d, device=dev), 1e-8, p, seed, any_width=True)
    keep = (y != 0).float()
    assert abs(keep.mean().item() - (1 - p)) < 0.03
    return keep / (1.0 - p)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_language_encoder_100_train_mode_dropout(dev, dtype, monkeypatch):
    """languageEncoder(100, 2, dropout=0.3) in .train(): Dropout(0.3) rides encode[3]'s RMSNorm kernel, the default-p Dropout()
    encode2[3]'s (ops.linear_gelu_rmsnorm).  The reference is the eager fp32 encoder with the kernels' masks, read back from the plain
    norm at the same [rows, 100] shape and seed (the method of tests/test_gpu_models_wide.py)."""
    import meant_amd
    from meant_amd import modules
    from oracle import meant_oracle as O
    d, heads, Bq, seed = 100, 2, 8, 4242
    monkeypatch.setattr(modules, "_seed", lambda: seed)
    ref, hip = pair(O.languageEncoder(d, heads), meant_amd.languageEncoder(d, heads, dropout=0.3), 1234, dev)
    hip.train()
    p1, p2 = hip.encode[4].p, hip.encode2[4].p
    assert p1 == 0.3 and p2 == 0.5
    gen = torch.Generator().manual_seed(9)
    x, w = torch.randn(Bq, S_, d, generator=gen), torch.randn(Bq, S_, d, generator=gen)
    m1 = _drop_mask(Bq * S_, d, p1, seed, dev).view(Bq, S_, d).cpu()
    m2 = _drop_mask(Bq * S_, d, p2, seed, dev).view(Bq, S_, d).cpu()

    xr = x.to(dtype).float()
    e, e2 = ref.encode, ref.encode2
    h = e[3](e[2](e[1](e[0](xr)), None)) * m1
    x1 = e[-1](h) + xr
    y_r = e2[3](torch.nn.functional.gelu(e2[1](e2[0](x1)))) * m2
    out_r = e2[-1](y_r) + x1
    (out_r * w).sum().backward()

    out = hip(x.to(dev).to(dtype))
    (out.float() * w.to(dev)).sum().backward()
    torch.cuda.synchronize()
    tol = TOL[dtype]
    assert_close(out, out_r, tol["out"] * max(1.0, out_r.abs().max().item()), "out")
    compare_param_grads(ref, hip, dtype, "languageEncoder_100_train")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the three kernels (and meant_add_rowvec_bwd) at the C ABI against float64
WIDTHS = (1, 7, 9, 100, 255, 260, 1028)
SENTINEL = 7.0


def _code(dt):
    from meant_amd import _lib
    return _lib.BF16 if dt == BF else _lib.F32


def _in_nan_pool(v, dtype, dev, lead=64, trail=256):
    """a device copy of v in `dtype` inside a NaN-filled allocation (lead elements in front, trail behind): a read in front of the first
    or behind the last element that entered a result would make it NaN"""
    pool = torch.full((lead + v.numel() + trail,), float("nan"), device=dev, dtype=dtype)
    view = pool[lead:lead + v.numel()].view(v.shape)
    view.copy_(v.to(dev).to(dtype))
    return pool, view


def _at_the_end(v, dtype, dev, lead=64):
    """a device copy of v in `dtype` whose last element is the last element of its allocation"""
    pool = torch.full((lead + v.numel(),), float("nan"), device=dev, dtype=dtype)
    view = pool[lead:].view(v.shape)
    view.copy_(v.to(dev).to(dtype))
    return pool, view


def _u(dt):
    return U16 if dt == BF else U32


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("period", [1, 3])
def test_add_rowvec_any_width(dev, dtype, period):
    from meant_amd import _lib
    rs = np.random.RandomState(period)
    for d in WIDTHS:
        for rows in (period, 5 * period, 64 * period):
            x = t(rs.standard_normal((rows, d)).astype("float32")).to(dtype)
            v = t(rs.standard_normal((period, d)).astype("float32"))
            place = _at_the_end if rows == period else _in_nan_pool
            (_, xh), (_, vh) = place(x, dtype, dev), place(v, torch.float32, dev)
            ybuf = torch.full((rows + 2, d), SENTINEL, device=dev, dtype=dtype)
            runs = []
            for _ in range(2):
                ybuf.fill_(SENTINEL)
                _lib.check(_lib.lib.meant_add_rowvec(xh.data_ptr(), vh.data_ptr(), ybuf[1].data_ptr(), rows, d, period, _code(dtype), _st()),
                           "add_rowvec")
                runs.append(ybuf.cpu().clone())
            assert torch.equal(runs[0], runs[1]), (d, rows)
            got = runs[0]
            assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all(), (d, rows)
            want = x.double() + v.double().repeat(rows // period, 1)
            err = (got[1:-1].double() - want).abs()
            assert torch.isfinite(got[1:-1].float()).all() and (err <= (_u(dtype) + U32) * want.abs() + 1e-30).all(), (d, rows, err.max().item())
            # the gradient of v: ordered sums over the rows of each residue class; no width rule before either
            dyh = xh
            dv = torch.full((period + 2, d), SENTINEL, device=dev, dtype=torch.float32)
            _lib.check(_lib.lib.meant_add_rowvec_bwd(dyh.data_ptr(), dv[1].data_ptr(), rows, d, period, _code(dtype), _st()), "add_rowvec_bwd")
            dvc = dv.cpu()
            assert (dvc[0] == SENTINEL).all() and (dvc[-1] == SENTINEL).all(), (d, rows)
            want_dv = x.double().view(rows // period, period, d).sum(0)
            bound = (rows // period + 1) * U32 * x.double().abs().view(rows // period, period, d).sum(0) + 1e-30
            assert ((dvc[1:-1].double() - want_dv).abs() <= bound).all(), (d, rows)


POOL_DTYPES = [(torch.float32, torch.float32), (BF, torch.float32), (BF, BF)]


@pytest.mark.parametrize("dt,dto", POOL_DTYPES, ids=["f32_f32", "bf16_f32", "bf16_bf16"])
@pytest.mark.parametrize("S", [1, 5, 64])
def test_meanpool_any_width(dev, dt, dto, S):
    """forward into, backward out of, columns [col_off, col_off + d) of rows of ld_out = col_off + d + 5 elements.  The output buffers
    carry a sentinel everywhere (a row in front, a row behind, the columns around the slice); the backward's dout carries NaN
    everywhere outside the slice; x is the last thing in its allocation (G = 1) or lies in a NaN pool."""
    from meant_amd import _lib
    rs = np.random.RandomState(S)
    for d in WIDTHS:
        for col_off in (0, 3, 100):
            ld = col_off + d + 5
            G = 1 if col_off == 3 else 3
            x = t(rs.standard_normal((G, S, d)).astype("float32")).to(dt)
            _, xh = (_at_the_end if G == 1 else _in_nan_pool)(x, dt, dev)
            out = torch.full((G + 2, ld), SENTINEL, device=dev, dtype=dto)
            runs = []
            for _ in range(2):
                out.fill_(SENTINEL)
                _lib.check(_lib.lib.meant_meanpool_fwd(xh.data_ptr(), out[1].data_ptr(), ld, col_off, G, S, d, _code(dt), _code(dto), _st()),
                           "meanpool_fwd")
                runs.append(out.cpu().clone())
            assert torch.equal(runs[0], runs[1]), (d, col_off)
            got = runs[0]
            inside = torch.zeros(G + 2, ld, dtype=torch.bool)
            inside[1:-1, col_off:col_off + d] = True
            assert (got[~inside] == SENTINEL).all(), (d, col_off)
            want = x.double().mean(dim=1)
            bound = (S + 2) * U32 * x.double().abs().amax(dim=1) + _u(dto) * want.abs() + 1e-30
            res = got[1:-1, col_off:col_off + d].double()
            assert torch.isfinite(res).all() and ((res - want).abs() <= bound).all(), (d, col_off, (res - want).abs().max().item())

            dout = torch.full((G, ld), float("nan"), dtype=torch.float32)
            dout[:, col_off:col_off + d] = t(rs.standard_normal((G, d)).astype("float32"))
            _, dh = _at_the_end(dout, dto, dev)
            dx = torch.full((G + 2, S, d), SENTINEL, device=dev, dtype=dt)
            runs = []
            for _ in range(2):
                dx.fill_(SENTINEL)
                _lib.check(_lib.lib.meant_meanpool_bwd(dh.data_ptr(), ld, col_off, dx[1].data_ptr(), G, S, d, _code(dt), _code(dto), _st()),
                           "meanpool_bwd")
                runs.append(dx.cpu().clone())
            assert torch.equal(runs[0], runs[1]), (d, col_off)
            got = runs[0]
            assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all(), (d, col_off)
            want = (dh.cpu().double()[:, col_off:col_off + d] / S)[:, None, :].expand(G, S, d)
            res = got[1:-1].double()
            assert torch.isfinite(res).all() and ((res - want).abs() <= (2 * U32 + _u(dt)) * want.abs() + 1e-30).all(), (d, col_off)


@pytest.mark.parametrize("dt,dto", POOL_DTYPES, ids=["f32_f32", "bf16_f32", "bf16_bf16"])
def test_aligned_shapes_keep_the_chunk_kernels_bits(dev, dt, dto):
    """d = 768 at col_off = 768 of rows of 1536 with 16-byte aligned bases takes the chunk kernels, as it always has; the same call on
    copies of the operands that start one element later is the element form.  Both sum in the same order: the results are equal bit
    for bit, so a shape that changed sides in the dispatch would not change a model's numbers -- and a dispatch that sent the aligned
    shape to the element form of a DIFFERENT order would show here."""
    from meant_amd import _lib
    rs = np.random.RandomState(768)
    G, S, d, off, ld = 3, 5, 768, 768, 1536
    x = t(rs.standard_normal((G, S, d)).astype("float32")).to(dt)
    res = []
    for shift in (0, 1):
        pool = torch.zeros(8 + x.numel(), device=dev, dtype=dt)
        xh = pool[shift:shift + x.numel()].view(G, S, d)
        xh.copy_(x.to(dev))
        obuf = torch.zeros(8 + G * ld, device=dev, dtype=dto)
        oh = obuf[shift:shift + G * ld].view(G, ld)
        assert (xh.data_ptr() % 16 == 0) == (shift == 0) and (oh.data_ptr() % 16 == 0) == (shift == 0)
        _lib.check(_lib.lib.meant_meanpool_fwd(xh.data_ptr(), oh.data_ptr(), ld, off, G, S, d, _code(dt), _code(dto), _st()), "meanpool_fwd")
        dx = torch.zeros(8 + x.numel(), device=dev, dtype=dt)
        dxh = dx[shift:shift + x.numel()].view(G, S, d)
        _lib.check(_lib.lib.meant_meanpool_bwd(oh.data_ptr(), ld, off, dxh.data_ptr(), G, S, d, _code(dt), _code(dto), _st()), "meanpool_bwd")
        y = torch.zeros(8 + x.numel(), device=dev, dtype=dt)
        yh = y[shift:shift + x.numel()].view(G * S, d)
        v = t(rs.standard_normal((S, d)).astype("float32")).to(dev) if shift == 0 else v
        _lib.check(_lib.lib.meant_add_rowvec(xh.data_ptr(), v.data_ptr(), yh.data_ptr(), G * S, d, S, _code(dt), _st()), "add_rowvec")
        res.append((oh.cpu().clone(), dxh.cpu().clone(), yh.cpu().clone()))
    for a, b, what in zip(res[0], res[1], ("meanpool_fwd", "meanpool_bwd", "add_rowvec")):
        assert torch.equal(a, b), what
    want = x.double().mean(dim=1)
    assert ((res[0][0][:, off:].double() - want).abs() <= (S + 2) * U32 * x.double().abs().amax(dim=1) + _u(dto) * want.abs()).all()


def _sentinel_rows(rows, d, dtype, dev, shift=0):
    """a SENTINEL-filled buffer of rows + 2 rows of d (+ shift elements in front) and its inner rows: the slice a kernel writes"""
    buf = torch.full((shift + (rows + 2) * d,), SENTINEL, device=dev, dtype=dtype)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[shift + d:shift + (rows + 1) * d].view(rows, d)


def _sentinels_intact(buf, rows, d, shift=0):
    got = buf.cpu()
    return bool((got[:shift + d] == SENTINEL).all() and (got[shift + (rows + 1) * d:] == SENTINEL).all())


def _rel64(a, b):
    """max-abs error against the float64 reference b over b's largest magnitude (tests/test_gpu_timesformer_any.py::_rel)"""
    return (a.double().cpu() - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


GUARD_WIDTHS = (9, 15, 17)      # one element past a chunk of 8, one short of two chunks, one past two: where a wrong guard shows
GUARD_OPS = {"gather_rows": 1, "token_shift": 2, "geglu_fwd": 1, "geglu_bwd": 1, "dropout": 1, "add_rowvec": 0, "embedding_fwd": 0}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("op", list(GUARD_OPS))
def test_row_ops_write_their_slice_only(dev, dtype, op):
    """the row-wise entries at widths 9, 15 and 17 (dropout: lengths), three rows (token_shift: two videos of 2 frames x 2 tokens): the
    output is the inside of a buffer with a sentinel row in front and one behind, the inputs lie in NaN pools.  The slice against
    torch at the op's tolerance elsewhere in the suite (tests/test_gpu_timesformer_any.py; add_rowvec: above; the embedding lookup is
    one rounding of an fp32 value: exact in fp32, within u16 |value| in bf16), bit for bit where the op only moves data; every
    sentinel intact; "rows_elem" counted once per launch by the entries that count it.  add_rowvec also at width 16 from bases one
    element past a 16-byte boundary, where the alignment alone sends it to the element form (the pools there: the next test); dropout
    both into an unaligned slice (every group by element) and from 16-byte aligned bases (16-byte groups and an element tail)."""
    from meant_amd import _lib
    lib, code, rs = _lib.lib, _code(dtype), np.random.RandomState(len(op))
    u = _u(dtype)

    def rnd(*shape, dt=dtype, lead=64):
        v = t(rs.standard_normal(shape).astype("float32")).to(dt)
        return v, _in_nan_pool(v, dt, dev, lead=lead)[1]

    for d in GUARD_WIDTHS + ((16,) if op == "add_rowvec" else ()):
        shift = 1 if d == 16 else 0
        rows = 10 if op == "token_shift" else (1 if op == "dropout" else 3)
        buf, out = _sentinel_rows(rows, 2 * d if op == "geglu_bwd" else d, dtype, dev, shift)
        hits = _lib.route_count("rows_elem")
        if op == "gather_rows":
            (src, src_d), (fill, fill_d) = rnd(4, d), rnd(d)
            idx = torch.tensor([2, -2, -1], dtype=torch.int32, device=dev)
            _lib.check(lib.meant_gather_rows(src_d.data_ptr(), idx.data_ptr(), fill_d.data_ptr(), out.data_ptr(), 3, d, code, _st()), op)
            assert torch.equal(out.cpu(), torch.stack((src[2], fill, torch.zeros(d, dtype=dtype)))), d
        elif op == "token_shift":
            from oracle import meant_oracle as O
            (x, x_d), (yb, yb_d) = rnd(2, 5, d), rnd(2, 5, d)
            xr = x.float().requires_grad_(True)
            ref = O._TSPreTokenShift(2, lambda y: y)(xr)
            ref.backward(yb.float())
            _lib.check(lib.meant_token_shift(x_d.data_ptr(), out.data_ptr(), 2, 2, 2, d, 0, code, _st()), op)
            assert torch.equal(out.cpu().view(2, 5, d), ref.detach().to(dtype)), d
            assert _sentinels_intact(buf, rows, d), d
            _lib.check(lib.meant_token_shift(yb_d.data_ptr(), out.data_ptr(), 2, 2, 2, d, 1, code, _st()), op)
            assert torch.equal(out.cpu().view(2, 5, d), xr.grad.to(dtype)), d
        elif op in ("geglu_fwd", "geglu_bwd"):
            (h, h_d), (dy, dy_d) = rnd(3, 2 * d), rnd(3, d)
            hr = h.double().requires_grad_(True)
            a, g = hr.chunk(2, dim=-1)
            yr = a * torch.nn.functional.gelu(g)
            yr.backward(dy.double())
            if op == "geglu_fwd":
                _lib.check(lib.meant_geglu_fwd(h_d.data_ptr(), out.data_ptr(), 3, d, code, _st()), op)
                assert _rel64(out, yr.detach()) <= (2e-5 if dtype == torch.float32 else 8e-3), d
            else:
                _lib.check(lib.meant_geglu_bwd(h_d.data_ptr(), dy_d.data_ptr(), out.data_ptr(), 3, d, code, _st()), op)
                assert _rel64(out, hr.grad) <= (2e-5 if dtype == torch.float32 else 1e-2), d
        elif op == "dropout":                                # keep_scale8's rule: element i takes part i & 7 of the draw for i >> 3, so the
            x = t(rs.standard_normal(24).astype("float32"))  # 16-byte kernel on 24 elements gives the first d of them the same mask
            x[x.abs() < 0.1] = 0.5
            x = x.to(dtype)
            x24, y24 = x.to(dev), torch.empty(24, device=dev, dtype=dtype)
            _, x_d = _in_nan_pool(x[:d], dtype, dev)
            _lib.check(lib.meant_dropout(x_d.data_ptr(), out.data_ptr(), d, 0.25, 1234, code, _st()), op)
            assert _lib.route_count("rows_elem") == hits + 1, d
            _lib.check(lib.meant_dropout(x24.data_ptr(), y24.data_ptr(), 24, 0.25, 1234, code, _st()), op)
            got = out.cpu().view(-1)
            assert torch.equal(got, y24.cpu()[:d]), d
            kept = (x[:d].float() * torch.tensor(65536.0 / (65536.0 - 16384.0))).to(dtype)
            assert torch.all((got == 0) | (got == kept)), d
            # the route a model takes: both bases on 16 bytes, so 16-byte groups and an element tail (above, `out` starts d elements
            # into its buffer: off 16 bytes at these d, every group by element)
            buf16 = torch.full((16 + d + 16,), SENTINEL, device=dev, dtype=dtype)
            out16 = buf16[16:16 + d]
            assert x_d.data_ptr() % 16 == 0 and out16.data_ptr() % 16 == 0 and out.data_ptr() % 16 != 0
            _lib.check(lib.meant_dropout(x_d.data_ptr(), out16.data_ptr(), d, 0.25, 1234, code, _st()), op)
            assert _lib.route_count("rows_elem") == hits + 2, d
            got16 = buf16.cpu()
            assert torch.equal(got16[16:16 + d], got) and (got16[:16] == SENTINEL).all() and (got16[16 + d:] == SENTINEL).all(), d
            hits += 1
        elif op == "add_rowvec":
            (x, x_d), (v, v_d) = rnd(3, d, lead=64 + shift), rnd(3, d, dt=torch.float32)
            assert d != 16 or (x_d.data_ptr() % 16 != 0 and out.data_ptr() % 16 != 0)
            _lib.check(lib.meant_add_rowvec(x_d.data_ptr(), v_d.data_ptr(), out.data_ptr(), 3, d, 3, code, _st()), op)
            want = x.double() + v.double()
            assert ((out.cpu().double() - want).abs() <= (u + U32) * want.abs() + 1e-30).all(), d
        else:
            table, table_d = rnd(5, d, dt=torch.float32)
            ids = torch.tensor([4, -3, 7], device=dev)       # clamped to [0, V)
            _lib.check(lib.meant_embedding_fwd(table_d.data_ptr(), ids.data_ptr(), out.data_ptr(), 3, d, 5, code, _st()), op)
            want = table[[4, 0, 4]]
            if dtype == torch.float32:
                assert torch.equal(out.cpu(), want), d
            else:
                assert ((out.cpu().double() - want.double()).abs() <= U16 * want.double().abs()).all(), d
        torch.cuda.synchronize()
        assert _sentinels_intact(buf, rows, out.shape[1], shift), (op, d)
        assert torch.isfinite(out.float()).all(), (op, d)
        assert _lib.route_count("rows_elem") == hits + GUARD_OPS[op], (op, d)


@pytest.mark.parametrize("dt,dto", POOL_DTYPES, ids=["f32_f32", "bf16_f32", "bf16_bf16"])
def test_meanpool_width_16_from_bases_one_element_off(dev, dt, dto):
    """d = 16 at col_off = 8 of rows of ld = 32 -- every width on the 8-grid -- with x, out, dout and dx one element past a 16-byte
    boundary: the alignment alone sends both pools to the element form, where every chunk is a whole one.  Sentinels in front of,
    behind and around the written slice (dout: NaN there), x in a NaN pool; the tolerances of test_meanpool_any_width; neither
    entry counts under "rows_elem"."""
    from meant_amd import _lib
    rs = np.random.RandomState(16)
    G, S, d, off, ld = 3, 5, 16, 8, 32
    x = t(rs.standard_normal((G, S, d)).astype("float32")).to(dt)
    _, xh = _in_nan_pool(x, dt, dev, lead=65)
    obuf = torch.full((1 + (G + 2) * ld,), SENTINEL, device=dev, dtype=dto)
    out = obuf[1 + ld:1 + (G + 1) * ld].view(G, ld)
    assert xh.data_ptr() % 16 != 0 and out.data_ptr() % 16 != 0 and obuf.data_ptr() % 16 == 0
    hits = _lib.route_count("rows_elem")
    _lib.check(_lib.lib.meant_meanpool_fwd(xh.data_ptr(), out.data_ptr(), ld, off, G, S, d, _code(dt), _code(dto), _st()), "meanpool_fwd")
    got = obuf.cpu()
    inside = torch.zeros(1 + (G + 2) * ld, dtype=torch.bool)
    inside[1 + ld:1 + (G + 1) * ld].view(G, ld)[:, off:off + d] = True
    assert (got[~inside] == SENTINEL).all()
    want = x.double().mean(dim=1)
    res = got[inside].view(G, d).double()
    bound = (S + 2) * U32 * x.double().abs().amax(dim=1) + _u(dto) * want.abs() + 1e-30
    assert torch.isfinite(res).all() and ((res - want).abs() <= bound).all(), (res - want).abs().max().item()

    dout = torch.full((G, ld), float("nan"), dtype=torch.float32)
    dout[:, off:off + d] = t(rs.standard_normal((G, d)).astype("float32"))
    _, dh = _in_nan_pool(dout, dto, dev, lead=65)
    dbuf = torch.full((1 + (G + 2) * S * d,), SENTINEL, device=dev, dtype=dt)
    dx = dbuf[1 + S * d:1 + (G + 1) * S * d].view(G, S, d)
    assert dh.data_ptr() % 16 != 0 and dx.data_ptr() % 16 != 0
    _lib.check(_lib.lib.meant_meanpool_bwd(dh.data_ptr(), ld, off, dx.data_ptr(), G, S, d, _code(dt), _code(dto), _st()), "meanpool_bwd")
    got = dbuf.cpu()
    assert (got[:1 + S * d] == SENTINEL).all() and (got[1 + (G + 1) * S * d:] == SENTINEL).all()
    want = (dh.cpu().double()[:, off:off + d] / S)[:, None, :].expand(G, S, d)
    res = got[1 + S * d:1 + (G + 1) * S * d].view(G, S, d).double()
    assert torch.isfinite(res).all() and ((res - want).abs() <= (2 * U32 + _u(dt)) * want.abs() + 1e-30).all()
    assert _lib.route_count("rows_elem") == hits


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. ops.linear, bf16, output widths off the grid
def _rand(rs, *shape, scale=1.0):
    return torch.from_numpy((rs.standard_normal(shape) * scale).astype("float32"))


def _routes(L):
    return {r: L.route_count(r) for r in ROUTES}


def _linear_case(L, dev, M_, N, K, epi, sink=False):
    """tests/test_gpu_linear_tail.py::_linear_case: ops.linear forward + backward against fp32 on the CPU on the bf16-rounded inputs;
    returns the route counts of the backward alone.  sink: weight and bias under GradReducer(direct_grads=True)"""
    from meant_amd import ops
    from meant_amd._lib import EPI_NONE, EPI_GELU, EPI_SIGMOID
    rs = np.random.RandomState(M_ % 1000 + N + K)
    x, w, b = _rand(rs, M_, K), _rand(rs, N, K, scale=1 / math.sqrt(K)), _rand(rs, N, scale=0.1)
    res, dy = _rand(rs, M_, N), _rand(rs, M_, N)
    xq, wq, resq, dyq = [v.to(BF).float() for v in (x, w, res, dy)]
    xr, wr, br, rr = xq.clone().requires_grad_(), wq.clone().requires_grad_(), b.clone().requires_grad_(), resq.clone().requires_grad_()
    yr = torch.nn.functional.linear(xr, wr, br)
    if epi == "gelu":
        yr = torch.nn.functional.gelu(yr)
    elif epi == "sigmoid":
        yr = torch.sigmoid(yr)
    elif epi == "residual":
        yr = yr + rr
    yr.backward(dyq)
    xh = x.to(dev).to(BF).requires_grad_()
    wh, bh = torch.nn.Parameter(wq.to(dev)), torch.nn.Parameter(b.to(dev))
    rh = res.to(dev).to(BF).requires_grad_()
    e = {"none": EPI_NONE, "gelu": EPI_GELU, "sigmoid": EPI_SIGMOID, "residual": EPI_NONE}[epi]
    red = None
    if sink:
        from meant_amd.parallel import GradReducer
        red = GradReducer([wh, bh], direct_grads=True)
        red.prepare()
        assert id(wh) in ops.grad_sinks and id(bh) in ops.grad_sinks
    L.route_reset()
    yh = ops.linear(xh, wh, bh, rh if epi == "residual" else None, e)
    fwd = _routes(L)
    yh.backward(dy.to(dev).to(BF))
    if red is not None:
        red.wait()
    torch.cuda.synchronize()
    bwd = {r: c - fwd[r] for r, c in _routes(L).items()}
    if red is not None:
        red.close()
    assert fwd["gemm_f32"] == 0 or N < 8, fwd
    assert yh.shape == (M_, N) and xh.grad.shape == (M_, K) and wh.grad.shape == (N, K) and bh.grad.shape == (N,)
    assert_close(yh, yr, 3e-2 * max(1.0, yr.abs().max().item()), "y")
    assert_grad_close(xh.grad, xr.grad, 2e-2, "dx")
    assert_grad_close(wh.grad, wr.grad, 2e-2, "dw")
    assert_grad_close(bh.grad, br.grad, 2e-2, "db")
    if epi == "residual":
        assert_grad_close(rh.grad, rr.grad, 2e-2, "dres")
    return bwd, (wh.grad.detach().clone(), bh.grad.detach().clone(), xh.grad.detach().clone())


def _assert_mfma_backward(bwd, M_):
    assert bwd["nt128k"] + bwd["nt256k"] == 1 and bwd["nt128"] + bwd["nt256"] + bwd["nt256s"] == 0, bwd            # dX
    assert bwd["tn128"] + bwd["tn256"] == (1 if M_ >= 64 else 0), bwd                                                 # dW: whole 64-row tiles
    assert bwd["tn_tail"] == (1 if M_ % 64 else 0) and bwd["gemm_f32"] == bwd["tn_tail"], bwd                        # module docstring


@pytest.mark.parametrize("K", [64, 100, 768])
@pytest.mark.parametrize("N", [9, 100, 588, 1001])
def test_linear_backward_at_output_widths_off_the_grid(L, dev, N, K):
    """dX reduces over ceil8(N) = 16 / 104 / 592 / 1008, none a multiple of 64: a K-tail NT kernel; dW on the TN kernel through a
    [ceil8(N), ceil8(K)] accumulator.  K = 100 composes with the K-side padding (both operands off the grid, as in an odd-width model)"""
    for M_ in (1, 130, 300):
        for epi in ("none", "gelu", "sigmoid", "residual"):
            bwd, _ = _linear_case(L, dev, M_, N, K, epi)
            _assert_mfma_backward(bwd, M_)


def test_linear_backward_off_the_grid_under_a_gradient_sink(L, dev):
    """GradReducer(direct_grads=True): the padded accumulator is never written into a sink's [N, K] view -- the gradient goes back to
    autograd, which adds it into the bucket; the reduced gradient equals the plain one"""
    for K in (64, 100):
        bwd_s, (dw_s, db_s, dx_s) = _linear_case(L, dev, 130, 100, K, "none", sink=True)
        bwd_p, (dw_p, db_p, dx_p) = _linear_case(L, dev, 130, 100, K, "none")
        _assert_mfma_backward(bwd_s, 130)
        assert bwd_s == bwd_p
        assert torch.equal(dx_s, dx_p)
        assert_grad_close(dw_s, dw_p, 1e-5, "dw under the sink")          # the TN kernel adds its row splits with float atomics
        assert_grad_close(db_s, db_p, 1e-5, "db under the sink")


def test_class_head_width_keeps_its_route(L, dev):
    """N = 4 < 8: both backward products on the exact engine, as before (one launch each)"""
    bwd, _ = _linear_case(L, dev, 130, 4, 64, "sigmoid")
    assert bwd["gemm_f32"] == 2 and bwd["tn_tail"] == 0, bwd
    assert all(bwd[r] == 0 for r in ROUTES if r != "gemm_f32"), bwd


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. option "deterministic"
def test_odd_width_model_under_the_deterministic_option(dev, deterministic):
    """meant(100, 50) with MEANT_DETERMINISTIC=1 set through the option API: completes, matches the oracle, and two runs give the same
    bits for every parameter's gradient except the embedding table's (its gradient stays on the float-atomics kernel at d % 8 != 0)"""
    assert deterministic.get_option("deterministic") == 1
    grads = []
    for _ in range(2):
        hip = _model_case("meant", 100, 50, 2, BF, dev)
        grads.append({k: p.grad.detach().clone() for k, p in hip.named_parameters() if p.grad is not None})
    assert grads[0] and set(grads[0]) == set(grads[1])
    for k in grads[0]:
        if k != "embedding.0.weight":
            assert torch.equal(grads[0][k], grads[1][k]), k
