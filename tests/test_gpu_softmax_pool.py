"""ops.softmax_pool (csrc/softpool.hip: meant_ln_gelu_dot_fwd / _bwd, meant_softmax_pool_fwd / _bwd around the library's Linear) against
the fp64 reference of tests/softpool_ref.py, in both tiers, with the project's tolerances (tests/util.py TOL): outputs by max-abs,
gradient norms relative with norm_floor, gradient elements relative to the tensor's largest.  The reference of a case is computed once per tier (on the CPU, in float64, on
the x the tier stores) and shared by the tests that use the case."""
import functools

import pytest
import torch

from tests import softpool_ref as R
from tests.util import TOL, DTYPES, IDS, assert_close, assert_grad_close, norm_floor

pytestmark = pytest.mark.gpu

# (G, S, d): one position (w = 1, dscore = 0); a few; S past one wave with element access; the model's width; S past a 512 block;
# the wide norm form (d > 2048)
SHAPES = [(3, 1, 8), (3, 5, 8), (2, 70, 100), (5, 64, 768), (2, 513, 128), (2, 16, 2056)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _mask(kind, G, S):
    if kind is None:
        return None
    if kind == "random":
        km = (torch.rand(G, S, generator=torch.Generator().manual_seed(7)) > 0.4).float()
        km[:, 0] = 1
        return km
    if kind == "one":                                            # exactly one position kept per sequence
        km = torch.zeros(G, S)
        for g in range(G):
            km[g, (3 * g + 1) % S] = 1
        return km
    km = torch.ones(G, S)                                        # "dead": sequence 1 masked completely
    km[1] = 0
    km[0, S // 2:] = 0
    return km


@functools.lru_cache(maxsize=None)
def _reference(G, S, d, w2_scale, mask_kind):
    case = R.make_case(G, S, d, seed=0, w2_scale=w2_scale)
    return case, _mask(mask_kind, G, S)


def _run_hip(case, km, dout, dtype, dev, out=None, col_off=0):
    """(pooled or the buffer, {name: gradient}) of ops.softmax_pool on the case's tensors: x in the tier's dtype, fp32 parameters"""
    import meant_amd
    leaves = {k: v.to(dev, torch.float32).requires_grad_(True) for k, v in case.items() if k != "x"}
    x = case["x"].to(dev, dtype).requires_grad_(True)
    res = meant_amd.ops.softmax_pool(x, *[leaves[k] for k in R.PARAMS], key_mask=None if km is None else km.to(dev), out=out,
                                     col_off=col_off)
    d = x.shape[-1]
    pooled = res if out is None else res[:, col_off:col_off + d]
    pooled.backward(dout.to(dev, pooled.dtype))
    torch.cuda.synchronize()
    leaves["x"] = x
    return res, {k: v.grad for k, v in leaves.items()}


def _x_in_tier(case, dtype):
    """the case with x rounded to the tier's storage type, which is what the device is given: the reference must see the same x"""
    c = dict(case)
    c["x"] = case["x"].to(dtype).double()
    return c


@functools.lru_cache(maxsize=None)
def _reference_tier(G, S, d, w2_scale, mask_kind, dtype):
    case, km = _reference(G, S, d, w2_scale, mask_kind)
    case = _x_in_tier(case, dtype)
    out, w, grads, dout = R.run_ref(case, key_mask=km)
    return case, km, out, w, grads, dout


def _compare(out, grads, ref_out, ref_grads, dtype, what):
    tol = TOL[dtype]
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    print(f"{what}: out err {(out.detach().double().cpu() - ref_out).abs().max().item():.3e}")
    assert_close(out, ref_out, tol["out"], f"{what}: pooled")
    floor = norm_floor([g.norm().item() for g in ref_grads.values()], dtype)
    for k, r in ref_grads.items():
        g = grads[k]
        assert g is not None, f"{what}: {k} has no gradient"
        assert torch.isfinite(g).all(), f"{what}: non-finite gradient of {k}"
        a, b = g.detach().double().cpu().norm().item(), r.norm().item()
        print(f"{what}: {k} grad norm {a:.6e} vs {b:.6e}")
        assert abs(a - b) <= tol["gnorm"] * max(b, floor) + 1e-7, f"{what}: {k} grad norm {a} vs {b}"
        if b > floor:
            assert_grad_close(g, r, tol["gelem"], f"{what}: {k}")
    assert grads["b2"].abs().max().item() == 0, f"{what}: the gradient of b2 is exactly zero"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_fp64(shape, dtype, dev):
    case, km, ref_out, ref_w, ref_grads, dout = _reference_tier(*shape, 1.0, None, dtype)
    out, grads = _run_hip(case, km, dout, dtype, dev)
    assert out.dtype == torch.float32 and tuple(out.shape) == (shape[0], shape[2])
    _compare(out, grads, ref_out, ref_grads, dtype, f"softmax_pool{shape}")
    if shape[1] == 1:                                             # one position: w = 1, the pooled row is x itself, the scores get no gradient
        assert torch.equal(out.cpu(), case["x"][:, 0].float())
        for k in ("w1", "b1", "gamma", "beta", "w2"):
            assert grads[k].abs().max().item() == 0, k


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_peaked(dtype, dev):
    """w2 scaled by 4: the largest weight of each sequence is above 0.3 at S = 70 (0.59 and 0.50 for seed 0 of softpool_ref.make_case;
    uniform weights would be 0.014), so an error in the softmax cannot hide behind near-uniform weights"""
    case, km, ref_out, ref_w, ref_grads, dout = _reference_tier(2, 70, 100, 4.0, None, dtype)
    assert ref_w.max(dim=1).values.min().item() > 0.3, ref_w.max(dim=1).values
    out, grads = _run_hip(case, km, dout, dtype, dev)
    _compare(out, grads, ref_out, ref_grads, dtype, "peaked")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mask_kind", ["random", "one", "dead"])
@pytest.mark.parametrize("shape", [(3, 70, 100), (3, 64, 128)], ids=["3x70x100", "3x64x128"])
def test_masks(shape, mask_kind, dtype, dev):
    case, km, ref_out, ref_w, ref_grads, dout = _reference_tier(*shape, 4.0, mask_kind, dtype)
    out, grads = _run_hip(case, km, dout, dtype, dev)
    _compare(out, grads, ref_out, ref_grads, dtype, f"mask[{mask_kind}]{shape}")
    if mask_kind == "dead":                                      # a sequence with nothing kept: zeros, not NaN, forward and backward
        assert out[1].abs().max().item() == 0
        assert grads["x"][1].abs().max().item() == 0
    if mask_kind == "one":                                       # the one kept row, bit for bit
        G, S, _ = shape
        for g in range(G):
            assert torch.equal(out[g].cpu(), case["x"][g, (3 * g + 1) % S].float())


@pytest.mark.parametrize("mask_dtype", [torch.bool, torch.int64, torch.int32, torch.uint8, torch.bfloat16, torch.float16])
def test_mask_dtypes_give_the_same_bits(mask_dtype, dev):
    import meant_amd
    case, km, *_ = _reference(3, 70, 100, 4.0, "random")
    args = [case["x"].to(dev, torch.float32)] + [case[k].to(dev, torch.float32) for k in R.PARAMS]
    a = meant_amd.ops.softmax_pool(*args, key_mask=km.to(dev))
    b = meant_amd.ops.softmax_pool(*args, key_mask=km.to(dev).to(mask_dtype))
    assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(5, 64, 768), (2, 70, 100)], ids=["5x64x768", "2x70x100"])
def test_concat_placement(shape, dtype, dev):
    """out with ld_out = d + 4, col_off = 0: the pooled columns equal the plain call's bits, the four other columns are bit-unchanged"""
    G, S, d = shape
    case, km, ref_out, ref_w, ref_grads, dout = _reference_tier(G, S, d, 1.0, None, dtype)
    plain, grads_plain = _run_hip(case, km, dout, dtype, dev)
    buf = torch.full((G, d + 4), -7.25, device=dev)
    res, grads = _run_hip(case, km, dout, dtype, dev, out=buf, col_off=0)
    assert res.data_ptr() == buf.data_ptr()
    assert torch.equal(buf[:, :d], plain)
    assert torch.equal(buf[:, d:], torch.full((G, 4), -7.25, device=dev))
    _compare(buf[:, :d], grads, ref_out, ref_grads, dtype, f"concat{shape}")      # the backward reads its columns of the buffer's gradient


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("pads", [(3, 2), (8, 8)], ids=["elem", "vec"])        # columns left / right of the pooled ones: (8, 8) keeps the 16-byte form
@pytest.mark.parametrize("shape", [(2, 70, 100), (5, 64, 768), (2, 16, 2056)], ids=lambda s: "x".join(map(str, s)))
def test_deterministic_and_no_stray_writes(shape, pads, dtype, dev):
    """two runs are bit-identical, and the entries write nothing at or beyond column d of a row: every output lives in a buffer whose
    guard elements (behind the last row / around the pooled columns) keep their sentinel"""
    import meant_amd
    from meant_amd import _lib as L
    lib, st = L.lib, torch.cuda.current_stream().cuda_stream
    G, S, d = shape
    T = G * S
    case, km, *_ = _reference(G, S, d, 4.0, None)
    kmd = _mask("random", G, S).to(dev)
    dt = L.F32 if dtype == torch.float32 else L.BF16
    x = case["x"].to(dev, dtype).contiguous()
    h = (case["x"] @ case["w1"].T + case["b1"]).to(dev, dtype).view(T, d).contiguous()
    g, b, u, b2 = (case[k].to(dev, torch.float32).contiguous().view(-1) for k in ("gamma", "beta", "w2", "b2"))
    SENT, PAD = 12288.0, 64                                       # exact in bfloat16
    off, ld = pads[0], d + pads[0] + pads[1]

    def guarded(n, dtype_):
        t = torch.full((n + PAD,), SENT, device=dev, dtype=dtype_)
        return t, t[:n]

    def run():
        score_g, score = guarded(T, torch.float32)
        stats_g, stats = guarded(2 * T, torch.float32)
        w_g, w = guarded(T, torch.float32)
        out = torch.full((G, ld), SENT, device=dev)
        L.check(lib.meant_ln_gelu_dot_fwd(h.data_ptr(), g.data_ptr(), b.data_ptr(), u.data_ptr(), b2.data_ptr(), score.data_ptr(),
                                          stats.data_ptr(), T, d, 1e-5, dt, st))
        L.check(lib.meant_softmax_pool_fwd(x.data_ptr(), score.data_ptr(), kmd.data_ptr(), L.MASK_F32, w.data_ptr(), out.data_ptr(), ld, off,
                                           G, S, d, dt, L.F32, st))
        dout = torch.full((G, ld), float("nan"), device=dev)          # outside the pooled columns: never read
        dout[:, off:off + d] = torch.randn(G, d, generator=torch.Generator().manual_seed(3)).to(dev)
        dx_g, dx = guarded(T * d, dtype)
        ds_g, ds = guarded(T, torch.float32)
        L.check(lib.meant_softmax_pool_bwd(dout.data_ptr(), ld, off, x.data_ptr(), w.data_ptr(), dx.data_ptr(), ds.data_ptr(), G, S, d, dt,
                                           L.F32, st))
        dh_g, dh = guarded(T * d, dtype)
        pg = [guarded(d, torch.float32) for _ in range(3)]
        wsb = lib.meant_ln_gelu_dot_bwd_ws(T, d)
        ws_g, ws = guarded(wsb // 4, torch.float32)
        L.check(lib.meant_ln_gelu_dot_bwd(ds.data_ptr(), h.data_ptr(), stats.data_ptr(), g.data_ptr(), b.data_ptr(), u.data_ptr(), dh.data_ptr(),
                                          pg[0][1].data_ptr(), pg[1][1].data_ptr(), pg[2][1].data_ptr(), T, d, dt, ws.data_ptr(), wsb, st))
        torch.cuda.synchronize()
        return [score_g, stats_g, w_g, out, dx_g, ds_g, dh_g, ws_g] + [p[0] for p in pg]

    first, second = run(), run()
    for i, (a, c) in enumerate(zip(first, second)):
        if i != 7:                                               # the workspace's unused partial rows hold whatever they held
            assert torch.equal(a, c), f"buffer {i} differs between two runs"
            assert torch.isfinite(a.float()).all(), f"buffer {i} holds a non-finite value"
    for i, a in enumerate(first):
        if i == 3:
            assert (a[:, :off] == SENT).all() and (a[:, off + d:] == SENT).all(), "pooled buffer written outside its columns"
            assert (a[:, off:off + d] != SENT).all()
        else:
            assert (a[-PAD:].float() == SENT).all(), f"buffer {i} written past its end"
