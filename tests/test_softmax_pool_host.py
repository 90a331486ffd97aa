"""The learned softmax pooling (csrc/softpool.hip, ops.softmax_pool, meantTweetPrice) as far as it can be held without a GPU: the closed
forms the backward kernels evaluate against autograd on the fp64 reference, the C ABI's declarations and argument checks, the model's
parameter names and shapes against lists typed from the fork, and the Python-level argument errors."""
import ctypes
import os
import re

import pytest
import torch

from tests import softpool_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("meant_ln_gelu_dot_fwd", "meant_softmax_pool_fwd", "meant_softmax_pool_bwd", "meant_ln_gelu_dot_bwd")


# ---- closed forms ------------------------------------------------------------------------------------------------------------------
def _closed_forms(case, key_mask):
    """dscore and the direct path of dx as meant_softmax_pool_bwd forms them, from the reference's own weights, against autograd with
    the scores as a leaf"""
    x = case["x"]
    score = R.scores(x, *[case[k] for k in R.PARAMS]).detach().requires_grad_(True)
    xl = x.detach().clone().requires_grad_(True)
    w = R.weights_of(score, key_mask)
    out = (w.unsqueeze(-1) * xl).sum(dim=1)
    dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    out.backward(dout)
    w = w.detach()
    r = (x * dout.unsqueeze(1)).sum(dim=-1)                                     # row dots x[g, s, :] . dout[g, :]
    dscore = w * (r - (w * r).sum(dim=1, keepdim=True))
    dx_direct = w.unsqueeze(-1) * dout.unsqueeze(1)
    return dscore, score.grad, dx_direct, xl.grad


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
def test_closed_forms_match_autograd(masked):
    case = R.make_case(3, 7, 12, seed=3, w2_scale=4.0)
    km = None
    if masked:
        km = (torch.rand(3, 7, generator=torch.Generator().manual_seed(9)) > 0.4).double()
        km[0] = 0                                                                # one sequence left out completely
        km[1, 2] = 1
    dscore, dscore_ad, dxd, dxd_ad = _closed_forms(case, km)
    assert (dscore - dscore_ad).abs().max().item() <= 1e-12
    assert (dxd - dxd_ad).abs().max().item() <= 1e-12
    if masked:
        assert dscore[0].abs().max().item() == 0 and dxd[0].abs().max().item() == 0


def test_b2_gradient_is_zero():
    case = R.make_case(2, 9, 8, seed=1, w2_scale=4.0)
    _, _, grads, _ = R.run_ref(case)
    assert grads["b2"].abs().max().item() <= 1e-12
    assert grads["w2"].abs().max().item() > 1e-3                                 # the test would pass on a dead graph otherwise


def test_reference_all_masked_is_zero_and_finite():
    case = R.make_case(2, 5, 8)
    km = torch.ones(2, 5)
    km[1] = 0
    out, w, grads, _ = R.run_ref(case, key_mask=km)
    assert out[1].abs().max().item() == 0 and w[1].abs().max().item() == 0
    assert all(torch.isfinite(g).all() for g in grads.values())
    assert grads["x"][1].abs().max().item() == 0


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entries():
    import meant_amd._lib as L
    with open(os.path.join(ROOT, "include", "meant_hip.h")) as f:
        src = f.read()
    for fn in ENTRIES:
        assert re.search(r"\bint\s+" + fn + r"\s*\(", src), f"{fn} is not declared in include/meant_hip.h"
        assert fn in L.SIGNATURES
        assert getattr(L.lib, fn) is not None
    assert len(L.SIGNATURES["meant_softmax_pool_fwd"][1]) == 14
    assert len(L.SIGNATURES["meant_softmax_pool_bwd"][1]) == 13
    assert len(L.SIGNATURES["meant_ln_gelu_dot_fwd"][1]) == 12
    assert len(L.SIGNATURES["meant_ln_gelu_dot_bwd"][1]) == 16
    raw = ctypes.CDLL(L.LIB_PATH)
    for fn in ENTRIES:
        assert hasattr(raw, fn), f"{fn} is not exported by the built library"


P = 0x10000          # a non-null, 16-byte aligned address: every check below fails before anything is launched or dereferenced


def _fwd_ln(rows=4, d=8, dtype=0):
    import meant_amd._lib as L
    return L.lib.meant_ln_gelu_dot_fwd(P, P, P, P, P, P, P, rows, d, 1e-5, dtype, None)


def _bwd_ln(rows=4, d=8, dtype=0):
    import meant_amd._lib as L
    return L.lib.meant_ln_gelu_dot_bwd(P, P, P, P, P, P, P, P, P, P, rows, d, dtype, P, 1 << 30, None)


def _fwd_pool(G=2, S=4, d=8, dtype=0, out_dtype=0, mask=None, kind=0, ld=8, off=0):
    import meant_amd._lib as L
    return L.lib.meant_softmax_pool_fwd(P, P, mask, kind, P, P, ld, off, G, S, d, dtype, out_dtype, None)


def _bwd_pool(G=2, S=4, d=8, dtype=0, out_dtype=0, ld=8, off=0):
    import meant_amd._lib as L
    return L.lib.meant_softmax_pool_bwd(P, ld, off, P, P, P, P, G, S, d, dtype, out_dtype, None)


@pytest.mark.parametrize("call", [
    lambda: _fwd_ln(rows=0), lambda: _fwd_ln(rows=-1), lambda: _fwd_ln(d=0), lambda: _fwd_ln(d=-8), lambda: _fwd_ln(dtype=7),
    lambda: _bwd_ln(rows=0), lambda: _bwd_ln(d=0), lambda: _bwd_ln(dtype=2),
    lambda: _fwd_pool(S=0), lambda: _fwd_pool(S=-3), lambda: _fwd_pool(G=0), lambda: _fwd_pool(d=0), lambda: _fwd_pool(dtype=5),
    lambda: _fwd_pool(out_dtype=9), lambda: _fwd_pool(mask=P, kind=5), lambda: _fwd_pool(mask=P, kind=-1), lambda: _fwd_pool(ld=8, off=4),
    lambda: _bwd_pool(S=0), lambda: _bwd_pool(G=0), lambda: _bwd_pool(d=-1), lambda: _bwd_pool(dtype=3), lambda: _bwd_pool(ld=4),
])
def test_bad_arguments_are_rejected_before_any_launch(call):
    import meant_amd._lib as L
    assert call() == L.ERR_ARG
    assert L.lib.meant_last_error()


def test_workspace_too_small_is_rejected():
    import meant_amd._lib as L
    need = L.lib.meant_ln_gelu_dot_bwd_ws(1000, 768)
    assert need == 3 * 250 * 768 * 4
    assert L.lib.meant_ln_gelu_dot_bwd_ws(10 ** 6, 768) == 3 * 1024 * 768 * 4            # the partial rows are bounded
    assert L.lib.meant_ln_gelu_dot_bwd(P, P, P, P, P, P, P, P, P, P, 1000, 768, 0, P, need - 1, None) == L.ERR_WORKSPACE


# ---- the model's surface -----------------------------------------------------------------------------------------------------------
def _language_encoder_keys(prefix, d):
    """src/meant/meant_tweet_price.py:28-68: xPos (RotaryEmbedding(dim=48, use_xpos=True): the frozen `freqs` parameter, 24 values),
    encode = [RMSNorm, Linear, xPosAttention, RMSNorm, Dropout, Linear], encode2 = [RMSNorm, Linear, GELU, RMSNorm, Dropout, Linear];
    the attention registers multi_mad, q, v, k and shares the encoder's xPos (src/meant/xPosAttention.py) -- the same object, which
    named_parameters() lists once, under the encoder's own name"""
    keys = {prefix + "xPos.freqs": (24,)}
    for name in ("encode.0", "encode.3", "encode2.0", "encode2.3"):
        keys[prefix + name + ".scale"] = (d,)
    for name in ("encode.1", "encode.5", "encode2.1", "encode2.5", "encode.2.multi_mad", "encode.2.q", "encode.2.v", "encode.2.k"):
        keys[prefix + name + ".weight"] = (d, d)
        keys[prefix + name + ".bias"] = (d,)
    return keys


def _expected_parameters(text_dim, price_dim, lag, num_classes, vocab, pool, num_encoders=1, num_temporal_encoders=1):
    dim = text_dim + price_dim
    keys = {"txt_classtkn": (1, lag, 1, text_dim), "embedding.0.weight": (vocab, text_dim)}             # :176, :165
    for i in range(num_encoders):                                                                         # :170
        keys.update(_language_encoder_keys(f"languageEncoders.{i}.", text_dim))
    for j in range(num_temporal_encoders):                                                                # :172, :113-128
        p = f"temporal_encoding.{j}."
        keys[p + "temp_embedding"] = (1, lag, dim)
        keys[p + "temp_encode.0.scale"] = (dim,)
        keys[p + "temp_encode.3.scale"] = (dim,)
        for name in ("temp_encode.1", "temp_encode.5", "temp_encode.2.multi_mad", "temp_encode.2.q", "temp_encode.2.v", "temp_encode.2.k"):
            keys[p + name + ".weight"] = (dim, dim)
            keys[p + name + ".bias"] = (dim,)
    keys.update({"mlpHead.0.weight": (dim,), "mlpHead.0.bias": (dim,), "mlpHead.1.weight": (num_classes, dim),     # :174
                 "mlpHead.1.bias": (num_classes,)})
    if pool == "softmax":                                                                                 # src/meant/meant_tweet.py:173
        keys.update({"lang_prep.0.weight": (text_dim, text_dim), "lang_prep.0.bias": (text_dim,), "lang_prep.1.weight": (text_dim,),
                     "lang_prep.1.bias": (text_dim,), "lang_prep.3.weight": (1, text_dim), "lang_prep.3.bias": (1,)})
    return keys


@pytest.mark.parametrize("pool", ["mean", "softmax"])
def test_parameter_names_and_shapes(pool):
    import meant_amd
    m = meant_amd.meantTweetPrice(128, 4, 3, 2, torch.nn.Embedding(97, 128), sequence_length=16, num_heads=4, num_encoders=2,
                                  num_temporal_encoders=2, pool=pool)
    got = {k: tuple(p.shape) for k, p in m.named_parameters()}
    assert got == _expected_parameters(128, 4, 3, 2, 97, pool, 2, 2)
    assert isinstance(m.lang_prep[4], torch.nn.Softmax) if pool == "softmax" else not hasattr(m, "lang_prep")
    assert m.mask_pool is False


def test_constructor_signature_is_the_forks():
    import inspect
    import meant_amd
    sig = inspect.signature(meant_amd.meantTweetPrice.__init__)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[1:]] == [
        ("text_dim", inspect.Parameter.empty), ("price_dim", inspect.Parameter.empty), ("lag", inspect.Parameter.empty),
        ("num_classes", inspect.Parameter.empty), ("embedding", inspect.Parameter.empty), ("sequence_length", 128), ("flash", False),
        ("num_heads", 8), ("num_encoders", 1), ("num_temporal_encoders", 1), ("channels", 4), ("pool", "mean")]


def test_dropin_exports_the_class():
    import sys
    import meant_amd
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        import meant
        from meant.meant_tweet_price import meantTweetPrice
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
    assert meantTweetPrice is meant_amd.meantTweetPrice is meant.meantTweetPrice


def test_argument_errors():
    import meant_amd
    emb = lambda: torch.nn.Embedding(11, 16)
    with pytest.raises(ValueError, match="pool"):
        meant_amd.meantTweetPrice(16, 2, 3, 2, emb(), pool="cls")
    m = meant_amd.meantTweetPrice(16, 2, 3, 2, emb(), sequence_length=8, num_heads=2, pool="softmax")
    ids = torch.zeros(2, 3, 5, dtype=torch.int64)
    with pytest.raises(ValueError, match="sequence_length"):
        m(ids, torch.zeros(2, 3, 2))
    with pytest.raises(ValueError, match="prices"):
        m(torch.zeros(2, 3, 8, dtype=torch.int64), torch.zeros(2, 3, 5))
    m.pool = "max"
    with pytest.raises(ValueError, match="pool"):
        m(torch.zeros(2, 3, 8, dtype=torch.int64), torch.zeros(2, 3, 2))
    x = torch.zeros(2, 4, 8)
    with pytest.raises(ValueError, match="G, S, d"):
        meant_amd.ops.softmax_pool(x[0], *[torch.zeros(1)] * 6)
    with pytest.raises(ValueError, match="shapes"):
        meant_amd.ops.softmax_pool(x, torch.zeros(8, 4), torch.zeros(8), torch.zeros(8), torch.zeros(8), torch.zeros(1, 8), torch.zeros(1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        meant_amd.ops.softmax_pool(x, torch.zeros(8, 8), torch.zeros(8), torch.zeros(8), torch.zeros(8), torch.zeros(1, 8), torch.zeros(1))
