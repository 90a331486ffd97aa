"""Models whose widths reach the one-row-per-workgroup norm kernels: meant(text_dim + image_dim > 2048) builds RMSNorm(2304) for its
temporal encoder and head, meant_vision(image_dim > 2048) a LayerNorm head of that width, and a languageEncoder wider than 2048
runs every one of its norms (the train-mode dropout norm included) there.  Against the CPU oracle, both tiers."""
import numpy as np
import pytest
import torch

from tests.util import DTYPES, IDS, TOL, t, assert_close, pair, compare_param_grads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _mk(cls_name, args, kw, emb, dev):
    import meant_amd
    from oracle import meant_oracle as O
    a = list(args)
    ref = getattr(O, cls_name)(*(a + ([torch.nn.Embedding(*emb)] if emb else [])), **kw)
    hip = getattr(meant_amd, cls_name)(*(a + ([torch.nn.Embedding(*emb)] if emb else [])), **kw)
    return pair(ref, hip, 1234, dev)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("heads", [8, 16])
def test_meant_text_1024_image_1280(dev, dtype, heads):
    """meant(1024, 1280): RMSNorm(2304) three times (temporal encoder x2, head); at 8 heads the vision head dim is 160 (the fp32
    attention core) and the temporal one 288, at 16 heads 80 and 144"""
    ref, hip = _mk("meant", (1024, 1280, 4, 32, 32, 16, 2, 3), dict(num_heads=heads, num_encoders=1, channels=4), (100, 1024), dev)
    r = np.random.RandomState(heads)
    ids = t(r.randint(0, 100, (2, 2, 16)).astype("int64"))
    img = t(r.standard_normal((2, 2, 4, 32, 32)).astype("float32"))
    mask = torch.ones(2, 2, 16)
    mask[1, :, 11:] = 0
    tgt = torch.tensor([2, 0])
    out_r = ref(ids, img, mask)
    loss_r = torch.nn.functional.cross_entropy(out_r, tgt)
    loss_r.backward()
    hip.compute_dtype = dtype
    out = hip(ids.to(dev), img.to(dev), mask.to(dev))
    loss = torch.nn.functional.cross_entropy(out, tgt.to(dev))
    loss.backward()
    assert_close(out, out_r, TOL[dtype]["out"], "out")
    assert abs(loss.item() - loss_r.item()) <= TOL[dtype]["out"]
    compare_param_grads(ref, hip, dtype, f"meant_1024_1280_h{heads}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_meant_vision_2560_layernorm_head(dev, dtype):
    """meant_vision(image_dim=2560): its head is LayerNorm(2560)"""
    ref, hip = _mk("meant_vision", (2560, 4, 32, 32, 16, 3, 2), dict(num_heads=20, num_encoders=1, channels=4), None, dev)
    r = np.random.RandomState(5)
    img = t(r.standard_normal((2, 3, 4, 32, 32)).astype("float32"))
    tgt = torch.tensor([1, 0])
    out_r = ref(img)
    loss_r = torch.nn.functional.cross_entropy(out_r, tgt)
    loss_r.backward()
    hip.compute_dtype = dtype
    out = hip(img.to(dev))
    loss = torch.nn.functional.cross_entropy(out, tgt.to(dev))
    loss.backward()
    assert_close(out, out_r, TOL[dtype]["out"], "out")
    assert abs(loss.item() - loss_r.item()) <= TOL[dtype]["out"]
    compare_param_grads(ref, hip, dtype, "meant_vision_2560")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_language_encoder_2560_train_mode_dropout_norm(dev, dtype, monkeypatch):
    """languageEncoder(2560, 20) in .train(): the default-p Dropout() of encode2[4] rides encode2[3]'s RMSNorm kernel
    (ops.linear_gelu_rmsnorm, meant/meant.py:105-107).  The reference is the eager fp32 encoder with the kernel's mask, read back
    from the plain norm at the same [rows, 2560] shape and seed, applied after encode2[3]."""
    import meant_amd
    from meant_amd import modules
    from oracle import meant_oracle as O
    from tests.test_gpu_bench_path import _mask_of
    d, heads, B, S, seed = 2560, 20, 2, 24, 31337
    monkeypatch.setattr(modules, "_seed", lambda: seed)
    ref, hip = pair(O.languageEncoder(d, heads), meant_amd.languageEncoder(d, heads), 1234, dev)
    hip.train()
    p = hip.encode2[4].p
    assert p == 0.5 and hip.encode[4].p == 0.0
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(B, S, d, generator=gen)
    w = torch.randn(B, S, d, generator=gen)
    mask = _mask_of(B * S, d, p, seed, dev).view(B, S, d).cpu()

    xr = x.to(dtype).float()
    h = xr
    for m in ref.encode:
        h = m(h, None) if isinstance(m, O.xPosAttention) else m(h)
    x1 = h + xr
    e2 = ref.encode2
    y_r = e2[3](torch.nn.functional.gelu(e2[1](e2[0](x1)))) * mask
    out_r = e2[5](y_r) + x1
    (out_r * w).sum().backward()

    out = hip(x.to(dev).to(dtype))
    (out.float() * w.to(dev)).sum().backward()
    assert out.dtype == dtype
    tol = TOL[dtype]
    assert_close(out, out_r, tol["out"] * max(1.0, out_r.abs().max().item()), "out")
    compare_param_grads(ref, hip, dtype, "languageEncoder_2560_train")
