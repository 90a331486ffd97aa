"""bench.py --dump-outputs, host side (no GPU): what dump_outputs writes, its size bound and its fixed gradient sample."""
import os
import zlib

import numpy as np
import torch

import bench


def _model_with_grads():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Embedding(3000, 200), torch.nn.Linear(200, 2))
    out = torch.softmax(m(torch.randint(0, 3000, (8, 5))).mean(1), -1)
    loss = -out[:, 0].log().mean()
    loss.backward()
    return m, out, loss


def test_dump_outputs_writes_float32_within_budget(tmp_path, monkeypatch):
    m, out, loss = _model_with_grads()
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 20)            # 600 000 embedding-gradient elements do not fit: sampled
    bench.dump_outputs(str(tmp_path), m, [out[:4], out[4:]], loss)
    names = sorted(os.listdir(tmp_path))
    assert names == sorted(["out.npy", "loss.npy"] + [f"grad.{k}.npy" for k, _ in m.named_parameters()])
    arrays = {n[:-4]: np.load(tmp_path / n) for n in names}
    assert all(a.dtype == np.float32 for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 1 << 20
    np.testing.assert_array_equal(arrays["out"], out.detach().numpy())
    assert arrays["loss"].shape == () and arrays["loss"] == loss.item()
    np.testing.assert_array_equal(arrays["grad.1.weight"], m[1].weight.grad.numpy())    # small: whole, in its own shape
    g = arrays["grad.0.weight"]
    assert g.ndim == 1 and 0 < g.size < m[0].weight.numel()
    idx = np.sort(np.random.default_rng(zlib.crc32(b"0.weight")).choice(m[0].weight.numel(), g.size, replace=False))
    np.testing.assert_array_equal(g, m[0].weight.grad.reshape(-1).numpy()[idx])


def test_dump_outputs_sample_is_the_same_every_run(tmp_path):
    m, out, loss = _model_with_grads()
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), m, [out], loss)
    for n in os.listdir(tmp_path / "a"):
        np.testing.assert_array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n))
