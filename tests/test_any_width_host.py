"""Host-side facts of the any-width path (no GPU): which output widths of a bf16 Linear move their backward onto the MFMA kernels,
the norm ops' default width rule, the weight cache's zero-padded transposed entry (the copy kernels replaced by host stand-ins that
keep their contracts), and the argument checks of the three element-wise entry points that now take any width."""
import ctypes

import numpy as np
import pytest
import torch


def test_which_output_widths_are_padded():
    from meant_amd import ops
    bf, f32 = torch.bfloat16, torch.float32
    for N in (9, 100, 150, 588, 1001):
        assert ops._n_pad_ok(N, bf) and not ops._n_pad_ok(N, f32)
    for N in (1, 4, 7):                                        # class heads stay on the exact engine
        assert not ops._n_pad_ok(N, bf)
    for N in (8, 96, 768, 1536):                               # what ran on the MFMA kernels already
        assert not ops._n_pad_ok(N, bf) and not ops._n_pad_ok(N, f32)


def test_norm_ops_keep_their_default_width_rule():
    from meant_amd import _lib, ops
    for d in (100, 99, 150, 260):
        with pytest.raises(_lib.MeantHipError, match="not a multiple of 8"):
            ops._norm_width(d, False, "rmsnorm")
        ops._norm_width(d, True, "rmsnorm")
    ops._norm_width(768, False, "rmsnorm")
    x, g = torch.zeros(2, 100), torch.ones(100)
    for call in (lambda: ops.rmsnorm(x, g), lambda: ops.rmsnorm_fork(x, g), lambda: ops.layernorm(x, g, g),
                 lambda: ops.linear_gelu_rmsnorm(torch.zeros(2, 64), torch.zeros(100, 64), None, g)):
        with pytest.raises(_lib.MeantHipError, match="not a multiple of 8"):
            call()


class _HostCopies:
    """meant_transpose2d / meant_pad_copy2d / meant_cast on host memory, float only, by the contracts of include/meant_hip.h"""

    @staticmethod
    def _arr(ptr, n):
        return np.ctypeslib.as_array((ctypes.c_float * n).from_address(ptr))

    def meant_transpose2d(self, src, ds, dst, dd, rows, cols, stream):
        self._arr(dst, rows * cols).reshape(cols, rows)[:] = self._arr(src, rows * cols).reshape(rows, cols).T
        return 0

    def meant_pad_copy2d(self, src, ld_src, cols_src, ds, dst, ld_dst, cols_dst, dd, rows, stream):
        s = self._arr(src, rows * ld_src).reshape(rows, ld_src)
        d = self._arr(dst, rows * ld_dst).reshape(rows, ld_dst)
        d[:, :cols_dst] = 0
        n = min(cols_src, cols_dst)
        d[:, :n] = s[:, :n]
        return 0


def test_weight_cache_padded_transposed_entry(monkeypatch):
    from meant_amd import ops
    monkeypatch.setattr(ops, "lib", _HostCopies())
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    cache = ops._WeightCache()
    N, K = 100, 50
    w = torch.nn.Parameter(torch.arange(N * K, dtype=torch.float32).view(N, K) + 1)
    plain = cache.get((w,), torch.float32, True)
    padded = cache.get((w,), torch.float32, True, pad_cols=4)
    assert plain.shape == (K, N) and padded.shape == (K, N + 4)
    assert torch.equal(plain, w.detach().t()) and torch.equal(padded[:, :N], w.detach().t())
    assert (padded[:, N:] == 0).all()
    assert len(cache) == 2                                                  # a key of its own
    assert cache.get((w,), torch.float32, True, pad_cols=4) is padded and cache.get((w,), torch.float32, True) is plain
    kpad = cache.get((w,), torch.float32, False, pad_cols=6)                # the K-side entry is a third one
    assert kpad.shape == (N, K + 6) and (kpad[:, K:] == 0).all() and torch.equal(kpad[:, :K], w.detach()) and len(cache) == 3
    with torch.no_grad():
        w.add_(1.0)                                                         # an optimizer step: the entry is rebuilt
    again = cache.get((w,), torch.float32, True, pad_cols=4)
    assert again is not padded and torch.equal(again[:, :N], w.detach().t()) and (again[:, N:] == 0).all()
    two = cache.get((w, w), torch.float32, True, pad_cols=4)                # concatenated parameters (the temporal k | v pair)
    assert two.shape == (K, 2 * N + 4) and (two[:, 2 * N:] == 0).all() and torch.equal(two[:, N:2 * N], w.detach().t())


@pytest.mark.parametrize("ld_out,col_off,d", [(150, 100, 51), (150, -1, 50), (150, 0, 0), (7, 3, 5)])
def test_meanpools_reject_slices_outside_the_row(ld_out, col_off, d):
    from meant_amd import _lib
    for fn, what in ((lambda: _lib.lib.meant_meanpool_fwd(16, 32, ld_out, col_off, 2, 3, d, _lib.F32, _lib.F32, None), b"meanpool_fwd"),
                     (lambda: _lib.lib.meant_meanpool_bwd(16, ld_out, col_off, 32, 2, 3, d, _lib.F32, _lib.F32, None), b"meanpool_bwd")):
        assert fn() != 0 and what in _lib.lib.meant_last_error()           # never dereferenced


def test_add_rowvec_rejects_bad_geometry():
    from meant_amd import _lib
    for rows, d, period in ((0, 100, 1), (4, 0, 1), (4, 100, 0)):
        assert _lib.lib.meant_add_rowvec(16, 32, 48, rows, d, period, _lib.F32, None) != 0
        assert b"add_rowvec" in _lib.lib.meant_last_error()
    assert _lib.lib.meant_embedding_fwd(16, 32, 48, 4, 0, 10, _lib.F32, None) != 0
