"""fp64 reference of the learned softmax pooling (src/meant/meant_tweet.py:173,259-261) for the softmax-pool tests:
lang_prep = Linear(d, d) -> LayerNorm(d) -> GELU -> Linear(d, 1) -> Softmax over the sequence, pooled = sum_s w_s x_s.
Plain torch on the CPU; gradients come from autograd."""
import torch
import torch.nn.functional as F

PARAMS = ("w1", "b1", "gamma", "beta", "w2", "b2")


def make_case(G, S, d, seed=0, w2_scale=1.0):
    """x [G, S, d] and the six parameters in float64, seeded; w2_scale sharpens the softmax"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    return dict(x=r(G, S, d), w1=r(d, d) / d ** 0.5, b1=0.1 * r(d), gamma=1.0 + 0.1 * r(d), beta=0.1 * r(d),
                w2=w2_scale * r(1, d) / d ** 0.5, b2=0.1 * r(1))


def scores(x, w1, b1, gamma, beta, w2, b2, eps=1e-5):
    h = F.linear(x, w1, b1)
    n = F.layer_norm(h, (x.shape[-1],), gamma, beta, eps)
    return F.linear(F.gelu(n), w2, b2).squeeze(-1)                       # [G, S]


def weights_of(score, key_mask=None):
    """softmax over the positions the mask keeps; a sequence with nothing kept gets all-zero weights"""
    if key_mask is None:
        return torch.softmax(score, dim=1)
    keep = key_mask != 0
    w = torch.softmax(score.masked_fill(~keep, float("-inf")), dim=1)
    return torch.where(keep.any(dim=1, keepdim=True), w, torch.zeros_like(w))


def softmax_pool_ref(x, w1, b1, gamma, beta, w2, b2, key_mask=None, eps=1e-5):
    """(pooled [G, d], w [G, S]) in the dtype of x"""
    w = weights_of(scores(x, w1, b1, gamma, beta, w2, b2, eps), key_mask)
    return (w.unsqueeze(-1) * x).sum(dim=1), w


def run_ref(case, key_mask=None, dout=None, eps=1e-5):
    """forward and backward of the reference on a make_case dict: (pooled, w, {name: gradient} for x and the parameters).
    dout: the gradient of pooled (seeded normal if None)."""
    leaves = {k: v.detach().clone().double().requires_grad_(True) for k, v in case.items()}
    out, w = softmax_pool_ref(leaves["x"], *[leaves[k] for k in PARAMS], key_mask=key_mask, eps=eps)
    if dout is None:
        dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(1234), dtype=torch.float64)
    out.backward(dout.double())
    return out.detach(), w.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}, dout
