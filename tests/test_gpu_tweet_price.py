"""meant_amd.meantTweetPrice against a plain-torch fp64 restatement of the fork's forward (src/meant/meant_tweet_price.py:139-219, with
the learned pooling of src/meant/meant_tweet.py:173,259-261 for pool='softmax'), the same state_dict loaded on both sides.  The
language layer is the oracle's (oracle/meant_oracle.py: the fork's copy at src/meant/meant_tweet_price.py:28-81 is that layer, its
two Dropouts identities in eval mode); what the fork's Stocknet model adds is restated here, line by line."""
import math

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from oracle import meant_oracle as O
from tests.util import TOL, DTYPES, IDS, assert_close, compare_param_grads

pytestmark = pytest.mark.gpu


class RefTemporal(nn.Module):
    """src/meant/temporal.py:11-74"""

    def __init__(self, num_heads, dim):
        super().__init__()
        self.num_heads, self.dim = num_heads, dim
        self.Dh = int(dim / num_heads)                                         # :18
        self.atten_size = self.Dh * num_heads                                  # :27
        self.multi_mad = nn.Linear(self.atten_size, dim)                       # :25
        self.q = nn.Linear(dim, self.atten_size)                               # :33-35
        self.v = nn.Linear(dim, self.atten_size)
        self.k = nn.Linear(dim, self.atten_size)

    def forward(self, x):
        b, H, Dh = x.shape[0], self.num_heads, self.Dh
        q = self.q(x[:, -1, :]).view(b, 1, H, Dh).transpose(1, 2)              # :44-45 'b l (h d) -> b h l d', the last lag step
        k = self.k(x).view(b, -1, H, Dh).transpose(1, 2)                       # :45: k gives the keys, v the values
        v = self.v(x).view(b, -1, H, Dh).transpose(1, 2)
        scores = q @ k.transpose(2, 3) / math.sqrt(Dh)                         # :52
        w = torch.softmax(scores, dim=-1)                                      # :68
        inter = (w @ v).transpose(1, 2).reshape(b, self.atten_size)            # :70-72 'b h l d -> b (l h d)', l = 1
        return self.multi_mad(inter)                                           # :73


class RefTemporalEncoder(nn.Module):
    """src/meant/meant_tweet_price.py:113-136"""

    def __init__(self, dim, num_heads, lag):
        super().__init__()
        self.temp_embedding = nn.Parameter(torch.randn(1, lag, dim))           # :120
        self.temp_encode = nn.ModuleList([O.RMSNorm(dim), nn.Linear(dim, dim), RefTemporal(num_heads, dim), O.RMSNorm(dim),
                                          nn.Dropout(0.0), nn.Linear(dim, dim)])   # :121-128

    def forward(self, x):
        x += self.temp_embedding.expand(x.shape[0], -1, -1)                    # :132-133, in place on the caller's tensor
        for mod in self.temp_encode:                                           # :134-135
            x = mod(x)
        return x


class RefTweetPrice(nn.Module):
    """src/meant/meant_tweet_price.py:139-219; pool='softmax': lang_prep of src/meant/meant_tweet.py:173 in place of the mean"""

    def __init__(self, text_dim, price_dim, lag, num_classes, embedding, sequence_length=128, num_heads=8, num_encoders=1,
                 num_temporal_encoders=1, pool="mean"):
        super().__init__()
        self.lag, self.price_dim, self.seq_len = lag, price_dim, sequence_length
        self.dim = text_dim + price_dim                                        # :161
        self.embedding = nn.ModuleList([embedding])                            # :165
        self.languageEncoders = nn.ModuleList([O.languageEncoder(text_dim, num_heads) for _ in range(num_encoders)])          # :170
        self.temporal_encoding = nn.ModuleList([RefTemporalEncoder(self.dim, num_heads, lag) for _ in range(num_temporal_encoders)])   # :172
        self.mlpHead = nn.ModuleList([nn.LayerNorm(self.dim), nn.Linear(self.dim, num_classes), nn.Sigmoid()])                # :174
        self.txt_classtkn = nn.Parameter(torch.randn(1, lag, 1, text_dim))     # :176
        if pool == "softmax":                                                  # src/meant/meant_tweet.py:173
            self.lang_prep = nn.Sequential(nn.Linear(text_dim, text_dim), nn.LayerNorm(text_dim), nn.GELU(), nn.Linear(text_dim, 1),
                                           nn.Softmax(dim=2))
        self.pool = pool
        self.mask_pool = False

    def forward(self, tweets, prices, attention_mask=None):
        b = tweets.shape[0]                                                    # :185
        words = tweets.view(b * self.lag, tweets.shape[2])                     # :186
        if attention_mask is not None:
            attention_mask = attention_mask.view(b * self.lag, attention_mask.shape[2])    # :188-189
        for mod in self.embedding:                                             # :191-192
            words = mod(words)
        for enc in self.languageEncoders:                                      # :194-195
            words = enc(words, attention_mask)
        words = words.view(b, self.lag, words.shape[1], words.shape[2])        # :196
        if self.pool == "mean":
            pooled = torch.mean(words, dim=2)                                  # :208
        else:
            assert words.shape[2] == self.seq_len                              # src/meant/meant_tweet.py:250-254: nothing to pad
            if self.mask_pool:                                                 # this project's addition: padding left out of the softmax
                s = self.lang_prep[:4](words)
                keep = attention_mask.view(b, self.lag, -1, 1) != 0
                wi = torch.softmax(s.masked_fill(~keep, float("-inf")), dim=2)
            else:
                wi = self.lang_prep(words)                                     # src/meant/meant_tweet.py:259
            pooled = torch.matmul(words.transpose(2, 3), wi).squeeze(dim=-1)   # src/meant/meant_tweet.py:260-261
        temporal_input = torch.cat((pooled, prices), dim=2)                    # :208
        for enc in self.temporal_encoding:                                     # :210-211
            output = enc.forward(temporal_input)
        for mod in self.mlpHead:                                               # :216-217
            output = mod(output)
        return output.squeeze(dim=1)                                           # :219


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _batch(B, lag, S, price_dim, vocab, seed=5):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, vocab, (B, lag, S), generator=g)
    prices = torch.randn(B, lag, price_dim, generator=g, dtype=torch.float64)
    mask = torch.ones(B, lag, S)
    mask[1, :, S - 5:] = 0                                                     # padding
    mask[2, 1, 3:] = 0
    return ids, prices, mask, torch.tensor([0, 1, 1][:B])


def _pair(text_dim, price_dim, lag, heads, vocab, S, pool, dev, **kw):
    import meant_amd
    ref = RefTweetPrice(text_dim, price_dim, lag, 2, nn.Embedding(vocab, text_dim), sequence_length=S, num_heads=heads, pool=pool, **kw)
    O.fill_weights_(ref, 4321)
    ref = ref.double().eval()
    model = meant_amd.meantTweetPrice(text_dim, price_dim, lag, 2, nn.Embedding(vocab, text_dim), sequence_length=S, num_heads=heads, pool=pool,
                                      **kw)
    assert set(model.state_dict()) == set(ref.state_dict())
    model.load_state_dict(ref.state_dict())
    return ref, model.to(dev).eval()


def _check(ref, model, batch, dtype, dev, what):
    ids, prices, mask, tgt = batch
    ref.zero_grad(set_to_none=True)
    out_ref = ref(ids, prices, mask.double())
    O.cross_entropy_on_probs(out_ref, tgt).backward()
    model.compute_dtype = dtype
    model.zero_grad(set_to_none=True)
    out = model(ids.to(dev), prices.float().to(dev), mask.to(dev))
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(out_ref.shape)
    O.cross_entropy_on_probs(out, tgt.to(dev)).backward()
    torch.cuda.synchronize()
    print(f"{what}: out err {(out.detach().double().cpu() - out_ref.detach()).abs().max().item():.3e}")
    assert_close(out, out_ref, TOL[dtype]["out"], what)
    compare_param_grads(ref, model, dtype, what)
    assert model.txt_classtkn.grad is None and ref.txt_classtkn.grad is None


# 2 heads at text_dim = 128, not 4: the language layer rotates the first 48 lanes of every head (RotaryEmbedding(dim=48),
# src/meant/meant_tweet_price.py:38-42), so a head dim of 128 / 4 = 32 fails in the reference itself (a 32-wide head against 48-wide
# tables); 64 is the smallest head dim at this width that it runs at
CONFIGS = {"d128": dict(text_dim=128, price_dim=4, lag=3, heads=2, vocab=97, S=16),
           "d100": dict(text_dim=100, price_dim=3, lag=3, heads=2, vocab=97, S=16)}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("pool", ["mean", "softmax"])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_against_fp64_restatement(cfg, pool, dtype, dev):
    c = CONFIGS[cfg]
    ref, model = _pair(pool=pool, dev=dev, **c)
    _check(ref, model, _batch(3, c["lag"], c["S"], c["price_dim"], c["vocab"]), dtype, dev, f"meantTweetPrice[{cfg}, {pool}]")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_mask_pool(dtype, dev):
    c = CONFIGS["d128"]
    ref, model = _pair(pool="softmax", dev=dev, **c)
    ref.mask_pool = model.mask_pool = True
    _check(ref, model, _batch(3, c["lag"], c["S"], c["price_dim"], c["vocab"]), dtype, dev, "meantTweetPrice[mask_pool]")


def test_two_temporal_encoders(dev):
    """the reference hands every temporal encoder the same tensor, each adds its temp_embedding to it in place, and the last one's
    output goes on (:210-211, :133)"""
    c = CONFIGS["d128"]
    ref, model = _pair(pool="softmax", dev=dev, num_temporal_encoders=2, **c)
    _check(ref, model, _batch(3, c["lag"], c["S"], c["price_dim"], c["vocab"]), torch.float32, dev, "meantTweetPrice[two temporal]")


@pytest.mark.parametrize("pool", ["mean", "softmax"])
def test_prices_reach_the_output(pool, dev):
    c = CONFIGS["d128"]
    _, model = _pair(pool=pool, dev=dev, **c)
    ids, prices, mask, _ = _batch(3, c["lag"], c["S"], c["price_dim"], c["vocab"])
    ids, mask = ids.to(dev), mask.to(dev)
    with torch.no_grad():
        a = model(ids, prices.to(dev), mask)
        b = model(ids, prices.float().to(dev), mask)
        assert torch.equal(a, b), "float64 prices must give the bits of their float32 cast"
        for dt in (torch.float16, torch.bfloat16):
            assert torch.equal(model(ids, prices.to(dt).to(dev), mask), model(ids, prices.to(dt).float().to(dev), mask)), dt
        moved = prices.clone()
        moved[0, 1, 2] += 1.0
        e = model(ids, moved.to(dev), mask)
    assert (e[0] - a[0]).abs().max().item() > 1e-6, "changing a price must change that sample's output"
    assert torch.equal(e[1:], a[1:])


def test_state_dict_round_trip(dev):
    import meant_amd
    c = CONFIGS["d100"]
    _, model = _pair(pool="softmax", dev=dev, **c)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    twin = meant_amd.meantTweetPrice(c["text_dim"], c["price_dim"], c["lag"], 2, nn.Embedding(c["vocab"], c["text_dim"]),
                                     sequence_length=c["S"], num_heads=c["heads"], pool="softmax")
    missing, unexpected = twin.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    twin = twin.to(dev).eval()
    ids, prices, mask, _ = _batch(3, c["lag"], c["S"], c["price_dim"], c["vocab"])
    with torch.no_grad():
        assert torch.equal(model(ids.to(dev), prices.to(dev), mask.to(dev)), twin(ids.to(dev), prices.to(dev), mask.to(dev)))
    for k, v in twin.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k
