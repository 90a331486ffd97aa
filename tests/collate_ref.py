"""The masking rule of the device collators (meant_amd/csrc/collate.hip), restated in numpy uint64 arithmetic.

    fin(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31        (mod 2^64)
    bits(seed, stream, idx)   = fin(seed + (idx | stream << 60) * 0x9E3779B97F4A7C15)
    draw24(seed, stream, idx) = bits >> 40
    idx = sample_id * E + e;  chosen iff draw24(seed, 0, idx) < floor(p * 2^24)

Nothing here imports the package: the tests compare the library against this file."""
import math

import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)


def _u64(x):
    return np.asarray(x).astype(np.uint64)


def fin(z):
    z = _u64(z)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
    return z ^ (z >> np.uint64(31))


def bits(seed, stream, idx):
    idx = _u64(idx)
    assert int(idx.max(initial=0)) < 1 << 60
    with np.errstate(over="ignore"):
        return fin(np.uint64(int(seed) & (2 ** 64 - 1)) + (idx | np.uint64(int(stream) << 60)) * GOLDEN)


def draw24(seed, stream, idx):
    return bits(seed, stream, idx) >> np.uint64(40)


def threshold(p):
    return int(math.floor(float(p) * (1 << 24)))


def collate_seed(seed, epoch):
    """the per-epoch seed: bits(seed, stream 3, epoch)"""
    return int(bits(seed, 3, np.array([epoch], dtype=np.uint64))[0])


def element_index(sample_ids, E):
    """idx [B, E] of samples `sample_ids` [B] with E elements each"""
    sid = _u64(sample_ids).reshape(-1, 1)
    return sid * np.uint64(E) + np.arange(E, dtype=np.uint64).reshape(1, -1)


def chosen(seed, sample_ids, E, p, stream=0):
    """bool [B, E]: the rule's choice for every element of the samples"""
    return draw24(seed, stream, element_index(sample_ids, E)) < np.uint64(threshold(p))


def mlm_expected(ids, attention_mask, sample_ids, special_ids, seed, p, mask_id, vocab_size, replace=1.0, random=0.0, ignore_index=-100):
    """(ids_out, labels, chosen) of meant_mlm_mask for ids int64 [B, S]"""
    ids = np.asarray(ids, dtype=np.int64)
    B, S = ids.shape
    idx = element_index(sample_ids, S)
    open_ = ~np.isin(ids, np.asarray(list(special_ids), dtype=np.int64))
    if attention_mask is not None:
        open_ &= np.asarray(attention_mask) != 0
    ch = open_ & (draw24(seed, 0, idx) < np.uint64(threshold(p)))
    r = draw24(seed, 1, idx)
    t_rep, t_rand = threshold(replace), threshold(random)
    rand_id = (bits(seed, 2, idx) % np.uint64(vocab_size)).astype(np.int64)
    out = ids.copy()
    to_mask = ch & (r < np.uint64(t_rep))
    to_rand = ch & ~to_mask & (r < np.uint64(t_rep + t_rand))
    out[to_mask] = mask_id
    out[to_rand] = rand_id[to_rand]
    labels = np.where(ch, ids, np.int64(ignore_index))
    return out, labels, ch


def normalise(images, mean, std):
    """((float)x - mean) * inv_std in fp32, inv_std = (float)(1 / std) as the wrappers pass it: the device's arithmetic bit for bit"""
    x = np.asarray(images).astype(np.float32)
    return (x - np.float32(mean)) * np.float32(1.0 / float(std))


def mim_inputs_labels(images, sample_ids, seed, p, mean=0.0, std=1.0, mask_value=0.0, unmasked_label=-100.0):
    """(inputs, labels, mask) of mim_dataset.mask_image on the normalised image, fp32 [B, C, H, W]: inputs = where(mask, mask_value, x),
    labels = x where masked and unmasked_label elsewhere.  `images` as a numpy array of any real dtype (bf16 widened by the caller)."""
    x = normalise(images, mean, std)
    B = x.shape[0]
    E = int(np.prod(x.shape[1:]))
    mask = chosen(seed, sample_ids, E, p).reshape(x.shape)
    inputs = np.where(mask, np.float32(mask_value), x).astype(np.float32)
    labels = np.where(mask, x, np.float32(unmasked_label)).astype(np.float32)
    return inputs, labels, mask
