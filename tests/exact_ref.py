"""Exact-integer GEMM checks: small-integer operands make every product and every partial sum an integer below 2^24, so fp32
accumulation is exact in ANY order -- MFMA trees, float atomics, split-K, stolen tiles all give the same bits -- and the result has
to equal an int64 reference with zero tolerance.  A dropped, doubled, misplaced or out-of-range term moves some output by >= 1.

Helpers (not collected): integer generators, placement of operands as column slices of wider poisoned buffers, outputs inside
sentinel-filled buffers, the exact comparison and the guard check.  Used by tests/test_gemm_exact_host.py (CPU: shows that the
method rejects the mutants the relative bounds accept) and tests/test_gpu_gemm_exact.py (every GEMM route at the C ABI); the
generators at the end carry the method to the norm kernels' cross-row reductions (tests/test_norm_exact_host.py,
tests/test_gpu_norm_exact.py)."""
import numpy as np
import torch

BF16_INT_LIMIT = 256          # every integer of magnitude <= 2^8 is a bf16 value (8 significant bits), whatever the rounding mode
F32_INT_LIMIT = 1 << 24       # ... and below 2^24 a float
SENTINEL_BITS = {torch.bfloat16: 0x7FA5, torch.float32: 0x7FA5A5A5}       # NaN payloads no kernel produces
_INT_VIEW = {torch.bfloat16: torch.int16, torch.float32: torch.int32}


def ints(shape, lo=-1, hi=1, density=0.5, seed=0):
    """int64 tensor: an element is non-zero with probability `density`, then uniform over the non-zero integers of [lo, hi]
    (default: ternary {-1, 0, 1}); density None: uniform over [lo, hi], zero included"""
    rs = np.random.RandomState(seed)
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    if density is None:
        return torch.from_numpy(rs.randint(lo, hi + 1, size=shape).astype(np.int64))
    pool = np.array([v for v in range(lo, hi + 1) if v != 0], dtype=np.int64)
    vals = pool[rs.randint(0, len(pool), size=shape)]
    keep = rs.random_sample(shape) < density
    return torch.from_numpy(np.where(keep, vals, 0).astype(np.int64))


def mm(a, b):
    """exact integer matrix product a @ b of int64 tensors (float64 BLAS: every sum stays below 2^53), as int64"""
    return (a.double() @ b.double()).to(torch.int64)


def _sentinel(dtype):
    return SENTINEL_BITS[dtype], _INT_VIEW[dtype]           # both patterns are positive in the signed view


def to_dev(t, dtype, dev, ld=None, poison=None, sentinel=None, tail_rows=1, rows=None, cols=None):
    """Place a [rows, cols] matrix on the device as a column slice of a wider buffer; returns (view, buffer).
    Input (sentinel None): buffer [rows + tail_rows, ld] of `poison` (default NaN) with t in its top left corner -- whatever a kernel
    reads at or beyond column `cols` of a row, or behind the last row, poisons its output.
    Output (sentinel True): the whole buffer holds the sentinel bit pattern; t (may be None with rows / cols given) pre-loads the
    valid region ("+=" contracts, in-place residuals).  ld: row stride in elements, a multiple of 8 for bf16 operands of the MFMA
    kernels; the base is the allocation's (>= 256-byte aligned)."""
    if t is not None:
        rows, cols = t.shape
    ld = cols if ld is None else int(ld)
    assert ld >= cols
    if sentinel:
        bits, it = _sentinel(dtype)
        buf = torch.full((rows + tail_rows, ld), bits, dtype=it, device=dev).view(dtype)
    else:
        buf = torch.full((rows + tail_rows, ld), float("nan") if poison is None else poison, dtype=dtype, device=dev)
    view = buf[:rows, :cols]
    if t is not None:
        ft = t.to(torch.float64)
        assert torch.equal(ft.to(dtype).to(torch.float64), ft), "operand not representable in the storage type"
        view.copy_(ft.to(dtype))
    assert buf.data_ptr() % 16 == 0
    return view, buf


def assert_exact(got, want, what="", denom=1):
    """got (bf16 or float tensor, any device) * denom == want (int64), element for element.  denom: a power of two for references in
    exact binary fractions (the rotary tables' halves).  The preconditions on the REFERENCE come first, so that a change of shapes
    cannot leave the exact regime unnoticed."""
    assert want.dtype == torch.int64, "the reference is int64"
    want = want.cpu()
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(want.shape), f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    assert denom >= 1 and denom & (denom - 1) == 0
    wmax = int(want.abs().max().item()) if want.numel() else 0
    if got.dtype == torch.bfloat16:
        assert wmax <= BF16_INT_LIMIT, f"{what}: |reference| reaches {wmax} > {BF16_INT_LIMIT}: outside the exact range of a bf16 output"
        wf = want.double() / denom
        assert torch.equal(wf.to(torch.bfloat16).double(), wf), f"{what}: reference not representable in bf16"
    else:
        assert got.dtype == torch.float32
        assert wmax < F32_INT_LIMIT, f"{what}: |reference| reaches {wmax} >= 2^24: outside the exact range of a float output"
    g = got.double() * denom
    w = want.double()
    if torch.equal(g, w):
        return
    bad = ~(g == w)                                       # NaN counts as wrong
    n = int(bad.sum().item())
    idx = bad.reshape(-1).nonzero()[0].item()
    pos = np.unravel_index(idx, tuple(want.shape)) if want.dim() else ()
    d = (g - w).reshape(-1)[idx].item()
    raise AssertionError(f"{what}: {n} of {want.numel()} elements wrong; first at {tuple(int(p) for p in pos)}: got - want = {d:g} "
                         f"(got {g.reshape(-1)[idx].item():g}, want {w.reshape(-1)[idx].item():g}, in units of 1/{denom})")


def assert_guard(buf, rows, cols, what=""):
    """every element of the output buffer outside [0, rows) x [0, cols) still holds the sentinel bits"""
    bits, it = _sentinel(buf.dtype)
    b = buf.view(it).cpu()
    ok = b == bits
    ok[:rows, :cols] = True
    if bool(ok.all()):
        return
    bad = (~ok).nonzero()
    r, c = int(bad[0, 0]), int(bad[0, 1])
    raise AssertionError(f"{what}: {bad.shape[0]} guard elements overwritten; first at (row {r}, column {c}) of a [{rows}, {cols}] "
                         f"output in a [{buf.shape[0]}, {buf.shape[1]}] buffer")


# ---- norm kernels: cross-row reductions on integers times powers of two (tests/test_norm_exact_host.py, tests/test_gpu_norm_exact.py) ----
# Every backward entry of csrc/norm.hip takes its statistics as INPUTS, so with integer dy / x, rinv[row] = 2^e(row) and an integer
# mean every term dy * x * rinv of a gain gradient is an integer in units of 2^POW2_LO: (dy * x) * r, dy * (x * r) and the fused
# multiply-add of either are all exact, and so is their fp32 sum in any order while it stays below 2^24 of those units.
POW2_LO, POW2_HI, POW2_PERIOD = -2, 2, 5      # e cycles through {-2, ..., 2}: period 5, coprime to the 4 wave slots and to R = 1, 2, 4
POW2_DENOM = 1 << -POW2_LO                    # references of rinv-weighted sums are in units of 1 / POW2_DENOM


def pow2_exponents(rows, shift=0):
    """e(row) in {POW2_LO, ..., POW2_HI}: rows of one packed group, of one workgroup and of one grid-stride pass differ"""
    return (torch.arange(int(rows), dtype=torch.int64) + shift) % POW2_PERIOD + POW2_LO


def pow2(e):
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double())


def ln_stats(rows):
    """LayerNorm statistics as inputs: (integer mean in [-2, 2] at period 3, exponent of rstd at period 5), both int64 [rows]"""
    return torch.arange(int(rows), dtype=torch.int64) % 3 * 2 - 2, pow2_exponents(rows, 1)


def expand_groups(dy_g, group_rows):
    """[groups, d] -> [groups * group_rows, d]: row r sees dy_g[r // group_rows] (the division by group_rows goes into `denom`)"""
    return dy_g.repeat_interleave(int(group_rows), dim=0)


def rms_dscale_ref(dy, x, e):
    """sum_r dy[r] * x[r] * 2^e[r] in units of 1 / POW2_DENOM, int64 [d]"""
    return (dy * x * (1 << (e - POW2_LO))[:, None]).sum(0)


def ln_dgamma_ref(dy, x, mean, e):
    """sum_r dy[r] * (x[r] - mean[r]) * 2^e[r] in units of 1 / POW2_DENOM, int64 [d]"""
    return (dy * (x - mean[:, None]) * (1 << (e - POW2_LO))[:, None]).sum(0)


def colsum_ref(dy):
    """doffset / dbeta: sum_r dy[r], int64 [d]"""
    return dy.sum(0)


def bits(buf):
    """a copy of the buffer's bit patterns (the signed integer view of its width): two runs of one entry have to agree in these"""
    return buf.view(_INT_VIEW[buf.dtype]).clone()


def assert_exact_regime(want, terms_bound, what=""):
    """a reference and the bound on the sum of the magnitudes of its terms (hence on every partial sum, in any order) stay below 2^24"""
    assert int(want.abs().max().item()) <= int(terms_bound) < F32_INT_LIMIT, f"{what}: partial sums may reach {terms_bound} >= 2^24"
