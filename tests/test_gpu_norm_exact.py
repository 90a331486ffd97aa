"""The cross-row reductions of csrc/norm.hip at the C ABI, at ZERO tolerance (tests/exact_ref.py).  Every backward entry takes its
statistics as inputs, so with integer dy / x / gains, rinv[row] = 2^e(row) (e cycling through {-2, ..., 2} at period 5: the rows of a
packed group, of a workgroup and of two grid-stride passes differ), an integer LayerNorm mean and a power-of-two group_rows, every
term of dscale / doffset / dgamma / dbeta / pooled is an integer times a power of two: fp32 accumulation is exact in any order, and
the per-wave registers, the LDS combine, the per-block partial rows and the final column sum have to reproduce an int64 reference
bit for bit.  A row that is skipped, counted twice or scaled by another row's rinv moves a column by >= one unit
(tests/test_norm_exact_host.py shows that the relative bound of the other norm tests accepts exactly these mutants).
dx is not a cross-row sum: it is compared with float64, evaluated with the SUPPLIED statistics, at the project's gradient bound.
Operands sit in front of NaN, outputs and the workspace inside sentinel-filled buffers whose guard must survive, and every entry is
called twice and has to give the same bits.  The sums that cannot be made integers (gelu', rinv computed in the kernel) get
row-fingerprint inputs: each probe row is non-zero in its own 8 columns only, so a column block of the output comes from one row.
Shapes: the smallest at which each structure of the launchers exists; the row counts that make a loop run twice follow
meant_num_cus() and the caps of norm.hip mirrored below, and assert that it does.
(utils/rms_norm.py:40-57, meant/meant.py:61-64,103-107,231, meant/meant_vision.py:147)"""
import math
from functools import lru_cache

import pytest
import torch

from tests import exact_ref as E
from tests.exact_ref import POW2_DENOM, assert_exact, assert_guard, ints, to_dev
from tests.util import TOL, assert_close, assert_grad_close

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
DTYPES, IDS = [F32, BF], ["f32", "bf16"]

# ---- the launch arithmetic of csrc/norm.hip (norm_route, norm_blocks, packed_blocks_bwd, launch_fwd_pooled), mirrored -------------------
MAXC, NORM_MAX_BLOCKS, NORM_PACKED_BLOCKS, WIDE_SLICE = 4, 1024, 2048, 8192


def norm_route(rows, d, may_pack=True):
    """(kind, R, C, V) as norm.hip: norm_route"""
    if d % 8 or d > MAXC * 512:
        return ("wide", 0, 0, 8 if d % 8 == 0 else 1)
    nchunk, R = d // 8, 1
    while may_pack and R <= 4:
        if (R * nchunk) % 64 == 0 and R * nchunk // 64 <= 3 and rows % R == 0:
            return ("packed", R, R * nchunk // 64, 8)
        R *= 2
    return ("row", 0, 0, 8)


def norm_blocks(rows):
    return max(1, min(-(-rows // 4), NORM_MAX_BLOCKS))


def packed_blocks_bwd(groups, cus):
    return max(1, min(-(-groups // 4), 2 * cus))


# ---- the tables of the cases (tests/test_norm_exact_host.py walks them and asserts the preconditions of every reference) ------------------
BIG_ROWS = 4 * NORM_MAX_BLOCKS + 7                        # one wave per row: a second grid-stride pass, ragged last block
ROW_CASES = [(8, 1), (8, 3), (8, 5), (8, BIG_ROWS),       # (d, rows): one chunk, 63 idle lanes
             (520, 5),                                    # lane 0 owns two chunks
             (2048, 5),                                   # MAXC full
             (768, 7)]                                    # a packed width whose rows % R != 0 falls back to one wave per row
PACKED = [(128, 4, 1), (512, 1, 1), (1024, 1, 2), (768, 2, 3)]                 # (d, R, C)
PACKED_ROWS = ["one", "few", "loop"]
WIDE_CASES = [(1, 9), (7, 9), (100, 9),                   # V = 1
              (WIDE_SLICE + 1, 9),                        # V = 1, two slices
              (2056, 9),                                  # V = 8
              (WIDE_SLICE, 9),                            # V = 8, exactly one slice (resident)
              (WIDE_SLICE + 8, 9),                        # V = 8, non-resident: accumulates in the partial row
              (3, 4 * NORM_MAX_BLOCKS + 3)]               # past the block cap
EXTRAS = [(520, 5), (768, 36), (2056, 9)]                 # dres and gelu_pre once per kernel family
PARTIAL = [(520, 1), (520, 260), (520, 520), (100, 1), (100, 50), (100, 100)]   # (d, d_part) at PARTIAL_ROWS rows
PARTIAL_ROWS = 13
POOLED_NGROUPS = [1, 5, NORM_PACKED_BLOCKS + 3]


def packed_rows(kind, R, cus):
    return {"one": 4, "few": 36, "loop": R * (8 * cus + 5)}[kind]


def pooled_bwd_rows(group_rows):
    return 36 if group_rows <= 4 else 5 * group_rows if group_rows == 8 else 3 * group_rows


def pooled_fwd_group_rows(ngroups):
    return 4 if ngroups > NORM_PACKED_BLOCKS else 8


# ---- generators and references -----------------------------------------------------------------------------------------------------------

@lru_cache(maxsize=4)
def rms_inputs(rows, d, seed=1):
    """int64 dy, x [rows, d], gain [d], exponents of rinv [rows]"""
    return (ints((rows, d), -3, 3, 0.5, seed), ints((rows, d), -3, 3, 0.7, seed + 1), ints((d,), -3, 3, 1.0, seed + 2),
            E.pow2_exponents(rows))


@lru_cache(maxsize=4)
def extra_inputs(rows, d, seed=1):
    """int64 dres and gelu_pre [rows, d]"""
    return ints((rows, d), -3, 3, 0.5, seed + 3), ints((rows, d), -3, 3, 0.8, seed + 4)


@lru_cache(maxsize=4)
def pooled_grads(groups, d, seed=1):
    return ints((groups, d), -3, 3, 0.7, seed + 5), ints((groups, d), -3, 3, 0.7, seed + 6)


def rms_terms_bound(rows):
    """sum of the magnitudes of the terms of one dscale column, in units of 1 / POW2_DENOM (pooled dy: 1 / (POW2_DENOM group_rows))"""
    return rows * 3 * 3 * (1 << (E.POW2_HI - E.POW2_LO))


def ln_terms_bound(rows):
    return rows * 3 * 5 * (1 << (E.POW2_HI - E.POW2_LO))


def phi64(p):
    return 0.5 * (1.0 + torch.special.erf(p / math.sqrt(2.0)))


def gelu_grad64(p):
    return phi64(p) + p * torch.exp(-0.5 * p * p) / math.sqrt(2.0 * math.pi)


def rms_dx_ref(dy, x, g, r, d_part=None, eps=0.0, dres=None, pre=None):
    """float64, with the supplied r [rows]: r g dy - x (sum_j g dy x) r^2 / ((1 / r - eps) d_part) below d_part (+ dres) (* gelu'(pre))"""
    dy, x, g, r = dy.double(), x.double(), g.double(), r.double()[:, None]
    d_part = x.shape[1] if d_part is None else d_part
    gd = g * dy
    k = (gd * x).sum(1, keepdim=True) * r * r / ((1.0 / r - eps) * d_part)
    dx = r * gd
    dx[:, :d_part] -= k * x[:, :d_part]
    if dres is not None:
        dx = dx + dres.double()
    if pre is not None:
        dx = dx * gelu_grad64(pre.double())
    return dx


def ln_dx_ref(dy, x, g, mean, rstd):
    dy, x, g = dy.double(), x.double(), g.double()
    xh = (x - mean.double()[:, None]) * rstd.double()[:, None]
    gd = g * dy
    return rstd.double()[:, None] * (gd - gd.mean(1, keepdim=True) - xh * (gd * xh).mean(1, keepdim=True))


# ---- device plumbing ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    from meant_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dt(L, dtype):
    return L.BF16 if dtype == BF else L.F32


def fvec(t, dev):
    """a float operand [n] (gain, rinv, bias) with NaN behind it"""
    return to_dev(t.reshape(1, -1), F32, dev)[0]


def out_fvec(n, dev, preload=None):
    """a float output [n] inside a sentinel-filled buffer: (view [1, n], buffer)"""
    return to_dev(None if preload is None else preload.reshape(1, -1), F32, dev, ld=n + 8, sentinel=True, rows=1, cols=n)


class Workspace:
    """the first meant_rmsnorm_bwd_ws(rows, d) bytes of a larger sentinel-filled buffer; whatever lies behind them must survive"""
    GUARD = 4096

    def __init__(self, L, rows, d, dev):
        self.bytes = int(L.lib.meant_rmsnorm_bwd_ws(rows, d))
        assert self.bytes % 4 == 0
        self.n = self.bytes // 4
        self.view, self.buf = to_dev(None, F32, dev, ld=self.n + self.GUARD, sentinel=True, rows=1, cols=self.n, tail_rows=0)
        self.ptr = self.view.data_ptr()

    def check(self, what):
        assert_guard(self.buf, 1, self.n, f"{what}: workspace tail")


def call_twice(call, bufs, what, reset=None):
    """the header promises ordered sums: two calls on the same inputs give the same bits in every output buffer"""
    call()
    first = [E.bits(b) for b in bufs]
    if reset:
        reset()
    call()
    for i, (a, b) in enumerate(zip(first, bufs)):
        assert torch.equal(a, E.bits(b)), f"{what}: output {i} differs between two calls on the same inputs"


def gelem(dtype):
    return TOL[dtype]["gelem"]


def _out_tol(dtype):
    return TOL[dtype]["out"] * (1 if dtype == F32 else 4)      # as tests/test_gpu_norm_wide.py


# ---- 2a. meant_rmsnorm_bwd / meant_rmsnorm_partial_bwd -----------------------------------------------------------------------------------------

def run_rms_bwd(L, dev, dtype, rows, d, *, extras=False, d_part=None, doffset=False, what=""):
    """dscale (and doffset) exact, dx against float64, every guard; d_part given: the partial entry (which never packs)"""
    dy, x, g, e = rms_inputs(rows, d)
    r = E.pow2(e)
    dres, pre = extra_inputs(rows, d) if extras else (None, None)
    want = E.rms_dscale_ref(dy, x, e)
    E.assert_exact_regime(want, rms_terms_bound(rows), what)
    dyd, xd = to_dev(dy, dtype, dev)[0], to_dev(x, dtype, dev)[0]
    gd, rd = fvec(g, dev), fvec(r, dev)
    dresd = to_dev(dres, dtype, dev)[0] if extras else None
    pred = to_dev(pre, dtype, dev)[0] if extras else None
    dxv, dxbuf = to_dev(None, dtype, dev, sentinel=True, rows=rows, cols=d)
    dsv, dsbuf = out_fvec(d, dev)
    dov, dobuf = out_fvec(d, dev) if doffset else (None, None)
    ws = Workspace(L, rows, d, dev)
    p = lambda t: None if t is None else t.data_ptr()

    def call():
        if d_part is None:
            rc = L.lib.meant_rmsnorm_bwd(p(dyd), p(xd), p(gd), p(rd), p(dxv), p(dsv), rows, d, 0.0, 0.0, 0, p(dresd), p(pred), _dt(L, dtype),
                                         ws.ptr, ws.bytes, _stream())
        else:
            rc = L.lib.meant_rmsnorm_partial_bwd(p(dyd), p(xd), p(gd), p(rd), p(dxv), p(dsv), p(dov), rows, d, d_part, 0.0, _dt(L, dtype),
                                                 ws.ptr, ws.bytes, _stream())
        L.check(rc, what)

    call_twice(call, [dxbuf, dsbuf] + ([dobuf] if doffset else []), what)
    assert_exact(dsv[0], want, f"{what}: dscale", denom=POW2_DENOM)
    if doffset:
        assert_exact(dov[0], E.colsum_ref(dy), f"{what}: doffset")
        assert_guard(dobuf, 1, d, f"{what}: doffset")
    assert_grad_close(dxv, rms_dx_ref(dy, x, g, r, d_part, 0.0, dres, pre), gelem(dtype), f"{what}: dx")
    assert_guard(dxbuf, rows, d, f"{what}: dx")
    assert_guard(dsbuf, 1, d, f"{what}: dscale")
    ws.check(what)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d,rows", ROW_CASES)
def test_rmsnorm_bwd_one_wave_per_row(L, dev, dtype, d, rows):
    """rmsnorm_bwd_wide_kernel<T, 8, 64, false>: one wave per row, the four waves' sums folded through LDS (partial_row)"""
    assert norm_route(rows, d)[0] == "row"
    if rows == BIG_ROWS:
        assert rows > 4 * norm_blocks(rows) and rows % 4, "the grid-stride loop has to run a second, ragged pass"
    run_rms_bwd(L, dev, dtype, rows, d, what=f"rmsnorm_bwd row d={d} rows={rows}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", PACKED_ROWS)
@pytest.mark.parametrize("d,R,C", PACKED)
def test_rmsnorm_bwd_packed(L, dev, dtype, d, R, C, kind):
    """rmsnorm_bwd_packed_kernel<T, C, 0, false>"""
    cus = L.lib.meant_num_cus()
    rows = packed_rows(kind, R, cus)
    assert norm_route(rows, d) == ("packed", R, C, 8)
    if kind == "loop":
        groups = rows // R
        assert groups > 4 * packed_blocks_bwd(groups, cus) and groups % 4, "the row-group loop has to run a second, ragged pass"
    run_rms_bwd(L, dev, dtype, rows, d, what=f"rmsnorm_bwd packed R={R} C={C} d={d} rows={rows}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d,rows", WIDE_CASES)
def test_rmsnorm_bwd_wide(L, dev, dtype, d, rows):
    """rmsnorm_bwd_wide_kernel<T, V, 256, false>: one workgroup per row; V = 1 off multiples of 8, else V = 8; resident up to one slice"""
    assert norm_route(rows, d) == ("wide", 0, 0, 8 if d % 8 == 0 else 1)
    assert rows > norm_blocks(rows), "every workgroup takes more than one row"
    if rows > 4 * NORM_MAX_BLOCKS:
        assert -(-rows // 4) > NORM_MAX_BLOCKS, "past the block cap"
    run_rms_bwd(L, dev, dtype, rows, d, what=f"rmsnorm_bwd wide d={d} rows={rows}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d,rows", EXTRAS)
def test_rmsnorm_bwd_with_residual_gradient_and_gelu(L, dev, dtype, d, rows):
    """dres and gelu_pre loaded in each kernel family; they do not enter dscale"""
    run_rms_bwd(L, dev, dtype, rows, d, extras=True, what=f"rmsnorm_bwd {norm_route(rows, d)[0]} d={d} rows={rows} dres gelu_pre")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("doffset", [False, True], ids=["plain", "doffset"])
@pytest.mark.parametrize("d,d_part", PARTIAL)
def test_rmsnorm_partial_bwd(L, dev, dtype, d, d_part, doffset):
    """rmsnorm_bwd_wide_kernel<T, 8, 64, OFF> (d = 520) and <T, 1, 256, OFF> (d = 100): the offset gradient in the second plane"""
    assert norm_route(PARTIAL_ROWS, d, may_pack=False)[0] == ("row" if d == 520 else "wide")
    run_rms_bwd(L, dev, dtype, PARTIAL_ROWS, d, d_part=d_part, doffset=doffset, what=f"rmsnorm_partial_bwd d={d} d_part={d_part}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d,rows", [(8, BIG_ROWS), (WIDE_SLICE + 8, 9), (3, 4 * NORM_MAX_BLOCKS + 3)])
def test_rmsnorm_partial_bwd_second_plane_at_the_caps(L, dev, dtype, d, rows):
    """the offset plane behind NORM_MAX_BLOCKS partial rows, and behind the in-place sums of a non-resident wide row"""
    run_rms_bwd(L, dev, dtype, rows, d, d_part=max(1, d // 2), doffset=True, what=f"rmsnorm_partial_bwd d={d} rows={rows}")


# ---- 2b. meant_rmsnorm_bwd_pooled, bc = 1, 2, 3 -------------------------------------------------------------------------------------------------

def run_bwd_pooled(L, dev, dtype, rows, d, group_rows, bc, what):
    dy, x, g, e = rms_inputs(rows, d)
    r = E.pow2(e)
    groups = rows // group_rows
    dyg, dresg = pooled_grads(groups, d)
    dres = extra_inputs(rows, d)[0]
    assert L.lib.meant_rmsnorm_pooled_ok(rows, d, group_rows) == 1 and group_rows & (group_rows - 1) == 0
    if bc & 1:
        dy_eff, denom = E.expand_groups(dyg, group_rows), POW2_DENOM * group_rows
        dyd = to_dev(dyg, F32, dev)[0]
    else:
        dy_eff, denom = dy, POW2_DENOM
        dyd = to_dev(dy, dtype, dev)[0]
    if bc & 2:
        dres64 = E.expand_groups(dresg, group_rows).double() / group_rows
        dresd = to_dev(dresg, F32, dev)[0]
    else:
        dres64 = dres.double()
        dresd = to_dev(dres, dtype, dev)[0]
    want = E.rms_dscale_ref(dy_eff, x, e)
    E.assert_exact_regime(want, rms_terms_bound(rows), what)
    xd, gd, rd = to_dev(x, dtype, dev)[0], fvec(g, dev), fvec(r, dev)
    dxv, dxbuf = to_dev(None, dtype, dev, sentinel=True, rows=rows, cols=d)
    dsv, dsbuf = out_fvec(d, dev)
    ws = Workspace(L, rows, d, dev)

    def call():
        L.check(L.lib.meant_rmsnorm_bwd_pooled(dyd.data_ptr(), bc & 1, xd.data_ptr(), gd.data_ptr(), rd.data_ptr(), dxv.data_ptr(),
                                               dsv.data_ptr(), rows, d, group_rows, 0.0, 0.0, 0, dresd.data_ptr(), (bc >> 1) & 1, None,
                                               _dt(L, dtype), ws.ptr, ws.bytes, _stream()), what)

    call_twice(call, [dxbuf, dsbuf], what)
    assert_exact(dsv[0], want, f"{what}: dscale", denom=denom)
    dy64 = dy_eff.double() / (group_rows if bc & 1 else 1)
    assert_grad_close(dxv, rms_dx_ref(dy64, x, g, r, dres=dres64), gelem(dtype), f"{what}: dx")
    assert_guard(dxbuf, rows, d, f"{what}: dx")
    assert_guard(dsbuf, 1, d, f"{what}: dscale")
    ws.check(what)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("bc", [1, 2, 3])
@pytest.mark.parametrize("gr", ["R", 8, 64])
@pytest.mark.parametrize("d,R,C", PACKED)
def test_rmsnorm_bwd_pooled(L, dev, dtype, d, R, C, gr, bc):
    """rmsnorm_bwd_packed_kernel<T, C, BC, false>, BC = 1, 2, 3; groups of R, 8 and 64 rows span waves and workgroups"""
    group_rows = R if gr == "R" else gr
    rows = pooled_bwd_rows(group_rows)
    assert norm_route(rows, d) == ("packed", R, C, 8) and rows % group_rows == 0
    run_bwd_pooled(L, dev, dtype, rows, d, group_rows, bc, f"rmsnorm_bwd_pooled bc={bc} R={R} C={C} d={d} rows={rows} group_rows={group_rows}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rmsnorm_bwd_pooled_row_group_loop(L, dev, dtype):
    """BC = 3 at d = 768 (R = 2, C = 3) with the row-group loop running twice"""
    d, R, C = 768, 2, 3
    cus = L.lib.meant_num_cus()
    rows = packed_rows("loop", R, cus)
    groups = rows // R
    assert norm_route(rows, d) == ("packed", R, C, 8) and groups > 4 * packed_blocks_bwd(groups, cus) and groups % 4
    run_bwd_pooled(L, dev, dtype, rows, d, R, 3, f"rmsnorm_bwd_pooled bc=3 d={d} rows={rows} group_rows={R}")


# ---- 2c. meant_layernorm_bwd -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d,rows", ROW_CASES + WIDE_CASES)
def test_layernorm_bwd(L, dev, dtype, d, rows):
    """layernorm_bwd_wide_kernel<T, 8, 64> (d % 8 == 0, d <= 2048: LayerNorm never packs) and <T, V, 256>"""
    what = f"layernorm_bwd d={d} rows={rows}"
    kind = norm_route(rows, d, may_pack=False)[0]
    assert kind == ("row" if d % 8 == 0 and d <= 2048 else "wide")
    dy, x, g, _ = rms_inputs(rows, d)
    mean, e = E.ln_stats(rows)
    rstd = E.pow2(e)
    want_g, want_b = E.ln_dgamma_ref(dy, x, mean, e), E.colsum_ref(dy)
    E.assert_exact_regime(want_g, ln_terms_bound(rows), what)
    dyd, xd, gd = to_dev(dy, dtype, dev)[0], to_dev(x, dtype, dev)[0], fvec(g, dev)
    std = to_dev(torch.stack([mean.double(), rstd], 1), F32, dev)[0]
    dxv, dxbuf = to_dev(None, dtype, dev, sentinel=True, rows=rows, cols=d)
    dgv, dgbuf = out_fvec(d, dev)
    dbv, dbbuf = out_fvec(d, dev)
    ws = Workspace(L, rows, d, dev)

    def call():
        L.check(L.lib.meant_layernorm_bwd(dyd.data_ptr(), xd.data_ptr(), gd.data_ptr(), std.data_ptr(), dxv.data_ptr(), dgv.data_ptr(),
                                          dbv.data_ptr(), rows, d, _dt(L, dtype), ws.ptr, ws.bytes, _stream()), what)

    call_twice(call, [dxbuf, dgbuf, dbbuf], what)
    assert_exact(dgv[0], want_g, f"{what}: dgamma", denom=POW2_DENOM)
    assert_exact(dbv[0], want_b, f"{what}: dbeta")
    assert_grad_close(dxv, ln_dx_ref(dy, x, g, mean, rstd), gelem(dtype), f"{what}: dx")
    assert_guard(dxbuf, rows, d, f"{what}: dx")
    assert_guard(dgbuf, 1, d, f"{what}: dgamma")
    assert_guard(dbbuf, 1, d, f"{what}: dbeta")
    ws.check(what)


# ---- 2d. meant_rmsnorm_fwd_pooled, pool_input != 0: the mean of x ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("with_y", [False, True], ids=["y_null", "y"])
@pytest.mark.parametrize("ngroups", POOLED_NGROUPS)
@pytest.mark.parametrize("d,R,C", PACKED)
def test_rmsnorm_fwd_pooled_mean_of_x(L, dev, dtype, d, R, C, ngroups, with_y):
    """rmsnorm_fwd_pooled_kernel<T, C, 2, false>; 2048 + 3 groups: the loop over groups runs twice in three workgroups"""
    group_rows = pooled_fwd_group_rows(ngroups)
    rows = ngroups * group_rows
    what = f"rmsnorm_fwd_pooled pool_input R={R} C={C} d={d} ngroups={ngroups} group_rows={group_rows}"
    assert norm_route(rows, d) == ("packed", R, C, 8) and L.lib.meant_rmsnorm_pooled_ok(rows, d, group_rows) == 1
    if ngroups > 5:
        assert ngroups > NORM_PACKED_BLOCKS, "the loop over groups has to run twice"
    _, x, g, _ = rms_inputs(rows, d)
    want = x.view(ngroups, group_rows, d).sum(1)
    E.assert_exact_regime(want, 3 * group_rows, what)
    xd, gd = to_dev(x, dtype, dev)[0], fvec(g, dev)
    yv, ybuf = to_dev(None, dtype, dev, sentinel=True, rows=rows, cols=d) if with_y else (None, None)
    rv, rbuf = out_fvec(rows, dev)
    pv, pbuf = to_dev(None, F32, dev, sentinel=True, rows=ngroups, cols=d)

    def call():
        L.check(L.lib.meant_rmsnorm_fwd_pooled(xd.data_ptr(), gd.data_ptr(), yv.data_ptr() if with_y else None, rv.data_ptr(), pv.data_ptr(),
                                               rows, d, group_rows, 1, 0, 0.0, 0.0, 0, _dt(L, dtype), _stream()), what)

    call_twice(call, [pbuf, rbuf] + ([ybuf] if with_y else []), what)
    assert_exact(pv, want, f"{what}: pooled", denom=group_rows)
    assert_guard(pbuf, ngroups, d, f"{what}: pooled")
    assert_guard(rbuf, 1, rows, f"{what}: rinv")
    rms = x.double().pow(2).mean(1).sqrt()
    assert bool((rms > 0).all())
    assert_grad_close(rv[0], 1.0 / rms, 1e-5, f"{what}: rinv")   # an exact sum of squares, then sqrt, rsqrt(d) and a division: a few fp32 ulps
    if with_y:
        assert_close(yv, g.double() * x.double() / rms[:, None], _out_tol(dtype), f"{what}: y")
        assert_guard(ybuf, rows, d, f"{what}: y")


# ---- 3. the sums that pass through gelu', the kernel's own rinv or the gain product: row fingerprints against float64 -----------------------------------

def probe_rows(rows, R, cus):
    """first and last row, the last row of the first pass over the row groups and the first of the second, one row in each of the 4 wave
    slots of a workgroup, and both rows of one packed group"""
    groups = rows // R
    per_pass = 4 * packed_blocks_bwd(groups, cus)
    p = {0, rows - 1}
    if groups > per_pass:
        p |= {R * per_pass - 1, R * per_pass}
    for w in range(4):
        p.add(R * min(4 + w, groups - 1) + w % R)
    if R > 1:
        p |= {R * min(9, groups - 1), R * min(9, groups - 1) + 1}
    return sorted(p)


def fingerprint(rows, d, probes, seed):
    """int64 [rows, d], zero except probe row i in columns [8 i, 8 i + 8), where every element is in +-{1, 2, 3}"""
    assert 8 * len(probes) <= d
    t = torch.zeros(rows, d, dtype=torch.int64)
    v = ints((len(probes), 8), -3, 3, 1.0, seed)
    for i, row in enumerate(probes):
        t[row, 8 * i:8 * i + 8] = v[i]
    return t


def assert_blocks_close(got, want, nblocks, tol, what):
    """the whole vector at the gradient bound, and every probe block against its OWN magnitude: a block that lost its row (0), got it
    twice (2 x) or got another row's factor is far outside any tolerance"""
    assert_grad_close(got, want, tol, what)
    for i in range(nblocks):
        blk = slice(8 * i, 8 * i + 8)
        assert want[blk].abs().max().item() > 0, f"{what}: probe block {i} of the reference is empty"
        assert_grad_close(got[blk], want[blk], tol, f"{what}: probe block {i}")


def run_chain(L, dev, rows, d, R, *, dy_pooled, fingerprints, what):
    """meant_rmsnorm_bwd_chain (bf16 tier).  Integer inputs with x given: dscale exact.  Fingerprints: dscale and dbias_up by block."""
    dtype, cus = BF, L.lib.meant_num_cus()
    group_rows = R if dy_pooled else 1
    _, x, g, e = rms_inputs(rows, d)
    r, ru = E.pow2(e), E.pow2(E.pow2_exponents(rows, 2))
    ub = ints((d,), -3, 3, 1.0, 17).double() / 4
    pre = ints((rows, d), -6, 6, 0.9, 18).double() / 4
    pre0 = ints((d,), -3, 3, 1.0, 19)                           # dbias_up arrives loaded: the header's +=
    up_d = 256
    if fingerprints:
        probes = probe_rows(rows, R, cus)
        dy = fingerprint(rows, d, probes, 20)
        if dy_pooled:                                           # a packed group shares its dy: the probe row alone has x != 0 in its block
            for i, row in enumerate(probes):
                g0 = row - row % R
                keep = pre[row, 8 * i:8 * i + 8].clone()
                pre[g0:g0 + R, 8 * i:8 * i + 8] = 0
                pre[row, 8 * i:8 * i + 8] = torch.where(keep == 0, torch.ones_like(keep), keep)
            dyg = dy.view(rows // R, R, d).sum(1)
            dy64 = E.expand_groups(dyg, R).double() / R
        else:
            dy64 = dy.double()
    else:
        assert not dy_pooled
        dy = rms_inputs(rows, d)[0]
        dy64 = dy.double()
    x64 = pre * phi64(pre) if dy_pooled else x.double()
    dpre = rms_dx_ref(dy64, x64, g, r, pre=pre)
    want_dx = dpre * ru[:, None]
    want_k = (dpre * (pre - ub)).sum(1) * ru * ru / up_d
    want_db = pre0.double() + dpre.sum(0)
    want_ds = (dy64 * x64 * r[:, None]).sum(0)

    dyd = to_dev(dyg, F32, dev)[0] if dy_pooled else to_dev(dy, dtype, dev)[0]
    xd = None if dy_pooled else to_dev(x, dtype, dev)[0]
    pred, gd, rd, rud, ubd = to_dev(pre, dtype, dev)[0], fvec(g, dev), fvec(r, dev), fvec(ru, dev), fvec(ub, dev)
    dxv, dxbuf = to_dev(None, dtype, dev, sentinel=True, rows=rows, cols=d)
    dsv, dsbuf = out_fvec(d, dev)
    kv, kbuf = out_fvec(rows, dev)
    dbv, dbbuf = out_fvec(d, dev, preload=pre0)
    ws = Workspace(L, rows, d, dev)

    def call():
        L.check(L.lib.meant_rmsnorm_bwd_chain(dyd.data_ptr(), int(dy_pooled), None if dy_pooled else xd.data_ptr(), gd.data_ptr(), rd.data_ptr(),
                                              dxv.data_ptr(), dsv.data_ptr(), rows, d, group_rows, 0.0, 0.0, 0, pred.data_ptr(), rud.data_ptr(),
                                              ubd.data_ptr(), 0.0, up_d, kv.data_ptr(), dbv.data_ptr(), _dt(L, dtype), ws.ptr, ws.bytes,
                                              _stream()), what)

    call_twice(call, [dxbuf, dsbuf, kbuf, dbbuf], what, reset=lambda: dbv.copy_(pre0.float().reshape(1, -1)))
    if fingerprints:
        assert_blocks_close(dsv[0].cpu().double(), want_ds, len(probes), gelem(dtype), f"{what}: dscale")
        # outside the probe blocks dbias_up is the pre-loaded integer plus the probe rows' -k x gelu' terms: the whole-vector bound
        assert_blocks_close(dbv[0].cpu().double() - pre0.double(), want_db - pre0.double(), len(probes), gelem(dtype), f"{what}: dbias_up - preload")
    else:
        want = E.rms_dscale_ref(dy, x, e)
        E.assert_exact_regime(want, rms_terms_bound(rows), what)
        assert_exact(dsv[0], want, f"{what}: dscale", denom=POW2_DENOM)
    assert_grad_close(dbv[0], want_db, gelem(dtype), f"{what}: dbias_up")
    assert_grad_close(dxv, want_dx, gelem(dtype), f"{what}: dx_scaled")
    assert_grad_close(kv[0], want_k, gelem(dtype), f"{what}: kcoef")
    for buf, n, name in ((dxbuf, (rows, d), "dx_scaled"), (dsbuf, (1, d), "dscale"), (kbuf, (1, rows), "kcoef"), (dbbuf, (1, d), "dbias_up")):
        assert_guard(buf, n[0], n[1], f"{what}: {name}")
    ws.check(what)


@pytest.mark.parametrize("kind", ["few", "loop"])
@pytest.mark.parametrize("d,R,C", PACKED)
def test_rmsnorm_bwd_chain_dscale_exact(L, dev, d, R, C, kind):
    """rmsnorm_bwd_packed_kernel<bf16, C, 0, true>: dscale has no gelu' factor when x is given; dbias_up is added to its pre-load"""
    cus = L.lib.meant_num_cus()
    rows = packed_rows(kind, R, cus)
    assert norm_route(rows, d) == ("packed", R, C, 8)
    if kind == "loop":
        assert rows // R > 4 * packed_blocks_bwd(rows // R, cus)
    run_chain(L, dev, rows, d, R, dy_pooled=False, fingerprints=False, what=f"rmsnorm_bwd_chain R={R} C={C} d={d} rows={rows}")


@pytest.mark.parametrize("dy_pooled", [False, True], ids=["tokens", "pooled"])
@pytest.mark.parametrize("d,R,C", PACKED)
def test_rmsnorm_bwd_chain_row_fingerprints(L, dev, d, R, C, dy_pooled):
    """rmsnorm_bwd_packed_kernel<bf16, C, 0 | 5, true> with the row-group loop running twice: dscale and dbias_up block by block"""
    cus = L.lib.meant_num_cus()
    rows = packed_rows("loop", R, cus)
    assert norm_route(rows, d) == ("packed", R, C, 8) and rows // R > 4 * packed_blocks_bwd(rows // R, cus)
    run_chain(L, dev, rows, d, R, dy_pooled=dy_pooled, fingerprints=True,
              what=f"rmsnorm_bwd_chain fingerprints R={R} C={C} d={d} rows={rows} dy_pooled={int(dy_pooled)}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d,R,C", PACKED)
def test_rmsnorm_bwd_pooled_gelu_on_load_row_fingerprints(L, dev, dtype, d, R, C):
    """rmsnorm_bwd_packed_kernel<T, C, 5, false>: x = gelu(gelu_pre) formed on load, pooled dy, the row-group loop running twice"""
    cus = L.lib.meant_num_cus()
    rows = packed_rows("loop", R, cus)
    what = f"rmsnorm_bwd_pooled bc=5 R={R} C={C} d={d} rows={rows}"
    assert norm_route(rows, d) == ("packed", R, C, 8) and rows // R > 4 * packed_blocks_bwd(rows // R, cus)
    _, _, g, e = rms_inputs(rows, d)
    r = E.pow2(e)
    pre = ints((rows, d), -6, 6, 0.9, 18).double() / 4
    probes = probe_rows(rows, R, cus)
    dy = fingerprint(rows, d, probes, 20)
    for i, row in enumerate(probes):                            # a packed group shares its dy: the probe row alone has x != 0 in its block
        g0 = row - row % R
        keep = pre[row, 8 * i:8 * i + 8].clone()
        pre[g0:g0 + R, 8 * i:8 * i + 8] = 0
        pre[row, 8 * i:8 * i + 8] = torch.where(keep == 0, torch.ones_like(keep), keep)
    dyg = dy.view(rows // R, R, d).sum(1)
    dy64 = E.expand_groups(dyg, R).double() / R
    x64 = pre * phi64(pre)
    dyd, pred, gd, rd = to_dev(dyg, F32, dev)[0], to_dev(pre, dtype, dev)[0], fvec(g, dev), fvec(r, dev)
    dxv, dxbuf = to_dev(None, dtype, dev, sentinel=True, rows=rows, cols=d)
    dsv, dsbuf = out_fvec(d, dev)
    ws = Workspace(L, rows, d, dev)

    def call():
        L.check(L.lib.meant_rmsnorm_bwd_pooled(dyd.data_ptr(), 1, None, gd.data_ptr(), rd.data_ptr(), dxv.data_ptr(), dsv.data_ptr(), rows, d, R,
                                               0.0, 0.0, 0, None, 0, pred.data_ptr(), _dt(L, dtype), ws.ptr, ws.bytes, _stream()), what)

    call_twice(call, [dxbuf, dsbuf], what)
    assert_blocks_close(dsv[0].cpu().double(), (dy64 * x64 * r[:, None]).sum(0), len(probes), gelem(dtype), f"{what}: dscale")
    assert_grad_close(dxv, rms_dx_ref(dy64, x64, g, r, pre=pre), gelem(dtype), f"{what}: dx")
    assert_guard(dxbuf, rows, d, f"{what}: dx")
    assert_guard(dsbuf, 1, d, f"{what}: dscale")
    ws.check(what)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("gelu_input", [0, 1], ids=["x", "gelu_on_load"])
@pytest.mark.parametrize("d,R,C", [(128, 4, 1), (512, 1, 1)])
def test_rmsnorm_fwd_pooled_mean_of_y_row_fingerprints(L, dev, dtype, d, R, C, gelu_input):
    """rmsnorm_fwd_pooled_kernel<T, C, 1, GELU_IN>: the mean of y, rinv computed in the kernel; 2048 + 3 groups of 4 R rows (one step
    per wave).  Probe rows: the four wave slots of group 0 (the first row among them), both rows of a packed group in group 1, one
    row in the last group of the first pass and in the first of the second, and the last row."""
    ngroups, group_rows, eps = NORM_PACKED_BLOCKS + 3, 4 * R, 1e-8
    rows = ngroups * group_rows
    what = f"rmsnorm_fwd_pooled mean of y R={R} C={C} d={d} ngroups={ngroups} group_rows={group_rows} gelu_input={gelu_input}"
    assert norm_route(rows, d) == ("packed", R, C, 8) and ngroups > NORM_PACKED_BLOCKS
    probes = {w * R + (w % R if w else 0) for w in range(4)}
    probes |= {group_rows + R, group_rows + R + (1 if R > 1 else 2)}
    probes |= {(NORM_PACKED_BLOCKS - 1) * group_rows + 1, NORM_PACKED_BLOCKS * group_rows + group_rows - 2, rows - 1}
    probes = sorted(probes)
    assert len(probes) == 9
    xin = fingerprint(rows, d, probes, 30).double()             # pre-activation (gelu_input) or activation
    if gelu_input:
        xin = xin.abs()                                         # gelu(-3) = -0.004: a negative pre-activation leaves nothing to see
    g = ints((d,), 2, 3, 1.0, 31)
    xd, gd = to_dev(xin, dtype, dev)[0], fvec(g, dev)
    rv, rbuf = out_fvec(rows, dev)
    pv, pbuf = to_dev(None, F32, dev, sentinel=True, rows=ngroups, cols=d)

    def call():
        L.check(L.lib.meant_rmsnorm_fwd_pooled(xd.data_ptr(), gd.data_ptr(), None, rv.data_ptr(), pv.data_ptr(), rows, d, group_rows, 0,
                                               gelu_input, eps, 0.0, 0, _dt(L, dtype), _stream()), what)

    call_twice(call, [pbuf, rbuf], what)
    x64 = xin * phi64(xin) if gelu_input else xin
    rinv = 1.0 / (x64.pow(2).mean(1).sqrt() + eps)
    want = (g.double() * x64 * rinv[:, None]).view(ngroups, group_rows, d).mean(1)
    got = pv.cpu().double()
    for i, row in enumerate(probes):
        blk = want[row // group_rows, 8 * i:8 * i + 8]
        assert blk.abs().min().item() > 2.5 * _out_tol(dtype), f"{what}: probe block {i} would hide under the bound"
    assert_close(got, want, _out_tol(dtype), f"{what}: pooled")
    assert bool((got[want == 0] == 0).all()), f"{what}: a value outside the probe blocks"
    assert_guard(pbuf, ngroups, d, f"{what}: pooled")
    assert_guard(rbuf, 1, rows, f"{what}: rinv")
