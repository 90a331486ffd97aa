"""The exact-integer method applied to the norm kernels' cross-row reductions, checked on the CPU (what tests/test_gemm_exact_host.py
is for the GEMMs):
  - a model of the launch structure of csrc/norm.hip (workgroups of 4 wave slots, grid-stride passes, per-block partial rows, the final
    column sum) gives dscale = sum_r dy[r] x[r] rinv[r] and LayerNorm's dgamma / dbeta, and is mutated the way these kernels can go
    wrong: one row dropped, the last rows % 4 rows dropped, one grid-stride pass counted twice, rinv taken from the neighbouring row
    of a packed group, one per-block partial row left out of the column sum;
  - on the integer inputs of tests/test_gpu_norm_exact.py every mutant is rejected by assert_exact;
  - on the randn inputs of tests/test_gpu_norm_wide.py the relative bound TOL[dtype]["gelem"] does not see them.  At that file's row
    counts (2 to 130) the loop mutants -- the first row of the second pass dropped, the second pass counted twice -- are the identity,
    because no second pass exists: whatever the loop does wrong there is accepted, in both tiers.  (A row dropped from the ONLY pass
    is seen at these row counts: it is 1 / sqrt(rows) of the sum.)  At the row counts where the loop exists (4096 + 7 rows, and the
    8 CUs + 5 row groups of the packed kernels) the same mutants change the result, and the bf16 bound still accepts them;
  - the generators keep the exact regime for every table of the GPU file: operands within the bf16 integers, every reference and the
    sum of the magnitudes of its terms below 2^24 in its unit (at the 256 compute units of an MI355X)."""
import numpy as np
import pytest
import torch

from tests import exact_ref as E
from tests import test_gpu_norm_exact as G
from tests import test_gpu_norm_wide as W
from tests.exact_ref import BF16_INT_LIMIT, POW2_DENOM, assert_exact
from tests.util import TOL, assert_grad_close

BF, F32 = torch.bfloat16, torch.float32
CUS = 256


# ---- the model ------------------------------------------------------------------------------------------------------------------------------

def reduce_model(terms, R=1, max_blocks=G.NORM_MAX_BLOCKS, mutate=None):
    """column sums of terms [rows, d] (float64) the way the kernels take them: units of R rows (R = 1: one wave per row) dealt to
    workgroups of 4 wave slots, `nb` workgroups, pass p covering units [4 nb p, 4 nb (p + 1)); one partial row per workgroup; the
    column sum of the partial rows.  mutate: ("drop_row", i) | ("drop_tail",) | ("double_pass", p) | ("skip_partial", b)"""
    rows, d = terms.shape
    terms = terms.clone()
    kind = mutate[0] if mutate else None
    if kind == "drop_row":
        terms[mutate[1]] = 0
    if kind == "drop_tail":
        terms[rows - rows % 4:] = 0
    units = rows // R
    unit_terms = terms[:units * R].view(units, R, d).sum(1)
    nb = max(1, min(-(-units // 4), max_blocks))
    partial = torch.zeros(nb, d, dtype=torch.float64)
    for p in range(-(-units // (4 * nb))):
        lo, hi = 4 * nb * p, min(units, 4 * nb * (p + 1))
        t = unit_terms[lo:hi] * (2 if kind == "double_pass" and mutate[1] == p else 1)
        partial.index_add_(0, torch.arange(hi - lo) // 4, t)
    if kind == "skip_partial":
        partial[mutate[1]] = 0
    return partial.sum(0)


def rms_terms(dy, x, r, neighbour_R=None):
    """dy x rinv [rows, d], float64; neighbour_R: every row of a packed group of R rows takes the rinv of the next row of its group"""
    r = r.double()
    if neighbour_R:
        i = torch.arange(r.numel())
        r = r[i - i % neighbour_R + (i % neighbour_R + 1) % neighbour_R]
    return dy.double() * x.double() * r[:, None]


def ln_terms(dy, x, mean, rstd):
    return dy.double() * (x.double() - mean.double()[:, None]) * rstd.double()[:, None], dy.double()


def live_row(terms, lo=0, hi=None):
    """a row in [lo, hi) that contributes to some column"""
    live = (terms[lo:hi] != 0).any(1).nonzero()
    assert live.numel(), "no live row in the range"
    return lo + int(live[len(live) // 2])


# ---- every mutant is rejected on the integer inputs --------------------------------------------------------------------------------------------

def _mutants(terms, R, max_blocks):
    rows = terms.shape[0]
    units = rows // R
    nb = max(1, min(-(-units // 4), max_blocks))
    m = {"one row dropped": ("drop_row", live_row(terms)), "one partial row left out": ("skip_partial", nb // 2)}
    if rows % 4 and R == 1:
        m["the last rows % 4 rows dropped"] = ("drop_tail",)
    if units > 4 * nb:
        m["the second pass counted twice"] = ("double_pass", 1)
        m["the first row of the second pass dropped"] = ("drop_row", live_row(terms, 4 * nb * R))
    return m


@pytest.mark.parametrize("d,rows,R", [(8, G.BIG_ROWS, 1), (8, 5, 1), (520, 5, 1), (768, 7, 1), (128, 36, 4), (768, 36, 2),
                                      (128, G.packed_rows("loop", 4, CUS), 4), (3, 4 * G.NORM_MAX_BLOCKS + 3, 1)])
def test_rmsnorm_mutants_are_rejected(d, rows, R):
    dy, x, _, e = G.rms_inputs(rows, d)
    r = E.pow2(e)
    want = E.rms_dscale_ref(dy, x, e)
    cap = 2 * CUS if R > 1 else G.NORM_MAX_BLOCKS
    terms = rms_terms(dy, x, r)
    assert_exact(reduce_model(terms, R, cap).float(), want, "unmutated", denom=POW2_DENOM)
    mutants = _mutants(terms, R, cap)
    if rows > 4 * G.NORM_MAX_BLOCKS or R > 1 and rows > 36:
        assert "the second pass counted twice" in mutants
    for name, m in mutants.items():
        with pytest.raises(AssertionError, match="elements wrong"):
            assert_exact(reduce_model(terms, R, cap, m).float(), want, name, denom=POW2_DENOM)
    if R > 1:
        with pytest.raises(AssertionError, match="elements wrong"):
            assert_exact(reduce_model(rms_terms(dy, x, r, neighbour_R=R), R, cap).float(), want, "rinv of the neighbouring row",
                         denom=POW2_DENOM)


@pytest.mark.parametrize("d,rows", [(8, G.BIG_ROWS), (8, 5), (2048, 5), (100, 9), (3, 4 * G.NORM_MAX_BLOCKS + 3)])
def test_layernorm_mutants_are_rejected(d, rows):
    dy, x, _, _ = G.rms_inputs(rows, d)
    mean, e = E.ln_stats(rows)
    tg, tb = ln_terms(dy, x, mean, E.pow2(e))
    want_g, want_b = E.ln_dgamma_ref(dy, x, mean, e), E.colsum_ref(dy)
    assert_exact(reduce_model(tg).float(), want_g, "dgamma unmutated", denom=POW2_DENOM)
    assert_exact(reduce_model(tb).float(), want_b, "dbeta unmutated")
    for terms, want, denom in ((tg, want_g, POW2_DENOM), (tb, want_b, 1)):
        for name, m in _mutants(terms, 1, G.NORM_MAX_BLOCKS).items():
            with pytest.raises(AssertionError, match="elements wrong"):
                assert_exact(reduce_model(terms, mutate=m).float(), want, name, denom=denom)
    # statistics of the neighbouring row: the mean and rstd of row i + 1 on row i
    shifted = ln_terms(dy, x, mean.roll(-1), E.pow2(e.roll(-1)))[0]
    with pytest.raises(AssertionError, match="elements wrong"):
        assert_exact(reduce_model(shifted).float(), want_g, "statistics of the neighbouring row", denom=POW2_DENOM)


def test_pooled_gradient_mutants_are_rejected():
    """dy_row = dy_g[row / group_rows] / group_rows: the unit is 1 / (POW2_DENOM group_rows); a row that reads the next group's dy"""
    d, R, group_rows = 768, 2, 8
    rows = G.pooled_bwd_rows(group_rows)
    _, x, _, e = G.rms_inputs(rows, d)
    dyg = G.pooled_grads(rows // group_rows, d)[0]
    dy = E.expand_groups(dyg, group_rows)
    want = E.rms_dscale_ref(dy, x, e)
    terms = rms_terms(dy, x, E.pow2(e)) / group_rows
    assert_exact(reduce_model(terms, R, 2 * CUS).float(), want, "unmutated", denom=POW2_DENOM * group_rows)
    wrong = dy.clone()
    wrong[group_rows - 1] = dyg[1]                              # the last row of group 0 takes the gradient of group 1
    with pytest.raises(AssertionError, match="elements wrong"):
        assert_exact(reduce_model(rms_terms(wrong, x, E.pow2(e)) / group_rows, R, 2 * CUS).float(), want, "next group's dy",
                     denom=POW2_DENOM * group_rows)
    for name, m in _mutants(terms, R, 2 * CUS).items():
        with pytest.raises(AssertionError, match="elements wrong"):
            assert_exact(reduce_model(terms, R, 2 * CUS, m).float(), want, name, denom=POW2_DENOM * group_rows)


# ---- the gap: what the relative bound of the randn tests lets through ---------------------------------------------------------------------------

def _randn_case(rows, d, dtype):
    """the inputs of tests/test_gpu_norm_wide.py::test_rmsnorm_any_width, rounded to the tier's storage type as there, and the true rinv"""
    x, dy, _ = W._inputs(rows, d, rows * 7 + d)
    x, dy = x.to(dtype).double(), dy.to(dtype).double()
    return dy, x, 1.0 / (x.pow(2).mean(1).sqrt() + 1e-8)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,d", W.WIDE_SHAPES)
def test_the_loop_mutants_are_invisible_at_the_row_counts_of_the_randn_tests(rows, d, dtype):
    """the wide kernels take one row per workgroup, norm_blocks(rows) workgroups: at 2 to 130 rows a second pass exists for none of
    the one-wave-per-row kernels' 4 x 1024 slots.  'The first row of the second pass dropped' and 'the second pass counted twice' are
    then no mutation at all, and pass the bound as the correct kernel does."""
    dy, x, r = _randn_case(rows, d, dtype)
    terms = rms_terms(dy, x, r)
    ref = reduce_model(terms)
    nb = G.norm_blocks(rows)
    assert rows <= 4 * nb, "no second grid-stride pass at this row count"
    doubled = reduce_model(terms, mutate=("double_pass", 1))
    dropped = reduce_model(terms[:4 * nb])                       # every row past the first pass dropped
    for name, got in (("second pass counted twice", doubled), ("rows past the first pass dropped", dropped)):
        assert_grad_close(got, ref, TOL[dtype]["gelem"], name)
        assert torch.equal(got, ref)
    # ... while a row dropped from the only pass is seen here: it is ~ 1 / sqrt(rows) of a column
    with pytest.raises(AssertionError):
        assert_grad_close(reduce_model(terms, mutate=("drop_row", rows - 1)), ref, TOL[dtype]["gelem"], "last row dropped")


@pytest.mark.parametrize("d,rows,R", [(8, G.BIG_ROWS, 1), (128, G.packed_rows("loop", 4, CUS), 4), (768, G.packed_rows("loop", 2, CUS), 2)])
def test_the_relative_bound_accepts_the_loop_mutants_where_the_loop_exists(d, rows, R):
    """randn inputs by the same recipe at the row counts of tests/test_gpu_norm_exact.py: the first row of the second pass dropped,
    the last row dropped, the ragged second pass counted twice and (packed) the neighbouring row's rinv in one row group all pass
    assert_grad_close(..., TOL[bf16]["gelem"] = 6e-2), and all differ from the reference.  The integer inputs reject each of them above.
    Measured: dropped rows 1.1e-2 to 4.0e-2, the doubled pass 3.2e-2 (d = 128) and 4.4e-2 (d = 8), the neighbour's rinv 4.9e-3 and
    1.7e-3.  At d = 768 the doubled pass of 5 groups (10 of 4106 rows) is at 6.5e-2 over 768 columns, just outside the bound: stated
    below, not hidden."""
    dy, x, r = _randn_case(rows, d, BF)
    terms = rms_terms(dy, x, r)
    cap = 2 * CUS if R > 1 else G.NORM_MAX_BLOCKS
    ref = reduce_model(terms, R, cap)
    units = rows // R
    nb = max(1, min(-(-units // 4), cap))
    assert units > 4 * nb
    mutants = {"first row of the second pass dropped": reduce_model(terms, R, cap, ("drop_row", 4 * nb * R)),
               "last row dropped": reduce_model(terms, R, cap, ("drop_row", rows - 1)),
               "second pass counted twice": reduce_model(terms, R, cap, ("double_pass", 1))}
    if R > 1:
        wrong = terms.clone()
        g0 = 4 * nb * R
        wrong[g0:g0 + R] = rms_terms(dy[g0:g0 + R], x[g0:g0 + R], r[g0:g0 + R], neighbour_R=R)
        mutants["rinv of the neighbouring row in one row group"] = reduce_model(wrong, R, cap)
    for name, got in mutants.items():
        e = ((got - ref).abs().max() / ref.abs().max()).item()
        print(f"d={d} rows={rows} {name}: relative max error {e:.2e}")
        assert not torch.equal(got, ref), name
        if (d, name) == (768, "second pass counted twice"):
            assert TOL[BF]["gelem"] < e < 1.2 * TOL[BF]["gelem"]
            continue
        assert_grad_close(got, ref, TOL[BF]["gelem"], name)


# ---- the preconditions hold for every table of the GPU file -------------------------------------------------------------------------------------

def _all_rms_shapes():
    s = {(d, rows) for d, rows in G.ROW_CASES + G.WIDE_CASES + G.EXTRAS}
    s |= {(d, G.packed_rows(k, R, CUS)) for d, R, _ in G.PACKED for k in G.PACKED_ROWS}
    s |= {(d, G.PARTIAL_ROWS) for d, _ in G.PARTIAL}
    s |= {(d, G.pooled_bwd_rows(R if gr == "R" else gr)) for d, R, _ in G.PACKED for gr in ("R", 8, 64)}
    return sorted(s)


@pytest.mark.parametrize("d,rows", _all_rms_shapes())
def test_references_stay_exact(d, rows):
    dy, x, g, e = G.rms_inputs(rows, d)
    for t in (dy, x, g) + G.extra_inputs(rows, d):
        assert int(t.abs().max()) <= 3 <= BF16_INT_LIMIT
    assert set(e.unique().tolist()) <= set(range(E.POW2_LO, E.POW2_HI + 1))
    assert E.POW2_PERIOD % 2 == 1 and (rows < E.POW2_PERIOD or len(e.unique()) == E.POW2_PERIOD)
    E.assert_exact_regime(E.rms_dscale_ref(dy, x, e), G.rms_terms_bound(rows), f"dscale ({rows}, {d})")
    E.assert_exact_regime(E.colsum_ref(dy), 3 * rows, f"doffset ({rows}, {d})")
    mean, el = E.ln_stats(rows)
    assert int(mean.abs().max()) <= 2 and set(el.unique().tolist()) <= set(range(E.POW2_LO, E.POW2_HI + 1))
    E.assert_exact_regime(E.ln_dgamma_ref(dy, x, mean, el), G.ln_terms_bound(rows), f"dgamma ({rows}, {d})")
    # what a correct kernel stores passes the comparison, in the float of the outputs
    assert_exact((E.rms_dscale_ref(dy, x, e).double() / POW2_DENOM).float(), E.rms_dscale_ref(dy, x, e), "dscale", denom=POW2_DENOM)


@pytest.mark.parametrize("d,R,C", G.PACKED)
def test_pooled_references_stay_exact(d, R, C):
    for gr in (R, 8, 64):
        rows = G.pooled_bwd_rows(gr)
        assert rows % gr == 0 and rows % R == 0 and gr % R == 0 and gr & (gr - 1) == 0
        assert G.norm_route(rows, d) == ("packed", R, C, 8)
        _, x, _, e = G.rms_inputs(rows, d)
        for t in G.pooled_grads(rows // gr, d):
            assert int(t.abs().max()) <= 3
        want = E.rms_dscale_ref(E.expand_groups(G.pooled_grads(rows // gr, d)[0], gr), x, e)
        E.assert_exact_regime(want, G.rms_terms_bound(rows), f"pooled dscale d={d} group_rows={gr}")
        assert POW2_DENOM * gr * 3 * 3 * (1 << (E.POW2_HI - E.POW2_LO)) < 1 << 24          # one term, in units of the smallest
    for ngroups in G.POOLED_NGROUPS:
        gr = G.pooled_fwd_group_rows(ngroups)
        assert gr % R == 0 and gr & (gr - 1) == 0
        assert G.norm_route(ngroups * gr, d) == ("packed", R, C, 8)
    rows = G.packed_rows("loop", R, CUS)
    assert rows // R > 4 * G.packed_blocks_bwd(rows // R, CUS) and (rows // R) % 4
    assert 8 * len(G.probe_rows(rows, R, CUS)) <= d


def test_route_tables_reach_the_kernel_forms_they_name():
    for d, rows in G.ROW_CASES:
        assert G.norm_route(rows, d)[0] == "row"
    for d, rows in G.WIDE_CASES:
        assert G.norm_route(rows, d) == ("wide", 0, 0, 8 if d % 8 == 0 else 1) and rows > G.norm_blocks(rows)
    for d, R, C in G.PACKED:
        for k in G.PACKED_ROWS:
            assert G.norm_route(G.packed_rows(k, R, CUS), d) == ("packed", R, C, 8)
    assert G.BIG_ROWS > 4 * G.norm_blocks(G.BIG_ROWS) and G.BIG_ROWS % 4
    assert E.POW2_PERIOD % 2 and all(E.POW2_PERIOD % R for R in (2, 4))        # coprime to the wave slots and to R


def test_fingerprints_put_each_probe_row_in_its_own_block():
    rows, R = G.packed_rows("loop", 2, CUS), 2
    probes = G.probe_rows(rows, R, CUS)
    per_pass = 4 * G.packed_blocks_bwd(rows // R, CUS) * R
    assert {0, rows - 1, per_pass - 1, per_pass} <= set(probes)
    assert {(p // R) % 4 for p in probes} == {0, 1, 2, 3}                      # every wave slot
    assert any(a + 1 == b and a % R == 0 for a, b in zip(probes, probes[1:]))  # both rows of one packed group
    t = G.fingerprint(rows, 768, probes, 20)
    nz = t.nonzero()
    assert sorted(set(nz[:, 0].tolist())) == probes
    for i, row in enumerate(probes):
        cols = nz[nz[:, 0] == row][:, 1]
        assert cols.tolist() == list(range(8 * i, 8 * i + 8))
    assert bool((np.abs(t.numpy()).sum(0) <= 3).all())                         # a column holds one row
