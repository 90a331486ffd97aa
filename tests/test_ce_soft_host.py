"""Host-side facts of the soft-target loss and the VQA score (no GPU): the two entry points are in the header, the ctypes table and
the built library and their route names exist; bad arguments come back with their status before anything is launched (the
pointers below are made-up addresses that are never dereferenced); vqa_score.from_state -- pure torch on the CPU -- against
hand-derived values; cross_entropy_on_probs refuses a class-probability target of another shape before it looks for a device."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2
SPAN = 1 << 40                                         # distance between the made-up buffers
PROBS, TARGET, ROWS, LOSS, DPROBS, STATE = (SPAN * (i + 1) for i in range(6))
F32, BF16 = 0, 1
ROUTES = ("ce_soft_wave", "ce_soft_block", "vqa_score")


def test_symbols_in_header_table_and_library():
    import meant_amd
    from meant_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "meant_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("meant_ce_probs_soft", "meant_vqa_score_update"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES
        assert re.search(r" T %s$" % name, out, flags=re.M), name
    _lib.route_reset()
    for route in ROUTES:
        assert _lib.route_count(route) == 0
    assert meant_amd.vqa_score is meant_amd.metrics.vqa_score


def _loss(lib, probs=PROBS, ldp=8, target=TARGET, ldt=8, tdtype=F32, rows=ROWS, loss=LOSS, dprobs=DPROBS, ldd=8, B=4, C=8):
    return lib.meant_ce_probs_soft(probs, ldp, target, ldt, tdtype, rows, loss, dprobs, ldd, B, C, None)


def _score(lib, scores=PROBS, lds=8, sdtype=F32, target=TARGET, ldt=8, tdtype=F32, B=4, C=8, state=STATE):
    return lib.meant_vqa_score_update(scores, lds, sdtype, target, ldt, tdtype, B, C, state, None)


@pytest.mark.parametrize("kw", [dict(probs=None), dict(target=None), dict(rows=None), dict(loss=None), dict(B=0), dict(B=-2), dict(C=0, ldp=0),
                                dict(C=-1), dict(ldp=7), dict(ldt=7), dict(ldd=7), dict(C=3129, ldp=3136, ldt=3128, ldd=3129),
                                dict(C=5000, ldp=4999, ldt=5000, ldd=5000), dict(tdtype=2), dict(tdtype=-1), dict(probs=PROBS + 2),
                                dict(target=TARGET + 2), dict(tdtype=BF16, target=TARGET + 1), dict(rows=ROWS + 1), dict(loss=LOSS + 2),
                                dict(dprobs=DPROBS + 2), dict(dprobs=PROBS)])
def test_loss_rejects_bad_arguments_before_any_launch(kw):
    from meant_amd import _lib
    _lib.route_reset()
    assert _loss(_lib.lib, **kw) == ERR_ARG, kw
    assert b"ce_probs_soft" in _lib.lib.meant_last_error()
    assert all(_lib.route_count(r) == 0 for r in ROUTES)


def test_loss_grid_limit():
    """a workgroup per row above C = 1024, four rows per workgroup up to it: 2^31 - 1 workgroups at the most"""
    from meant_amd import _lib
    _lib.route_reset()
    assert _loss(_lib.lib, B=1 << 31, C=3129, ldp=3129, ldt=3129, dprobs=None) == ERR_UNSUPPORTED
    assert b"2^31" in _lib.lib.meant_last_error()
    assert _loss(_lib.lib, B=1 << 33, dprobs=None) == ERR_UNSUPPORTED
    assert _loss(_lib.lib, B=1 << 31, C=0, ldp=0) == ERR_ARG         # the argument checks come first
    assert all(_lib.route_count(r) == 0 for r in ROUTES)


@pytest.mark.parametrize("kw", [dict(scores=None), dict(target=None), dict(state=None), dict(B=-1), dict(C=0, lds=0), dict(C=-4), dict(lds=7),
                                dict(ldt=7), dict(C=3129, lds=3136, ldt=3128), dict(sdtype=3), dict(tdtype=9), dict(scores=PROBS + 2),
                                dict(sdtype=BF16, scores=PROBS + 1), dict(target=TARGET + 1), dict(tdtype=BF16, target=TARGET + 3),
                                dict(state=STATE + 4)])
def test_score_rejects_bad_arguments_before_any_launch(kw):
    from meant_amd import _lib
    _lib.route_reset()
    assert _score(_lib.lib, **kw) == ERR_ARG, kw
    assert b"vqa_score_update" in _lib.lib.meant_last_error()
    assert all(_lib.route_count(r) == 0 for r in ROUTES)


def test_score_row_limit_and_empty_batch():
    from meant_amd import _lib
    _lib.route_reset()
    assert _score(_lib.lib, B=1 << 40) == ERR_UNSUPPORTED
    assert b"2^40" in _lib.lib.meant_last_error()
    assert _score(_lib.lib, B=0) == OK                               # nothing to count: no launch
    assert _score(_lib.lib, B=0, C=3129, lds=3136, ldt=3129, sdtype=BF16, tdtype=BF16) == OK
    assert _score(_lib.lib, B=0, C=0, lds=0) == ERR_ARG              # the argument checks come first
    assert all(_lib.route_count(r) == 0 for r in ROUTES)


def test_from_state_hand_derived():
    """three questions scoring 1.0, 0.3 and 0 : the weights in 2^-32 units are 2^32, round(0.3f * 2^32) and 0, their mean is
    (1 + 0.3f) / 3 with 0.3f the float32 nearest 0.3; the nan and invalid counters do not enter"""
    from meant_amd import vqa_score
    w = float(torch.tensor(0.3, dtype=torch.float32).item())
    fx = (1 << 32) + round(w * 2 ** 32)
    got = vqa_score.from_state(torch.tensor([fx, 3, 1, 5], dtype=torch.int64))
    assert got.dtype == torch.float64 and got.dim() == 0
    assert abs(got.item() - (1.0 + w) / 3) <= 1e-15
    assert vqa_score.from_state(torch.tensor([5 << 31, 5, 0, 0], dtype=torch.int64)).item() == 0.5       # exact
    assert vqa_score.from_state(torch.tensor([0, 0, 0, 7], dtype=torch.int64)).item() == 0.0             # no rows: 0, not NaN
    assert vqa_score.from_state(torch.tensor([[16 << 32, 1], [0, 0]], dtype=torch.int64)).item() == 16.0
    for bad in (torch.zeros(4, dtype=torch.int32), torch.zeros(5, dtype=torch.int64)):
        with pytest.raises(ValueError):
            vqa_score.from_state(bad)
    m = vqa_score("Empty")                                           # never updated: no device touched
    assert m.compute().item() == 0.0 and m.compute().dtype == torch.float64
    assert m.nan_rows() == 0 and m.invalid_rows() == 0
    m.reset()
    assert m.merge(vqa_score()) is m and m.state is None


def test_soft_target_shape_is_checked_before_the_device():
    from meant_amd.train import cross_entropy_on_probs
    probs = torch.rand(4, 7)
    for shape in ((4, 6), (3, 7), (7, 4), (4, 8)):
        with pytest.raises(ValueError, match="shape of probs"):
            cross_entropy_on_probs(probs, torch.zeros(shape))
    with pytest.raises(ValueError):
        cross_entropy_on_probs(probs, torch.zeros(4, 6, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):       # the right shape gets as far as the device check
        cross_entropy_on_probs(probs, torch.zeros(4, 7))


def test_vqa_score_update_checks_types_and_shapes_first():
    from meant_amd import vqa_score
    m = vqa_score()
    with pytest.raises(TypeError):
        m.update(torch.rand(4, 7), torch.zeros(4, 7, dtype=torch.int64))
    with pytest.raises(TypeError):
        m.update(torch.zeros(4, dtype=torch.int64), torch.zeros(4, 7))
    with pytest.raises(ValueError):
        m.update(torch.rand(4, 7), torch.zeros(4, 6))
    with pytest.raises(ValueError):
        m.update(torch.rand(7), torch.zeros(7))
    assert m.state is None
