"""Host side of the guarded optimizer tail (no GPU): the header's declarations as the binding sees them, the workspace size
query, the argument checks that come before any launch, and the two epoch schedulers against torch's."""
import ctypes as C

import pytest
import torch

OK, ERR_ARG, ERR_WORKSPACE = 0, -1, -4
P = C.c_void_p


def test_signatures_are_bound_from_the_header():
    from meant_amd import _lib
    want = {
        "meant_grad_stats_ws": (C.c_size_t, [C.c_int64]),
        "meant_grad_stats_f32": (C.c_int, [P, C.c_int64, P, C.c_int, P, C.c_size_t, P]),
        "meant_optim_step_f32": (C.c_int, [P, P, P, P, C.c_int64, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                           C.c_float, C.c_int, P, P]),
        "meant_optim_finish": (C.c_int, [P, C.c_float, C.c_float, C.c_int, C.c_int, P]),
    }
    for name, (res, args) in want.items():
        assert name in _lib.SIGNATURES, name
        assert _lib.SIGNATURES[name] == (res, args), name
        assert getattr(_lib.lib, name).argtypes == args and getattr(_lib.lib, name).restype == res


def test_constants():
    from meant_amd import _lib
    assert (_lib.OPTIM_ADAMW, _lib.OPTIM_ADAM, _lib.OPTIM_STATE_BYTES) == (0, 1, 64)


def test_grad_stats_workspace_size():
    from meant_amd._lib import lib
    ws = lib.meant_grad_stats_ws
    assert ws(0) == 0 and ws(-1) == 0 and ws(-2 ** 40) == 0
    assert ws(1) > 0 and ws(1) % 16 == 0
    sweep = [1, 2, 3, 4, 5, 4095, 4096, 4097, 8192, 8193, 10 ** 6, 1300003, 2 ** 24, 2 ** 28 - 1, 2 ** 28, 2 ** 28 + 1, 2 ** 31, 2 ** 33 + 7,
             2 ** 40]
    sizes = [ws(n) for n in sweep]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[-1] < 2 ** 24                               # bounded: the span grows instead of the number of partials
    assert ws(4097) > ws(4096)                               # one partial per span of 4096 elements


def test_argument_checks_come_before_any_launch():
    """fake device addresses: every call below has to return from its checks (a launch would fault on them)"""
    from meant_amd import _lib
    lib = _lib.lib
    g, st, w = 0x10000, 0x20000, 0x30000
    need = lib.meant_grad_stats_ws(5000)
    stats = lib.meant_grad_stats_f32
    assert stats(None, 5000, st, 1, w, need, None) == ERR_ARG
    assert stats(g, 5000, None, 1, w, need, None) == ERR_ARG
    assert stats(g, 5000, st, 1, None, need, None) == ERR_ARG
    assert stats(g, -1, st, 1, w, need, None) == ERR_ARG
    assert stats(g + 4, 5000, st, 1, w, need, None) == ERR_ARG           # 16-byte loads of g
    assert stats(g, 5000, st + 4, 1, w, need, None) == ERR_ARG           # the state's 8-byte words
    assert stats(g, 5000, st, 1, w + 8, need, None) == ERR_ARG
    assert stats(g, 5000, st, 1, w, need - 1, None) == ERR_WORKSPACE and b"workspace" in lib.meant_last_error()
    assert stats(g, 5000, st, 1, w, 0, None) == ERR_WORKSPACE
    assert stats(g, 0, st, 1, None, 0, None) == OK                        # n == 0: nothing to do, no launch

    p, m, v = 0x40000, 0x50000, 0x60000
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.01, 1.0, 0)

    def step(p=p, g=g, m=m, v=v, n=100, kind=_lib.OPTIM_ADAMW, st=st):
        return lib.meant_optim_step_f32(p, g, m, v, n, kind, *hyper, st, None)
    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(st=None), dict(n=-1), dict(kind=2), dict(kind=-1),
               dict(p=p + 4), dict(g=g + 8), dict(m=m + 4), dict(v=v + 12), dict(st=st + 4)):
        assert step(**kw) == ERR_ARG, kw
    assert step(n=0) == OK and step(n=0, kind=_lib.OPTIM_ADAM) == OK

    assert lib.meant_optim_finish(None, 2.0, 0.5, 2000, 1, None) == ERR_ARG
    assert lib.meant_optim_finish(st + 4, 2.0, 0.5, 2000, 1, None) == ERR_ARG
    assert lib.meant_optim_finish(st, 2.0, 0.5, 0, 1, None) == ERR_ARG    # a growth interval of 0 would never be reached


class _Opt:
    def __init__(self, lr):
        self.lr = lr


def _torch_pair(make_ref, lr):
    p = torch.nn.Parameter(torch.zeros(1))
    ref_opt = torch.optim.SGD([p], lr=lr)
    return ref_opt, make_ref(ref_opt)


@pytest.mark.parametrize("T_max,eta_min", [(5, 0.0), (7, 1e-6)])
def test_cosine_annealing_matches_torch(T_max, eta_min):
    """every epoch of 2 * T_max + 3 (past T_max torch's recursion climbs back: the closed form is periodic the same way), to the
    1e-12 of the CosineWarmRestarts test, and again after a state_dict round trip into a fresh scheduler"""
    from meant_amd.train import CosineAnnealing
    ref_opt, ref = _torch_pair(lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=T_max, eta_min=eta_min), 5e-5)
    mine = CosineAnnealing(_Opt(5e-5), T_max=T_max, eta_min=eta_min)
    assert abs(mine.opt.lr - ref_opt.param_groups[0]["lr"]) < 1e-12
    again = None
    for epoch in range(1, 2 * T_max + 4):
        ref_opt.step(); ref.step(); mine.step()
        assert abs(mine.opt.lr - ref_opt.param_groups[0]["lr"]) < 1e-12, epoch
        if again is not None:
            again.step()
            assert again.opt.lr == mine.opt.lr and again.epoch == mine.epoch
        if epoch == 3:
            again = CosineAnnealing(_Opt(1.0), T_max=99, eta_min=0.5)
            again.load_state_dict(mine.state_dict())
            assert again.epoch == 3 and again.opt.lr == mine.opt.lr and again.T_max == T_max and again.eta_min == eta_min


@pytest.mark.parametrize("kw", [dict(), dict(start_factor=0.1, end_factor=0.8, total_iters=3)])
def test_linear_lr_matches_torch(kw):
    """torch's defaults (what the reference's bare LinearLR(optimizer) runs) and another ramp, over 8 epochs"""
    from meant_amd.train import LinearLR
    ref_opt, ref = _torch_pair(lambda o: torch.optim.lr_scheduler.LinearLR(o, **kw), 5e-5)
    mine = LinearLR(_Opt(5e-5), **kw)
    assert abs(mine.opt.lr - ref_opt.param_groups[0]["lr"]) < 1e-12        # torch sets base * start_factor at construction
    again = None
    for epoch in range(1, 9):
        ref_opt.step(); ref.step(); mine.step()
        assert abs(mine.opt.lr - ref_opt.param_groups[0]["lr"]) < 1e-12, epoch
        if again is not None:
            again.step()
            assert again.opt.lr == mine.opt.lr
        if epoch == 2:
            again = LinearLR(_Opt(1.0), start_factor=0.5, end_factor=0.6, total_iters=50)
            again.load_state_dict(mine.state_dict())
            assert again.epoch == 2 and again.opt.lr == mine.opt.lr and again.state_dict() == mine.state_dict()
    assert abs(mine.opt.lr - 5e-5 * kw.get("end_factor", 1.0)) < 1e-15
