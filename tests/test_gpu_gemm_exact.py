"""Every GEMM route at the C ABI on small-integer operands, at ZERO tolerance (tests/exact_ref.py): all products and partial sums are
integers below 2^24, so MFMA accumulation, float atomics, split-K and stolen tiles give the same bits and the output must equal the
int64 reference exactly; one dropped, doubled or misplaced term moves an element by >= 1 (tests/test_gemm_exact_host.py shows which
mutants the relative bounds of the other GEMM tests accept).  Inputs are column slices of wider NaN-poisoned buffers, outputs sit in
sentinel-filled buffers whose guard must survive, and every case asserts the WHOLE route table, so each shape provably reaches the
kernel it is meant for.  Shapes are the smallest that reach a route and follow meant_num_cus() where the dispatch does.
(nn.Linear call sites meant/meant.py:59-64,101-107, meant/attention.py:31-40; activations are compared with float64 on the exact
pre-activation under a derived bound.)

MEANT_EXACT_ROUTES_LOG=<file>: append one line per case (shape, options, route table, pass / fail, seconds) --
profiles/gemm_exact_routes.txt is such a run."""
import math
import os
import time
from contextlib import contextmanager
from functools import lru_cache

import pytest
import torch

from tests.exact_ref import assert_exact, assert_guard, ints, mm, to_dev

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
ROUTES = ("nt128", "nt128k", "nt256", "nt256k", "nt256s", "nt256s_rot", "nt_split", "nt_overlap", "nt_rot", "tn128", "tn256", "tn256_det",
          "tn256_rows", "tn_tail", "gemm_f32")
OPTS = {"nt_dynamic": 1, "nt_grid_cap": 0, "nt_stream": 1, "deterministic": 0, "nt_ragged": 1}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture()
def L():
    from meant_amd import _lib
    saved = {k: _lib.get_option(k) for k in OPTS}
    for k, v in OPTS.items():
        _lib.set_option(k, v)                        # the route tables below are about the default dispatch, whatever the environment says
    _lib.route_reset()
    yield _lib
    for k, v in saved.items():
        _lib.set_option(k, v)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@contextmanager
def case(L, what, **opts):
    """one logged case: sets the options, resets the counters; c.routes(...) asserts the whole table"""
    for k, v in {**OPTS, **opts}.items():
        L.set_option(k, v)
    L.route_reset()

    class C:
        table = {}

        def routes(self, **want):
            torch.cuda.synchronize()
            exp = dict.fromkeys(ROUTES, 0)
            exp.update(want)
            got = {r: L.route_count(r) for r in ROUTES}
            self.table = {r: n for r, n in got.items() if n}
            assert got == exp, f"{what}: routes {self.table}, expected {want}"
            L.route_reset()

    c, t0, status = C(), time.perf_counter(), "FAIL"
    try:
        yield c
        status = "pass"
    finally:
        for k, v in OPTS.items():
            L.set_option(k, v)
        path = os.environ.get("MEANT_EXACT_ROUTES_LOG")
        if path:
            o = " ".join(f"{k}={v}" for k, v in opts.items()) or "defaults"
            with open(path, "a") as f:
                f.write(f"{what} | {o} | {c.table} | {status} | {time.perf_counter() - t0:.2f} s\n")


def tall_m(cus, N, extra=0):
    """smallest M, a multiple of 256, that takes 256 x 256 tiles at width N:  M >= 1024 && 2 * ceil(M / 256) * (N / 256) >= CUs"""
    assert N % 256 == 0
    return 256 * max(4, -(-cus // (2 * (N // 256)))) + extra


def tall(L, N, extra=0):
    return tall_m(L.lib.meant_num_cus(), N, extra)


# the tables of the cases (tests/test_gemm_exact_host.py walks them and asserts the preconditions of every reference on the CPU)
FWD_NT128 = [(1, 8, 64), (127, 72, 64), (129, 136, 128), (129, 8, 64), (1, 136, 192), (300, 264, 64)]
FWD_NT128K = [(129, 136, 8), (127, 72, 72), (1, 8, 200), (129, 136, 200)]
FWD_NT256 = [(64, 1), (128, 1), (192, 1), (256, 0)]                        # (K, nt_stream)
FWD_NT256K = [200, 264]
FWD_NT256S = [(256, 1), (320, 1), (768, 1), (768, 0)]                      # (K, nt_dynamic)
RAGGED = [1, 100, 255]
ACT = [("nt128", 64, 0, {}), ("nt128k", 72, 0, {}), ("nt256", 128, 0, {}), ("nt256k", 200, 0, {}), ("nt256s", 256, 0, {}),
       ("nt_overlap", 256, 100, {}), ("nt_split", 256, 100, {"nt_ragged": 0})]
ACT_DENS, ACT_SEED, FEW_SEED, RAGGED_SEED = 0.15, 11, 5, 7
DX_ONE = [(129, 8, 136, None, "nt128k"), (127, 72, 72, None, "nt128k"), (129, 256, 136, None, "nt128"), (1, 320, 8, None, "nt128"),
          (129, 256, 100, 104, "nt128"), (129, 72, 100, 101, "nt128k"), (300, 320, 100, 100, "nt128")]
DX_TALL = [(64, 0, {}, dict(nt256=1)), (72, 0, {}, dict(nt256k=1)), (256, 0, {}, dict(nt256s=1)), (320, 0, {}, dict(nt256s=1)),
           (256, 100, {}, dict(nt256s=1, nt_overlap=1)), (256, 100, {"nt_ragged": 0}, dict(nt256s=1, nt_split=1, nt128=1))]
QKV_STREAM = [(512, 256, 1), (512, 768, 1), (512, 768, 0), (196, 256, 1)]   # (S, K, nt_dynamic) at H, Dh, R = 4, 64, 32
QKV_ONE = [(64, "nt128"), (72, "nt128k"), (200, "nt128k")]                  # K at G, S, H, Dh, R = 3, 24, 2, 16, 8
QKV_TALL_ONE_TILE = [(128, "nt256"), (200, "nt256k")]                       # K at the S = 512 shape of QKV_STREAM
EXT = ["nt256s", "nt_overlap", "nt128"]
DW_TN128 = [(64, 8, 136), (128, 72, 72), (320, 136, 8), (1024, 72, 136), (1024, 264, 136)]
DW_TN_TAIL = [(1, 72, 136), (63, 136, 72), (64 + 37, 72, 72), (320 + 37, 136, 136)]
DW_TN256_M, DW_TN256_NK = [4096, 4288, 4288 + 37], [(256, 256), (512, 256), (256, 512)]
DW_ROWS_M = [4096, 4288]                                                    # the row-list cases, at N, K = 256, 512


def few_workgroups_shape(cus):
    return max(tall_m(cus, 1024), 16384), 1024, 512


def qkv_stream_shape(cus, S):
    H, Dh, R = 4, 64, 32
    G = -(-tall_m(cus, 3 * H * Dh) // S)
    while (G * S) % 256:
        G += 1
    return G, S, H, Dh, R


def qkv_live_shape(cus):
    S, H, Dh, R, K = 512, 8, 64, 32, 768
    return -(-(tall_m(cus, H * Dh) // 256) // 2), S, H, Dh, R, K


def ext_shape(cus, kind):
    return {"nt256s": (tall_m(cus, 512), 512, 512), "nt_overlap": (tall_m(cus, 512, 104), 512, 512), "nt128": (200, 192, 64)}[kind]


def fwd_wants(M, N, K, dens=0.5, seed=1):
    """the int64 references of the three variants of a forward case: plain, with bias, with bias and residual"""
    pre = _xw(M, N, K, dens, seed)[2]
    b, r = _ints((N,), -3, 3, 1.0, seed + 2), _ints((M, N), -4, 4, 0.7, seed + 3)
    return pre, pre + b, pre + b + r


@lru_cache(maxsize=12)
def _ints(shape, lo=-1, hi=1, density=0.5, seed=0):
    return ints(shape, lo, hi, density, seed)


@lru_cache(maxsize=3)
def _xw(M, N, K, dens, seed):
    """operands of one product and its int64 result, computed once for the variants of a case"""
    x, w = ints((M, K), density=dens, seed=seed), ints((N, K), density=dens, seed=seed + 1)
    return x, w, mm(x, w.t())


# ---- a / b: forward ---------------------------------------------------------------------------------------------------------------

def _gelu64(p):
    return 0.5 * p * (1.0 + torch.special.erf(p / math.sqrt(2.0)))


def assert_act(y, pre, kind, what):
    """|y - act(pre)| <= 2^-8 |ref| + 1e-6 max(1, |pre|): one bf16 rounding in either mode, plus the 7.5e-8 of the rational Phi /
    the fast exp with fp32 rounding on top"""
    p = pre.double()
    ref = _gelu64(p) if kind == "gelu" else torch.sigmoid(p)
    err = (y.detach().cpu().double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 1e-6 * p.abs().clamp(min=1.0)
    over = err > bound                                    # NaN compares false: caught below
    assert not bool(over.any()) and not bool(torch.isnan(err).any()), \
        f"{what}: {int(over.sum())} elements over the bound, worst excess {(err - bound).max().item():.3e} at pre = {p.reshape(-1)[(err - bound).argmax()].item():g}"


def run_fwd(L, dev, M, N, K, *, bias=True, res=None, act=None, preact=False, dens=0.5, seed=1, dtype=BF, ldx=None, ldy=None, what=""):
    """meant_linear_fwd on integers; returns (y view, int64 pre-activation incl. bias, int64 expected y or None for activations)"""
    x, w, pre = _xw(M, N, K, dens, seed)
    ldx = K + 8 if ldx is None else ldx
    ldy = N + 8 if ldy is None else ldy
    xd, _ = to_dev(x, dtype, dev, ld=ldx)
    wd, _ = to_dev(w, dtype, dev)                          # the ABI fixes w's row stride at K: dense, NaN behind row N
    bd = None
    if bias:
        b = _ints((N,), -3, 3, 1.0, seed + 2)
        pre = pre + b
        bd = b.float().to(dev)
    yv, ybuf = to_dev(None, dtype, dev, ld=ldy, sentinel=True, rows=M, cols=N)
    r, rptr, ldr = None, None, 0
    if res:
        r = _ints((M, N), -4, 4, 0.7, seed + 3)
        if res == "inplace":
            yv.copy_(r.to(dtype))
            rptr, ldr = yv.data_ptr(), ldy
        else:
            ldr = ldy if res == "same_ld" else N + 16      # ldr != ldy
            rv, _ = to_dev(r, dtype, dev, ld=ldr)
            rptr = rv.data_ptr()
    pv = pbuf = None
    if preact:
        pv, pbuf = to_dev(None, dtype, dev, ld=ldy, sentinel=True, rows=M, cols=N)
    epi = {None: 0, "gelu": L.EPI_GELU, "sigmoid": L.EPI_SIGMOID}[act] | (L.EPI_RESIDUAL if res else 0)
    L.check(L.lib.meant_linear_fwd(xd.data_ptr(), ldx, wd.data_ptr(), bd.data_ptr() if bias else None, rptr, ldr, yv.data_ptr(), ldy,
                                   pv.data_ptr() if preact else None, M, N, K, epi, 1 if dtype == BF else 0, _stream()), "linear_fwd")
    torch.cuda.synchronize()
    tag = f"{what} fwd ({M},{N},{K}) bias={bias} res={res} act={act}"
    assert_guard(ybuf, M, N, tag + " y")
    if preact:
        assert_exact(pv, pre, tag + " preact")
        assert_guard(pbuf, M, N, tag + " preact")
    if act:
        assert res is None
        assert_act(yv, pre, act, tag)
        return yv, pre, None
    want = pre + r if res else pre
    assert_exact(yv, want, tag)
    return yv, pre, want


def fwd_variants(L, dev, c, M, N, K, routes, **kw):
    """plain, with bias, with bias and a residual of its own row stride: the same route table each time"""
    for bias, res in ((False, None), (True, None), (True, "sep")):
        run_fwd(L, dev, M, N, K, bias=bias, res=res, **kw)
        c.routes(**routes)


def test_canary_single_tile_nt128(L, dev):
    """the method's one unmeasured assumption: the bf16 MFMA accumulates integer products below 2^24 without loss"""
    with case(L, "canary nt128 (128,128,64)") as c:
        run_fwd(L, dev, 128, 128, 64, bias=False)
        c.routes(nt128=1)


@pytest.mark.parametrize("M,N,K", FWD_NT128)
def test_fwd_nt128(L, dev, M, N, K):
    """one tile and its neighbours: edge rows clamped, edge columns below a 16-byte store"""
    with case(L, f"fwd nt128 ({M},{N},{K})") as c:
        fwd_variants(L, dev, c, M, N, K, dict(nt128=1))


@pytest.mark.parametrize("M,N,K", FWD_NT128K)
def test_fwd_nt128k(L, dev, M, N, K):
    """K % 64 != 0: the K-tail form reads neither operand at or beyond column K (x carries NaN there)"""
    with case(L, f"fwd nt128k ({M},{N},{K})") as c:
        fwd_variants(L, dev, c, M, N, K, dict(nt128k=1))


@pytest.mark.parametrize("K,stream", FWD_NT256)
def test_fwd_nt256(L, dev, K, stream):
    """fewer than four K-steps, or nt_stream = 0: the one-tile 256 x 256 kernel"""
    M = tall(L, 512)
    with case(L, f"fwd nt256 ({M},512,{K})", nt_stream=stream) as c:
        fwd_variants(L, dev, c, M, 512, K, dict(nt256=1))


@pytest.mark.parametrize("K", FWD_NT256K)
def test_fwd_nt256k(L, dev, K):
    M = tall(L, 512)
    with case(L, f"fwd nt256k ({M},512,{K})") as c:
        fwd_variants(L, dev, c, M, 512, K, dict(nt256k=1))


@pytest.mark.parametrize("K,dynamic", FWD_NT256S)
def test_fwd_nt256s(L, dev, K, dynamic):
    """the streaming kernel from its four-step minimum on; K = 768 has the >= 8 steps the dynamic draw needs"""
    M = tall(L, 512)
    with case(L, f"fwd nt256s ({M},512,{K})", nt_dynamic=dynamic) as c:
        fwd_variants(L, dev, c, M, 512, K, dict(nt256s=1))


@pytest.mark.parametrize("dynamic", [1, 3])
def test_fwd_nt256s_few_workgroups(L, dev, dynamic):
    """64 workgroups on >= 256 tiles: four or more tiles each through the draw; nt_dynamic = 3 leaves seven of the eight counters to the
    steal path, whose counter must move"""
    M, N, K = few_workgroups_shape(L.lib.meant_num_cus())
    assert (M // 256) * (N // 256) >= 256 and K == 512
    with case(L, f"fwd nt256s ({M},{N},512) 64 workgroups", nt_dynamic=dynamic, nt_grid_cap=64) as c:
        before = L.lib.meant_debug_nt_steals()
        for bias, res in ((False, None), (True, "sep")):
            run_fwd(L, dev, M, N, 512, bias=bias, res=res, seed=FEW_SEED)
            c.routes(nt256s=1)
        stolen = L.lib.meant_debug_nt_steals() - before
        if dynamic == 3:
            assert stolen > 0, "no tile went through the steal path"


@pytest.mark.parametrize("extra", RAGGED)
def test_fwd_ragged_overlap_and_split(L, dev, extra):
    """M = 256 k + extra: the overlapped last tile, the head + tail split (nt_ragged = 0), bit-equal to each other, and the in-place
    residual that must fall back to the split"""
    M = tall(L, 512, extra)
    ys = {}
    for ragged, routes in ((1, dict(nt256s=1, nt_overlap=1)), (0, dict(nt256s=1, nt_split=1, nt128=1))):
        with case(L, f"fwd {'nt_overlap' if ragged else 'nt_split'} ({M},512,256)", nt_ragged=ragged) as c:
            for bias, res in ((False, None), (True, None), (True, "sep")):
                y, _, _ = run_fwd(L, dev, M, 512, 256, bias=bias, res=res, seed=RAGGED_SEED)
                c.routes(**routes)
                ys[ragged, bias, res] = y.clone()
    for (ragged, bias, res), y in ys.items():
        if ragged:
            assert torch.equal(y.view(torch.int16), ys[0, bias, res].view(torch.int16)), "overlap and split differ in bits"
    with case(L, f"fwd nt_split in place ({M},512,256)") as c:
        run_fwd(L, dev, M, 512, 256, res="inplace", seed=RAGGED_SEED)
        c.routes(nt256s=1, nt_split=1, nt128=1)


@pytest.mark.parametrize("act", ["gelu", "sigmoid"])
@pytest.mark.parametrize("route,K,extra,opts", ACT)
def test_fwd_activation_epilogues(L, dev, act, route, K, extra, opts):
    """exact pre-activation copy; y against float64 act(pre) under the derived bound.  Sparse operands keep pre where the activations
    bend (|pre| of a few units)"""
    small = route in ("nt128", "nt128k")
    M, N = (129, 136) if small else (tall(L, 512, extra), 512)
    want = {"nt_overlap": dict(nt256s=1, nt_overlap=1), "nt_split": dict(nt256s=1, nt_split=1, nt128=1)}.get(route, {route: 1})
    with case(L, f"fwd {route} {act} ({M},{N},{K})", **opts) as c:
        run_fwd(L, dev, M, N, K, act=act, preact=(act == "gelu"), dens=ACT_DENS, seed=ACT_SEED)
        c.routes(**want)


# ---- c: dX --------------------------------------------------------------------------------------------------------------------------

def run_dx(L, dev, M, N, K, *, lddx=None, dens=0.5, seed=21, dtype=BF, lddy=None, what=""):
    """dx[M, K] = dy[M, N] w[N, K]; wT [K, N] dense.  The reduction length is N."""
    dy, wT, want = _xw(M, K, N, dens, seed)
    lddy = N + 8 if lddy is None else lddy
    lddx = K + 8 if lddx is None else lddx
    dyd, _ = to_dev(dy, dtype, dev, ld=lddy)
    wd, _ = to_dev(wT, dtype, dev)
    dxv, dxbuf = to_dev(None, dtype, dev, ld=lddx, sentinel=True, rows=M, cols=K)
    L.check(L.lib.meant_linear_bwd_dx(dyd.data_ptr(), lddy, wd.data_ptr(), dxv.data_ptr(), lddx, M, N, K, 1 if dtype == BF else 0, _stream()),
            "linear_bwd_dx")
    torch.cuda.synchronize()
    tag = f"{what} dx ({M},{N},{K}) lddx={lddx}"
    assert_guard(dxbuf, M, K, tag)
    assert_exact(dxv, want, tag)
    return dxv


@pytest.mark.parametrize("M,N,K,lddx,route", DX_ONE)
def test_dx_one_tile(L, dev, M, N, K, lddx, route):
    """reduction lengths 8, 72 (K-tail forms), 256, 320 (plain); output widths off a multiple of 8 store element by element"""
    with case(L, f"dx {route} ({M},{N},{K}) lddx={lddx}") as c:
        run_dx(L, dev, M, N, K, lddx=lddx)
        c.routes(**{route: 1})


@pytest.mark.parametrize("N,extra,opts,routes", DX_TALL)
def test_dx_tall(L, dev, N, extra, opts, routes):
    M = tall(L, 512, extra)
    with case(L, f"dx {'+'.join(routes)} ({M},{N},512)", **opts) as c:
        run_dx(L, dev, M, N, 512)
        c.routes(**routes)


# ---- d / e: dW ----------------------------------------------------------------------------------------------------------------------

def dw_operands(dev, M, N, K, *, dens=0.5, seed=31, lddy=None, ldx=None, dtype=BF, live_rows=None):
    dy, x = _ints((M, N), density=dens, seed=seed), _ints((M, K), density=dens, seed=seed + 1)
    if live_rows is not None:
        dy = dy * live_rows[:, None]
    lddy = N + 8 if lddy is None else lddy
    ldx = K + 8 if ldx is None else ldx
    dyd, _ = to_dev(dy, dtype, dev, ld=lddy)
    xd, _ = to_dev(x, dtype, dev, ld=ldx)
    return dy, x, dyd, xd, lddy, ldx


def run_dw(L, dev, M, N, K, *, dbias=True, rows=None, ops=None, what="", dtype=BF, **kw):
    """meant_linear_bwd_dw (or _rows with rows = (list ptr, count ptr)) into pre-loaded accumulators: the contract is "+=" """
    dy, x, dyd, xd, lddy, ldx = ops if ops is not None else dw_operands(dev, M, N, K, dtype=dtype, **kw)
    dw0, db0 = _ints((N, K), -5, 5, 1.0, 41), _ints((1, N), -5, 5, 1.0, 42)
    dwv, dwbuf = to_dev(dw0, F32, dev, sentinel=True)                      # dense [N, K] by the ABI; sentinel row behind it
    dbv, dbbuf = to_dev(db0, F32, dev, ld=N + 8, sentinel=True, tail_rows=0)
    dt = 1 if dtype == BF else 0
    wsb = L.lib.meant_linear_bwd_dw_ws(M, N, K, dt)
    ws = torch.empty(max(wsb, 16), device=dev, dtype=torch.uint8)
    if rows is None:
        L.check(L.lib.meant_linear_bwd_dw(dyd.data_ptr(), lddy, xd.data_ptr(), ldx, dwv.data_ptr(), dbv.data_ptr() if dbias else None, M, N, K,
                                          dt, ws.data_ptr() if wsb else None, wsb, _stream()), "linear_bwd_dw")
    else:
        L.check(L.lib.meant_linear_bwd_dw_rows(dyd.data_ptr(), lddy, xd.data_ptr(), ldx, dwv.data_ptr(), dbv.data_ptr() if dbias else None,
                                               rows[0], rows[1], M, N, K, dt, ws.data_ptr() if wsb else None, wsb, _stream()), "linear_bwd_dw_rows")
    torch.cuda.synchronize()
    tag = f"{what} dw ({M},{N},{K}) dbias={dbias}"
    assert_guard(dwbuf, N, K, tag + " dw")
    assert_guard(dbbuf, 1, N, tag + " dbias")
    assert_exact(dwv, dw0 + mm(dy.t(), x), tag + " dw")
    assert_exact(dbv, db0 + dy.sum(0, keepdim=True) if dbias else db0, tag + " dbias")
    return dwv


@pytest.mark.parametrize("det", [0, 1], ids=["atomics", "det"])
@pytest.mark.parametrize("M,N,K", DW_TN128)
def test_dw_tn128(L, dev, M, N, K, det):
    """128 x 128 dW kernel; 320 and 1024 rows split unevenly over the token axis (64-row units)"""
    with case(L, f"dw tn128 ({M},{N},{K})", deterministic=det) as c:
        for dbias in (True, False):
            run_dw(L, dev, M, N, K, dbias=dbias)
            c.routes(tn128=1)


@pytest.mark.parametrize("M,N,K", DW_TN_TAIL)
def test_dw_tn_tail(L, dev, M, N, K):
    """fewer than 64 trailing token rows go through the exact engine into the same accumulators"""
    with case(L, f"dw tn_tail ({M},{N},{K})") as c:
        run_dw(L, dev, M, N, K)
        c.routes(tn_tail=1, gemm_f32=1, **({"tn128": 1} if M >= 64 else {}))


@pytest.mark.parametrize("det", [0, 1], ids=["atomics", "det"])
@pytest.mark.parametrize("M", DW_TN256_M)
@pytest.mark.parametrize("N,K", DW_TN256_NK)
def test_dw_tn256(L, dev, M, N, K, det):
    """256 x 256 dW kernel: even splits, the uneven splits of 67 blocks, a tail behind them; atomics and ordered partial sums both equal
    the integers, hence each other"""
    tail = dict(tn_tail=1, gemm_f32=1) if M % 64 else {}
    with case(L, f"dw {'tn256_det' if det else 'tn256'} ({M},{N},{K})", deterministic=det) as c:
        for dbias in (True, False):
            run_dw(L, dev, M, N, K, dbias=dbias)
            c.routes(**{"tn256_det" if det else "tn256": 1}, **tail)


def _blocks_case(L, dev, c, M, blocks, rows, det, what, live_rows=None):
    """dy is zero outside the listed blocks, x is not"""
    live = torch.zeros(M, dtype=torch.int64)
    for b in blocks:
        live[64 * b:64 * b + 64] = 1
    if live_rows is not None:
        assert bool((live_rows <= live).all())
        live = live_rows
    ops = dw_operands(dev, M, 256, 512, live_rows=live, seed=51)
    assert bool((ops[1] != 0).any(dim=1)[live == 0].any()) or len(blocks) == M // 64
    run_dw(L, dev, M, 256, 512, rows=rows, ops=ops, what=what)
    c.routes(**({"tn256_det": 1} if det else {"tn256_rows": 1}))


@pytest.mark.parametrize("det", [0, 1], ids=["list", "det"])
@pytest.mark.parametrize("M", DW_ROWS_M)
@pytest.mark.parametrize("pick", ["one", "all", "alternate", "last"])
def test_dw_rows_hand_made_lists(L, dev, M, pick, det):
    nblk = M // 64
    blocks = {"one": [5], "all": list(range(nblk)), "alternate": list(range(0, nblk, 2)), "last": [nblk - 1]}[pick]
    lst = torch.tensor(blocks + [0] * (nblk - len(blocks)), dtype=torch.int32, device=dev)
    cnt = torch.tensor([len(blocks)], dtype=torch.int32, device=dev)
    with case(L, f"dw tn256_rows ({M},256,512) {pick}", deterministic=det) as c:
        _blocks_case(L, dev, c, M, blocks, (lst.data_ptr(), cnt.data_ptr()), det, pick)


def test_dw_rows_a_skipped_block_of_one_live_row_shows(L, dev):
    """the sensitivity of the method on the device: a list that leaves out a block whose dy holds ONE non-zero row (against the
    contract, on purpose: the kernel reads the listed blocks only) must fail the exact comparison -- the defect the relative bounds
    let through (tests/test_gemm_exact_host.py)"""
    M, skipped = 4096, 7
    live = torch.ones(M, dtype=torch.int64)
    live[64 * skipped + 1:64 * skipped + 64] = 0
    ops = dw_operands(dev, M, 256, 512, live_rows=live, seed=51)
    assert bool(ops[0][64 * skipped].any()) and bool(ops[1][64 * skipped].any())
    blocks = [b for b in range(M // 64) if b != skipped]
    lst = torch.tensor(blocks + [0], dtype=torch.int32, device=dev)
    cnt = torch.tensor([len(blocks)], dtype=torch.int32, device=dev)
    with case(L, f"dw tn256_rows ({M},256,512) one-row block left out: rejected") as c:
        with pytest.raises(AssertionError, match=r" dw: \d+ of 131072 elements wrong; first at .*got - want = -?1 "):
            run_dw(L, dev, M, 256, 512, rows=(lst.data_ptr(), cnt.data_ptr()), ops=ops)
        c.routes(tn256_rows=1)


@pytest.mark.parametrize("det", [0, 1], ids=["list", "det"])
@pytest.mark.parametrize("mask", ["suffix", "holes"])
def test_dw_rows_lists_of_kv_live_rows(L, dev, mask, det):
    """the lists meant_kv_live_rows makes from key masks (G = 4 sequences of 1024 tokens); dy lives on the unmasked rows only, so
    blocks at a mask edge hold few rows"""
    G, S = 4, 1024
    km = torch.ones(G, S)
    if mask == "suffix":
        for g, n in enumerate((1024, 65, 513, 1)):
            km[g, n:] = 0
    else:
        km[0, 64:192] = 0
        km[1, 3:1000] = 0
        km[2, 256:512] = 0
        km[3, 100:101] = 0
    kmb = km.view(G * S // 64, 64)
    blocks = [b for b in range(G * S // 64) if kmb[b].any()]                # every sequence keeps a live key: a block is dead iff all its keys are padding
    nbytes = L.lib.meant_kv_live_rows_ws(G, S)
    lists = torch.zeros(nbytes // 4, dtype=torch.int32, device=dev)
    kmd = km.to(dev)
    L.check(L.lib.meant_kv_live_rows(kmd.data_ptr(), G, S, 0, lists.data_ptr(), nbytes, _stream()), "kv_live_rows")
    torch.cuda.synchronize()
    hdr = L.KV_LIST_HDR
    assert lists[0].item() == len(blocks) and lists[hdr:hdr + len(blocks)].tolist() == blocks
    with case(L, f"dw tn256_rows (4096,256,512) kv_live_rows {mask}", deterministic=det) as c:
        _blocks_case(L, dev, c, G * S, blocks, (lists.data_ptr() + 4 * hdr, lists.data_ptr()), det, mask, live_rows=km.view(-1).to(torch.int64))


# ---- f: fused projection with the rotary epilogue --------------------------------------------------------------------------------------

def rot_tables(S, R):
    """quarter turns times a power-of-two xPos scale, doubled into integers: 2 (cos, sin) s for q and 2 (cos, sin) / s for k, s in
    {1/2, 1, 2} by position; every entry of the real tables is in {0, +-1/2, +-1, +-2}"""
    pos, j = torch.arange(S)[:, None], torch.arange(R // 2)[None, :]
    turn = (pos + j) % 4
    cos2 = torch.tensor([2, 0, -2, 0])[turn]
    sin2 = torch.tensor([0, 2, 0, -2])[turn]
    e = (pos % 3) - 1                                                      # s = 2^e
    up = lambda v, e_: torch.where(e_ > 0, v * 2, torch.where(e_ < 0, v // 2, v))
    rep = lambda v: v.repeat_interleave(2, dim=1).to(torch.int64)
    return rep(up(cos2, e)), rep(up(sin2, e)), rep(up(cos2, -e)), rep(up(sin2, -e))     # 2 qa, 2 qb, 2 ka, 2 kb  [S, R]


def rot_ref2(t, S, H, Dh, R, tabs2):
    """2 x the formula of meant_rotary_qk on the integer projection t [M, 3 H Dh]: out[c] = t[c] A[pos, c] + rot(t)[c] B[pos, c],
    rot(t)[2j] = -t[2j+1], rot(t)[2j+1] = t[2j], lanes c < R of the q and k heads"""
    M = t.shape[0]
    v = t.view(M // S, S, 3, H, Dh).clone()
    out = 2 * v
    for sec, (A2, B2) in enumerate(((tabs2[0], tabs2[1]), (tabs2[2], tabs2[3]))):
        tt = v[:, :, sec, :, :R]
        rt = torch.empty_like(tt)
        rt[..., 0::2] = -tt[..., 1::2]
        rt[..., 1::2] = tt[..., 0::2]
        out[:, :, sec, :, :R] = tt * A2[None, :, None, :] + rt * B2[None, :, None, :]
    return out.reshape(M, 3 * H * Dh)


@lru_cache(maxsize=1)
def _qkv_ref(G, S, H, Dh, R, K, dens, seed):
    M, D = G * S, H * Dh
    x, w, b = ints((M, K), density=dens, seed=seed), ints((3 * D, K), density=dens, seed=seed + 1), ints((3 * D,), -2, 2, 1.0, seed + 2)
    tabs2 = rot_tables(S, R)
    return x, w, b, tabs2, rot_ref2(mm(x, w.t()) + b, S, H, Dh, R, tabs2)


def run_qkv(L, dev, G, S, H, Dh, R, K, *, lists=None, dens=0.2, seed=61):
    M, D = G * S, H * Dh
    x, w, b, tabs2, want2 = _qkv_ref(G, S, H, Dh, R, K, dens, seed)
    xd, _ = to_dev(x, BF, dev, ld=K + 8)
    wd, _ = to_dev(w, BF, dev)
    bd = b.float().to(dev)
    td = [(t2.double() / 2).float().to(dev).contiguous() for t2 in tabs2]
    ov, obuf = to_dev(None, BF, dev, sentinel=True, rows=M, cols=3 * D)     # the ABI packs qkv densely; sentinel row behind it
    args = (xd.data_ptr(), K + 8, wd.data_ptr(), bd.data_ptr(), ov.data_ptr(), M, K, S, H, Dh, R, *[t.data_ptr() for t in td])
    if lists is None:
        L.check(L.lib.meant_qkv_proj_fwd(*args, 1, _stream()), "qkv_proj_fwd")
    else:
        L.check(L.lib.meant_qkv_proj_fwd_live(*args, lists.data_ptr(), 1, _stream()), "qkv_proj_fwd_live")
    torch.cuda.synchronize()
    assert_guard(obuf, M, 3 * D, "qkv")
    return ov, want2


@pytest.mark.parametrize("S,K,dynamic", QKV_STREAM)
def test_qkv_rot_streaming(L, dev, S, K, dynamic):
    """nt256s_rot: S = 512 walks the row panels by position range, S = 196 does not; R = 32 < Dh = 64"""
    G, S, H, Dh, R = qkv_stream_shape(L.lib.meant_num_cus(), S)
    with case(L, f"qkv nt256s_rot G={G} S={S} H={H} Dh={Dh} R={R} K={K}", nt_dynamic=dynamic) as c:
        ov, want2 = run_qkv(L, dev, G, S, H, Dh, R, K)
        c.routes(nt256s_rot=1, nt_rot=1)
        assert_exact(ov, want2, "qkv", denom=2)


@pytest.mark.parametrize("K,route", QKV_TALL_ONE_TILE)
def test_qkv_rot_tall_one_tile_kernels(L, dev, K, route):
    """the rotary epilogue of the 256 x 256 one-tile kernel and of its K-tail form (K % 64 != 0)"""
    G, S, H, Dh, R = qkv_stream_shape(L.lib.meant_num_cus(), 512)
    with case(L, f"qkv {route} G={G} S={S} H={H} Dh={Dh} R={R} K={K}") as c:
        ov, want2 = run_qkv(L, dev, G, S, H, Dh, R, K)
        c.routes(**{route: 1}, nt_rot=1)
        assert_exact(ov, want2, "qkv", denom=2)


@pytest.mark.parametrize("K,route", QKV_ONE)
def test_qkv_rot_one_tile(L, dev, K, route):
    with case(L, f"qkv {route} G=3 S=24 H=2 Dh=16 R=8 K={K}") as c:
        ov, want2 = run_qkv(L, dev, 3, 24, 2, 16, 8, K)
        c.routes(**{route: 1}, nt_rot=1)
        assert_exact(ov, want2, "qkv", denom=2)


@pytest.mark.parametrize("dynamic", [1, 0])
def test_qkv_rot_live_panels(L, dev, dynamic):
    """live lists: the k | v columns of dead panels are exact zeros, everything else is the plain call bit for bit (two streaming
    launches: q over all panels, k | v over the live ones)"""
    G, S, H, Dh, R, K = qkv_live_shape(L.lib.meant_num_cus())
    D, M = H * Dh, G * S
    km = torch.ones(G, S)
    km[1, 200:] = 0                       # second panel of sequence 1 dead
    km[2, 256:] = 0
    km[G - 1, 1:] = 0
    dead = [p for p in range(M // 256) if not km.view(-1, 256)[p].any()]
    assert len(dead) >= 3
    nbytes = L.lib.meant_kv_live_rows_ws(G, S)
    lists = torch.zeros(nbytes // 4, dtype=torch.int32, device=dev)
    kmd = km.to(dev)
    L.check(L.lib.meant_kv_live_rows(kmd.data_ptr(), G, S, 0, lists.data_ptr(), nbytes, _stream()), "kv_live_rows")
    torch.cuda.synchronize()
    assert lists[2].item() == len(dead) and lists[1].item() == M // 256 - len(dead)
    with case(L, f"qkv live nt256s_rot G={G} S={S} H={H} Dh={Dh} R={R} K={K}", nt_dynamic=dynamic) as c:
        plain, want2 = run_qkv(L, dev, G, S, H, Dh, R, K)
        c.routes(nt256s_rot=1, nt_rot=1)
        assert_exact(plain, want2, "qkv plain", denom=2)
        live, _ = run_qkv(L, dev, G, S, H, Dh, R, K, lists=lists)
        c.routes(nt256s_rot=2, nt_rot=2)
        exp = plain.clone()
        for p in dead:
            exp[256 * p:256 * p + 256, D:] = 0
        assert torch.equal(live.view(torch.int16), exp.view(torch.int16)), "live-list projection differs from the plain one"


# ---- g: extended epilogue ----------------------------------------------------------------------------------------------------------------

@lru_cache(maxsize=1)
def ext_ref(M, N, K):
    """operands and int64 references of the extended-epilogue case: r in {1/2, 1, 2} (kept doubled: r2), integer coef, dres_pooled in
    multiples of the 8 rows of a group; pre2 / y2 in half units"""
    from types import SimpleNamespace as NS
    x, w, b = ints((M, K), density=0.2, seed=71), ints((N, K), density=0.2, seed=72), ints((N,), -3, 3, 1.0, 73)
    e = ints((M,), -1, 1, None, 74)
    r2 = torch.where(e > 0, 4, torch.where(e < 0, 1, 2))
    res = ints((M, N), -4, 4, 0.7, 75)
    pre2 = r2[:, None] * mm(x, w.t()) + 2 * b
    dy, coef = ints((M, N), density=0.2, seed=76), ints((M,), -2, 2, None, 77)
    dres, dpool = ints((M, K), -4, 4, 0.7, 78), 8 * ints((M // 8, K), -3, 3, 0.7, 79)
    base = mm(dy, w) - coef[:, None] * x
    dx = {(wr, wp): base + (dres if wr else 0) + (dpool.repeat_interleave(8, dim=0) // 8 if wp else 0) for wr in (0, 1) for wp in (0, 1)}
    return NS(x=x, w=w, b=b, r2=r2, res=res, pre2=pre2, y2res=pre2 + 2 * res, dy=dy, coef=coef, dres=dres, dpool=dpool, dx=dx)


@pytest.mark.parametrize("kind", EXT)
def test_extended_epilogue(L, dev, kind):
    """y = r (x) (x W^T) + b (+ residual) and dx = dy W - c (x) x + dres + dres_pooled / 8 with r in {1/2, 1, 2}, integer c and
    dres_pooled in multiples of 8: every term exact.  Square weights, so the forward and dX take the same route."""
    M, N, K = ext_shape(L.lib.meant_num_cus(), kind)
    routes = {"nt256s": dict(nt256s=1), "nt_overlap": dict(nt256s=1, nt_overlap=1), "nt128": dict(nt128=1)}[kind]
    o = ext_ref(M, N, K)
    xd, _ = to_dev(o.x, BF, dev, ld=K + 8)
    wd, _ = to_dev(o.w, BF, dev)
    bd, rd = o.b.float().to(dev), (o.r2.double() / 2).float().to(dev)
    rv, _ = to_dev(o.res, BF, dev, ld=N + 16)
    with case(L, f"rowscale {kind} ({M},{N},{K})") as c:
        for with_res in (False, True):
            yv, ybuf = to_dev(None, BF, dev, ld=N + 8, sentinel=True, rows=M, cols=N)
            pv, pbuf = to_dev(None, BF, dev, ld=N + 8, sentinel=True, rows=M, cols=N)
            L.check(L.lib.meant_linear_fwd_rowscale(xd.data_ptr(), K + 8, wd.data_ptr(), bd.data_ptr(), rd.data_ptr(), rv.data_ptr() if with_res else None,
                                                    N + 16, yv.data_ptr(), N + 8, None if with_res else pv.data_ptr(), M, N, K,
                                                    L.EPI_RESIDUAL if with_res else L.EPI_GELU, 1, _stream()), "linear_fwd_rowscale")
            c.routes(**routes)
            assert_guard(ybuf, M, N, "rowscale y")
            if with_res:
                assert_exact(yv, o.y2res, "rowscale + residual", denom=2)
            else:
                assert_exact(pv, o.pre2, "rowscale preact", denom=2)
                assert_guard(pbuf, M, N, "rowscale preact")
                pre = o.pre2.double() / 2
                ref = _gelu64(pre)
                err = (yv.cpu().double() - ref).abs()
                assert bool((err <= 2.0 ** -8 * ref.abs() + 1e-6 * pre.abs().clamp(min=1.0)).all()), "rowscale gelu"
    # input gradient: dy [M, N] wT [K, N] -> dx [M, K]
    dyd, _ = to_dev(o.dy, BF, dev, ld=N + 8)
    wTd, _ = to_dev(o.w.t().contiguous(), BF, dev)
    dresd, _ = to_dev(o.dres, BF, dev, ld=K + 16)
    coefd, dpoold = o.coef.float().to(dev), o.dpool.float().to(dev).contiguous()
    with case(L, f"dx_norm {kind} ({M},{N},{K})") as c:
        for with_res, with_pool in ((1, 0), (0, 1), (1, 1), (0, 0)):
            dxv, dxbuf = to_dev(None, BF, dev, ld=K + 8, sentinel=True, rows=M, cols=K)
            L.check(L.lib.meant_linear_bwd_dx_norm(dyd.data_ptr(), N + 8, wTd.data_ptr(), xd.data_ptr(), K + 8, coefd.data_ptr(),
                                                   dresd.data_ptr() if with_res else None, K + 16 if with_res else 0,
                                                   dpoold.data_ptr() if with_pool else None, 8, dxv.data_ptr(), K + 8, M, N, K, 1, _stream()), "bwd_dx_norm")
            c.routes(**routes)
            assert_guard(dxbuf, M, K, "dx_norm")
            assert_exact(dxv, o.dx[with_res, with_pool], f"dx_norm res={with_res} pool={with_pool}")


# ---- h: the fp32 engine ------------------------------------------------------------------------------------------------------------------

def _place(t, dev, fast_last, pad, bstride0=False):
    """logical [nb1, nb2, R, C] int64 -> float device storage with NaN padding; returns (tensor kept alive, ptr, strides b1, b2, r, c).
    fast_last: the last logical axis is the contiguous one; otherwise the row axis is.  bstride0: one matrix, both batch strides 0."""
    nb1, nb2, R, Cc = t.shape
    if bstride0:
        assert bool((t == t[:1, :1]).all())
        nb1 = nb2 = 1
        t = t[:1, :1]
    if fast_last:
        buf = torch.full((nb1, nb2, R, Cc + pad), float("nan"), device=dev)
        buf[..., :Cc] = t.float().to(dev)
        s = (buf.stride(0), buf.stride(1), buf.stride(2), 1)
    else:
        buf = torch.full((nb1, nb2, Cc, R + pad), float("nan"), device=dev)
        buf[..., :R] = t.float().transpose(2, 3).to(dev)
        s = (buf.stride(0), buf.stride(1), 1, buf.stride(2))
    if bstride0:
        s = (0, 0) + s[2:]
    return buf, buf.data_ptr(), s


def run_f32(L, dev, M, N, K, *, nb=(1, 1), a_kfast=True, b_nfast=True, c_t=False, alpha2=2, accumulate=0, bcast=False, seed=81, dens=0.5):
    """C = alpha A B (+ C); alpha2 = 2 alpha, so that alpha = 1/2 stays in integers of half units"""
    import ctypes
    nb1, nb2 = nb
    A = _ints((nb1, nb2, M, K), density=dens, seed=seed)
    B = _ints((1, 1, K, N), density=dens, seed=seed + 1).expand(nb1, nb2, K, N) if bcast else _ints((nb1, nb2, K, N), density=dens, seed=seed + 1)
    C0 = _ints((nb1, nb2, M, N), -5, 5, 1.0, seed + 2)
    want2 = alpha2 * mm(A.reshape(-1, M, K), B.reshape(-1, K, N)).view(nb1, nb2, M, N) + (2 * C0 if accumulate else 0)
    ka, pa, sa = _place(A, dev, a_kfast, 3)
    kb, pb, sb = _place(B, dev, b_nfast, 5, bstride0=bcast)
    rows, cols = (N, M) if c_t else (M, N)
    cv, cbuf = to_dev(None, F32, dev, ld=cols + 7, sentinel=True, rows=nb1 * nb2 * rows, cols=cols)
    ld = cols + 7
    c4 = cbuf[:nb1 * nb2 * rows].view(nb1, nb2, rows, ld)[..., :cols]        # the batches stacked along the rows of one guarded buffer
    c4.copy_((C0.transpose(2, 3) if c_t else C0).float())
    sc = (nb2 * rows * ld, rows * ld, 1, ld) if c_t else (nb2 * rows * ld, rows * ld, ld, 1)
    arr = lambda s: (ctypes.c_int64 * 4)(*s)
    sA, sB, sC = arr(sa), arr(sb), arr(sc)
    L.check(L.lib.meant_gemm_f32_strided(pa, pb, cbuf.data_ptr(), M, N, K, nb1, nb2, ctypes.addressof(sA), ctypes.addressof(sB), ctypes.addressof(sC),
                                         alpha2 / 2.0, accumulate, _stream()), "gemm_f32_strided")
    torch.cuda.synchronize()
    tag = f"f32 ({M},{N},{K}) nb={nb} a_kfast={a_kfast} b_nfast={b_nfast} c_t={c_t} alpha={alpha2 / 2} acc={accumulate} bcast={bcast}"
    assert_guard(cbuf, nb1 * nb2 * rows, cols, tag)
    got = c4.transpose(2, 3) if c_t else c4
    assert_exact(got, want2, tag, denom=2)


@pytest.mark.parametrize("a_kfast", [True, False])
@pytest.mark.parametrize("b_nfast", [True, False])
def test_f32_engine_shapes(L, dev, a_kfast, b_nfast):
    """both BK forms (K < 256 / >= 256) and the partial last k-tile, edge tiles, for each contiguity of A and B"""
    with case(L, f"gemm_f32 K sweep a_kfast={a_kfast} b_nfast={b_nfast}") as c:
        for K in (1, 15, 16, 17, 255, 256, 300):
            for M, N in ((1, 63), (63, 65), (65, 1) if K < 256 else (65, 2)):
                run_f32(L, dev, M, N, K, a_kfast=a_kfast, b_nfast=b_nfast, alpha2=2, seed=81 + K)
                c.routes(gemm_f32=1)


@pytest.mark.parametrize("alpha2,accumulate", [(1, 0), (-4, 1), (1, 1), (-4, 0)])
def test_f32_engine_batches_alpha_and_transposed_output(L, dev, alpha2, accumulate):
    """alpha = 1/2 and -2, with and without accumulate; nb1 x nb2 batches, a broadcast B, a transposed C"""
    with case(L, f"gemm_f32 batches alpha={alpha2 / 2} accumulate={accumulate}") as c:
        for nb, bcast, c_t, a_kfast in (((2, 3), False, False, True), ((3, 2), True, False, False), ((1, 2), False, True, True), ((2, 1), True, True, False)):
            run_f32(L, dev, 65, 63, 17, nb=nb, bcast=bcast, c_t=c_t, a_kfast=a_kfast, alpha2=alpha2, accumulate=accumulate)
            c.routes(gemm_f32=1)
            run_f32(L, dev, 63, 65, 300, nb=nb, bcast=bcast, c_t=c_t, a_kfast=a_kfast, alpha2=alpha2, accumulate=accumulate)
            c.routes(gemm_f32=1)


@pytest.mark.parametrize("a_kfast", [True, False])
def test_f32_engine_gemv(L, dev, a_kfast):
    with case(L, f"gemm_f32 gemv a_kfast={a_kfast}") as c:
        for M, K, accumulate in ((1, 256, 0), (65, 300, 1), (1000, 1027, 0)):
            run_f32(L, dev, M, 1, K, a_kfast=a_kfast, alpha2=1, accumulate=accumulate, seed=91)
            c.routes(gemm_f32=1)


@pytest.mark.parametrize("det", [0, 1], ids=["atomics", "det"])
@pytest.mark.parametrize("K", [1024, 2048])
def test_f32_engine_split_k(L, dev, K, det):
    """few tiles and a long K: two or four workgroups per tile add with float atomics into a C that is a slice of a guarded buffer
    (zeroed by a 2-D memset without accumulate); ordered under the deterministic option"""
    with case(L, f"gemm_f32 split-K (130,70,{K})", deterministic=det) as c:
        for accumulate in (0, 1):
            run_f32(L, dev, 130, 70, K, alpha2=-4, accumulate=accumulate, a_kfast=False, seed=95)
            c.routes(gemm_f32=1)


def test_f32_engine_on_bf16_storage_and_f32_linear(L, dev):
    """what the MFMA kernels refuse: K = 12 forward, N = 12 dX, lddy % 8 != 0 dW (bf16 storage); and the f32 tier's Linear with bias,
    residual and the pre-activation copy"""
    with case(L, "gemm_f32 on bf16 storage / f32 linear") as c:
        run_fwd(L, dev, 65, 63, 12, ldx=12, res="same_ld", ldy=70)
        c.routes(gemm_f32=1)
        run_dx(L, dev, 65, 12, 63, lddy=12, lddx=70)
        c.routes(gemm_f32=1)
        run_dw(L, dev, 100, 72, 136, lddy=75)
        c.routes(gemm_f32=1)
        run_fwd(L, dev, 65, 63, 300, dtype=F32, res="same_ld", ldx=303, ldy=70, preact=True)
        c.routes(gemm_f32=1)
        run_fwd(L, dev, 65, 63, 17, dtype=F32, act="gelu", ldx=20, ldy=70, preact=True, dens=0.3)
        c.routes(gemm_f32=1)
        run_dx(L, dev, 65, 300, 63, dtype=F32, lddy=301, lddx=64)
        c.routes(gemm_f32=1)
        run_dw(L, dev, 100, 63, 65, dtype=F32, lddy=64, ldx=67)
        c.routes(gemm_f32=1)


# ---- i: smaller kernels that share the method ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,K", [(1, 8), (63, 136), (130, 768)])
def test_colscale_and_its_gradient(L, dev, N, K):
    """W' = W diag(g);  dW += dW' diag(g), dg[k] += sum_n dW'[n, k] W[n, k]"""
    w, g, dwp = _ints((N, K), -3, 3, 0.8, 101), _ints((1, K), -3, 3, 1.0, 102), _ints((N, K), -3, 3, 0.8, 103)
    dw0, dg0 = _ints((N, K), -5, 5, 1.0, 104), _ints((1, K), -5, 5, 1.0, 105)
    wd, gd, dwpd = w.float().to(dev), g.float().to(dev), dwp.float().to(dev)
    with case(L, f"colscale ({N},{K})") as c:
        ov, obuf = to_dev(None, F32, dev, sentinel=True, rows=N, cols=K)
        L.check(L.lib.meant_colscale(wd.data_ptr(), gd.data_ptr(), ov.data_ptr(), N, K, _stream()), "colscale")
        dwv, dwbuf = to_dev(dw0, F32, dev, sentinel=True)
        dgv, dgbuf = to_dev(dg0, F32, dev, ld=K + 8, sentinel=True, tail_rows=0)
        L.check(L.lib.meant_colscale_bwd(dwpd.data_ptr(), wd.data_ptr(), gd.data_ptr(), dwv.data_ptr(), dgv.data_ptr(), N, K, _stream()), "colscale_bwd")
        c.routes()
        assert_guard(obuf, N, K, "colscale")
        assert_exact(ov, w * g, "colscale")
        assert_guard(dwbuf, N, K, "colscale_bwd dw")
        assert_guard(dgbuf, 1, K, "colscale_bwd dg")
        assert_exact(dwv, dw0 + dwp * g, "colscale_bwd dw")
        assert_exact(dgv, dg0 + (dwp * w).sum(0, keepdim=True), "colscale_bwd dg")


@pytest.mark.parametrize("rows,cols", [(1, 1), (63, 65), (130, 768), (768, 100)])
def test_transpose_into_bf16(L, dev, rows, cols):
    """the wT operand of dX: float [rows, cols] -> bf16 [cols, rows]"""
    src = _ints((rows, cols), -256, 256, None, 111)
    sd = src.float().to(dev)
    with case(L, f"transpose2d ({rows},{cols})") as c:
        ov, obuf = to_dev(None, BF, dev, sentinel=True, rows=cols, cols=rows)
        L.check(L.lib.meant_transpose2d(sd.data_ptr(), 0, ov.data_ptr(), 1, rows, cols, _stream()), "transpose2d")
        c.routes()
        assert_guard(obuf, cols, rows, "transpose2d")
        assert_exact(ov, src.t().contiguous(), "transpose2d")
