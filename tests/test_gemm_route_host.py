"""Which kernel a bf16 GEMM shape takes, checked on the CPU: meant_debug_gemm_route names the route counters a launch would hit, from
the launchers' own classifiers (nt_plan / tn_plan of meant_amd/csrc/gemm_bf16.hip) without launching anything.  Every expected table
here is the one tests/test_gpu_gemm_exact.py asserts with c.routes(...) for the same row of the same table, at the 256 compute units
of an MI355X (as tests/test_gemm_exact_host.py takes them); none comes from the library.  For every forward / dX case the entry's
return value -- "the streaming kernel over whole 256-row panels", what meant_qkv_proj_fwd_live asks before it hands a panel list over
and what the by-id forward needs of both its products -- must hold exactly where the table is the streaming kernel and nothing else."""
import ctypes
from collections import Counter

import pytest

from tests import test_gpu_gemm_exact as G

CUS = 256
T512 = G.tall_m(CUS, 512)
SPLIT = dict(nt256s=1, nt_split=1, nt128=1)
OVERLAP = dict(nt256s=1, nt_overlap=1)


@pytest.fixture()
def L():
    from meant_amd import _lib
    saved = {k: _lib.get_option(k) for k in G.OPTS}
    for k, v in G.OPTS.items():
        _lib.set_option(k, v)
    yield _lib
    for k, v in saved.items():
        _lib.set_option(k, v)


def nt(what, M, N, K, want, opts=None, ldc=None, facts=(), rot_S=0):
    """one "nt" launch: C [M, N] over a reduction of K; ldc as the GPU case passes it (None: a multiple of 8)"""
    facts = tuple(facts) + (("ldc_off8",) if ldc is not None and ldc % 8 else ())
    return pytest.param(M, N, K, dict(opts or {}), facts, rot_S, want, id=what)


def _fwd(what, M, N, K, want, opts=None):
    """fwd_variants / run_fwd: without a residual and with one of its own row stride (N + 16, a multiple of 8 wherever N is)"""
    assert N % 8 == 0
    return [nt(what, M, N, K, want, opts), nt(what + " +res", M, N, K, want, opts, facts=("residual",))]


def _nt_cases():
    c = []
    for M, N, K in G.FWD_NT128:
        c += _fwd(f"fwd nt128 ({M},{N},{K})", M, N, K, dict(nt128=1))
    for M, N, K in G.FWD_NT128K:
        c += _fwd(f"fwd nt128k ({M},{N},{K})", M, N, K, dict(nt128k=1))
    for K, stream in G.FWD_NT256:
        c += _fwd(f"fwd nt256 K={K} nt_stream={stream}", T512, 512, K, dict(nt256=1), {"nt_stream": stream})
    for K in G.FWD_NT256K:
        c += _fwd(f"fwd nt256k K={K}", T512, 512, K, dict(nt256k=1))
    for K, dynamic in G.FWD_NT256S:
        c += _fwd(f"fwd nt256s K={K} nt_dynamic={dynamic}", T512, 512, K, dict(nt256s=1), {"nt_dynamic": dynamic})
    M, N, K = G.few_workgroups_shape(CUS)
    for dynamic in (1, 3):
        c += _fwd(f"fwd nt256s 64 workgroups nt_dynamic={dynamic}", M, N, K, dict(nt256s=1), {"nt_dynamic": dynamic, "nt_grid_cap": 64})
    for extra in G.RAGGED:
        for ragged, want in ((1, OVERLAP), (0, SPLIT)):
            c += _fwd(f"fwd ragged +{extra} nt_ragged={ragged}", T512 + extra, 512, 256, want, {"nt_ragged": ragged})
        c.append(nt(f"fwd ragged +{extra} residual in place", T512 + extra, 512, 256, SPLIT, facts=("residual", "alias_c")))
    for route, K, extra, opts in G.ACT:
        M, N = (129, 136) if route in ("nt128", "nt128k") else (T512 + extra, 512)
        c.append(nt(f"act {route}", M, N, K, {"nt_overlap": OVERLAP, "nt_split": SPLIT}.get(route, {route: 1}), opts))
    for M, N, K, lddx, route in G.DX_ONE:                                   # dx [M, K] = dy [M, N] wT [K, N]^T: the reduction length is N
        c.append(nt(f"dx {route} ({M},{N},{K}) lddx={lddx}", M, K, N, {route: 1}, ldc=lddx))
    for N, extra, opts, want in G.DX_TALL:
        c.append(nt(f"dx tall N={N} +{extra} {opts}", T512 + extra, 512, N, want, opts))
    for kind in G.EXT:                                                      # the forward and the input gradient take the same route
        M, N, K = G.ext_shape(CUS, kind)
        want = {"nt256s": dict(nt256s=1), "nt_overlap": OVERLAP, "nt128": dict(nt128=1)}[kind]
        c += _fwd(f"rowscale {kind}", M, N, K, want) + _fwd(f"dx_norm {kind}", M, K, N, want)
    for K, route in G.QKV_ONE:
        c.append(nt(f"qkv {route} K={K}", 3 * 24, 3 * 2 * 16, K, {route: 1, "nt_rot": 1}, rot_S=24))
    g, S, H, Dh, _ = G.qkv_stream_shape(CUS, 512)
    for K, route in G.QKV_TALL_ONE_TILE:
        c.append(nt(f"qkv {route} K={K}", g * S, 3 * H * Dh, K, {route: 1, "nt_rot": 1}, rot_S=S))
    for S, K, dynamic in G.QKV_STREAM:
        g, S, H, Dh, _ = G.qkv_stream_shape(CUS, S)
        c.append(nt(f"qkv nt256s_rot S={S} K={K} nt_dynamic={dynamic}", g * S, 3 * H * Dh, K, dict(nt256s_rot=1, nt_rot=1), {"nt_dynamic": dynamic},
                    rot_S=S))
    return c


def route(L, op, M, N, K, facts=(), rot_S=0):
    bits = sum({"ldc_off8": L.FACT_LDC_OFF8, "ldr_off8": L.FACT_LDR_OFF8, "residual": L.FACT_RESIDUAL, "alias_c": L.FACT_ALIAS_C}[f] for f in facts)
    buf = ctypes.create_string_buffer(128)
    rc = L.lib.meant_debug_gemm_route(op.encode(), M, N, K, bits, rot_S, CUS, buf, len(buf))
    assert rc >= 0, L.lib.meant_last_error().decode()
    return buf.value.decode().split(), rc


@pytest.mark.parametrize("M,N,K,opts,facts,rot_S,want", _nt_cases())
def test_forward_and_dx_tables(L, M, N, K, opts, facts, rot_S, want):
    for k, v in opts.items():
        L.set_option(k, v)
    names, streams = route(L, "nt", M, N, K, facts, rot_S)
    assert Counter(names) == Counter(want), f"({M},{N},{K}) {opts} {facts}: {names}"
    assert (streams == 1) == (sorted(names) in (["nt256s"], ["nt256s_rot", "nt_rot"])), f"({M},{N},{K}): streams={streams} with {names}"


def test_hit_order_and_an_unaligned_residual(L):
    """the order the counters move in (the launcher counts the rotary epilogue first, the split before its head and tail, the overlap
    before the kernel); and what no table row sets: on a tall shape an output stride, or the stride of a residual that is there, off a
    multiple of 8 leaves the one-tile kernel (the streaming kernel stores and reads them in 16-byte pieces)"""
    assert route(L, "nt", T512 + 100, 512, 256) == (["nt_overlap", "nt256s"], 0)
    L.set_option("nt_ragged", 0)
    assert route(L, "nt", T512 + 100, 512, 256) == (["nt_split", "nt256s", "nt128"], 0)
    g, S, H, Dh, _ = G.qkv_stream_shape(CUS, 512)
    assert route(L, "nt", g * S, 3 * H * Dh, 256, rot_S=S) == (["nt_rot", "nt256s_rot"], 1)
    assert route(L, "nt", T512, 512, 256, ("residual",)) == (["nt256s"], 1)
    assert route(L, "nt", T512, 512, 256, ("residual", "ldr_off8")) == (["nt256"], 0)
    assert route(L, "nt", T512, 512, 256, ("ldr_off8",)) == (["nt256s"], 1)          # no residual: its stride is not read
    assert route(L, "nt", T512, 512, 256, ("ldc_off8",)) == (["nt256"], 0)


def _dw_cases():
    c = [("tn", M, N, K, dict(tn128=1)) for M, N, K in G.DW_TN128]
    c += [("tn", M, N, K, dict(tn_tail=1, gemm_f32=1, **({"tn128": 1} if M >= 64 else {}))) for M, N, K in G.DW_TN_TAIL]
    c += [("tn", M, N, K, dict(tn256=1, **(dict(tn_tail=1, gemm_f32=1) if M % 64 else {}))) for M in G.DW_TN256_M for N, K in G.DW_TN256_NK]
    c += [("tn_rows", M, 256, 512, dict(tn256_rows=1)) for M in G.DW_ROWS_M]
    return c


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("op,M,N,K,want", _dw_cases())
def test_dw_tables(L, op, M, N, K, want, det):
    """deterministic = 1 turns tn256 and tn256_rows into tn256_det and nothing else; only that route has a workspace"""
    L.set_option("deterministic", det)
    if det:
        want = {{"tn256": "tn256_det", "tn256_rows": "tn256_det"}.get(r, r): n for r, n in want.items()}
    names, streams = route(L, op, M, N, K)
    assert Counter(names) == Counter(want) and streams == 0, f"{op} ({M},{N},{K}) det={det}: {names}"
    assert "tn_tail" not in want or names[:2] == ["tn_tail", "gemm_f32"]    # the tail goes first, through the exact engine
    assert (L.lib.meant_linear_bwd_dw_ws(M, N, K, L.BF16) != 0) == ("tn256_det" in want)


def test_bad_arguments_are_refused(L):
    buf = ctypes.create_string_buffer(8)
    assert L.lib.meant_debug_gemm_route(b"nn", 64, 64, 64, 0, 0, CUS, buf, len(buf)) == L.ERR_ARG
    assert L.lib.meant_debug_gemm_route(b"nt", 0, 64, 64, 0, 0, CUS, buf, len(buf)) == L.ERR_ARG
    assert L.lib.meant_debug_gemm_route(b"nt", T512, 768, 256, 0, 1 << 32, CUS, buf, len(buf)) == L.ERR_ARG            # not a sequence length of 0
    L.set_option("nt_ragged", 0)
    assert L.lib.meant_debug_gemm_route(b"nt", T512 + 100, 512, 256, 0, 0, CUS, buf, len(buf)) == L.ERR_WORKSPACE   # 21 characters
    assert L.lib.meant_debug_gemm_route(b"nt", T512, 512, 256, 0, 0, CUS, buf, len(buf)) == 1 and buf.value == b"nt256s"
