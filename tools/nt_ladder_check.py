"""The launch ladder gemm_bf16_nt_launch had before it was given a classifier (commit 76749fe), transcribed by hand -- the route counters in
hit order, the head / tail recursion, and the old gemm_bf16_nt_streams formula -- against meant_debug_gemm_route of the built library on
random shapes, strides, residual / rotary / aliasing facts, options nt_stream / nt_ragged and compute-unit counts.  CPU only.

    python tools/nt_ladder_check.py [CASES]      (default 200000; prints the first differences and their count)"""
import ctypes
import os
import random
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from meant_amd import _lib as L

B2, BK = 256, 64
cd = lambda a, b: -(-a // b)


def old(M, N, K, ldc8, ldr8, res, rot_S, alias, stream, ragged, ncus, out):
    ktail = K % BK != 0
    rot = rot_S > 0
    if rot:
        out.append("nt_rot")
    if M >= 1024 and N % 256 == 0 and cd(M, B2) * (N // B2) * 2 >= ncus:
        stream_ok = stream != 0 and not ktail
        elig = K >= 4 * BK and ldc8 and (not res or ldr8)
        ragged_overlap = stream_ok and ragged != 0 and M % B2 != 0 and elig and not alias
        m_full = (M // B2) * B2
        if not ragged_overlap and stream_ok and m_full >= 1024 and m_full != M and elig and (not rot or m_full % rot_S == 0):
            out.append("nt_split")
            old(m_full, N, K, ldc8, ldr8, res, rot_S, alias, stream, ragged, ncus, out)
            old(M - m_full, N, K, ldc8, ldr8, res, rot_S, alias, stream, ragged, ncus, out)
            return
        if stream_ok and (M % B2 == 0 or ragged_overlap) and elig:
            if ragged_overlap:
                out.append("nt_overlap")
            out.append("nt256s_rot" if rot else "nt256s")
        elif ktail:
            out.append("nt256k")
        else:
            out.append("nt256")
        return
    out.append("nt128k" if ktail else "nt128")


def old_streams(M, N, K, ldc8, ldr8, res, stream, ncus):
    return (M >= 1024 and M % B2 == 0 and N % 256 == 0 and cd(M, B2) * (N // B2) * 2 >= ncus and stream != 0 and K % BK == 0 and K >= 4 * BK
            and ldc8 and (not res or ldr8))


rnd = random.Random(1)
buf = ctypes.create_string_buffer(256)
bad = 0
n = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
for i in range(n):
    M = rnd.choice([1, 100, 1023, 1024, 1025, 1279, 1280, 2048, 2048 + 37, 4096, 16384, 16384 + 100, 16384 + 255, 75296, rnd.randint(1, 40000)])
    N = rnd.choice([8, 72, 256, 264, 512, 768, 1024, 1536, rnd.randint(1, 300) * 8])
    K = rnd.choice([8, 64, 72, 128, 192, 200, 248, 256, 264, 320, 768, rnd.randint(1, 200) * 8])
    ldc8, ldr8, res, alias = rnd.random() < .8, rnd.random() < .8, rnd.random() < .5, rnd.random() < .2
    rot_S = rnd.choice([0, 0, 24, 196, 256, 512, 1024, rnd.randint(1, 3000)])
    stream, ragged = rnd.choice([1, 1, 0]), rnd.choice([1, 1, 0])
    ncus = rnd.choice([0, 8, 64, 256, 304])
    L.set_option("nt_stream", stream); L.set_option("nt_ragged", ragged)
    want = []
    old(M, N, K, ldc8, ldr8, res, rot_S, alias, stream, ragged, ncus, want)
    facts = (0 if ldc8 else L.FACT_LDC_OFF8) | (0 if ldr8 else L.FACT_LDR_OFF8) | (L.FACT_RESIDUAL if res else 0) | (L.FACT_ALIAS_C if alias else 0)
    rc = L.lib.meant_debug_gemm_route(b"nt", M, N, K, facts, rot_S, ncus, buf, len(buf))
    got = buf.value.decode().split()
    if rc < 0 or got != want or bool(rc) != bool(old_streams(M, N, K, ldc8, ldr8, res, stream, ncus)):
        bad += 1
        if bad < 10:
            print("DIFF", (M, N, K, ldc8, ldr8, res, rot_S, alias, stream, ragged, ncus), got, want, rc)
print("cases", n, "differences", bad)
