"""Worst error per entry, regime and tier of tests/test_gpu_loss_regimes.py next to its gate, from the lines the tests print:
    pytest tests/test_gpu_loss_regimes.py -q -s > LOG; python tools/loss_regimes_errors.py LOG
and the device time of the softmax cross-entropy at the pretrainer's shape (T = 1024, V = 64001, ld = 64256, bf16, forward +
backward between device events), of the library in the tree or of another build of it:
    python tools/loss_regimes_errors.py --time [--lib PATH/libmeant_hip.so]
(profiles/loss_regimes_errors.txt).  Columns as loss_ref.check takes them: row_loss, mean and lse as |err| / max(1, |ref|), dlogits
as max |err| / |gscale| (bf16 tier: less one bf16 rounding of the reference element), rowsum the |sum_j dlogits| / |gscale| of a row
that counts (f32 tier), zeros the largest magnitude where the reference is a structural zero; for meant_ce_probs loss and
dprobs * B."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COLS = ("row_loss", "mean", "lse", "dlogits", "rowsum", "zeros", "loss", "dprobs")


def collect(path):
    from tests import loss_ref as L
    worst, cases = {}, 0
    for line in open(path):
        at = line.find("loss-regime-errors")
        if at < 0:
            continue
        cases += 1
        kv = dict(p.split("=", 1) for p in line[at:].split()[1:])
        w = worst.setdefault((kv["entry"], kv["regime"], kv["tier"]), {})
        for c in COLS:
            if c in kv:
                w[c] = max(w.get(c, 0.0), float(kv[c]))
    print(f"{cases} cases")
    print(f"{'entry':<22}{'regime':<20}{'tier':<6}" + "".join(f"{c:>10}" for c in COLS))
    for (entry, regime, tier), w in sorted(worst.items()):
        print(f"{entry:<22}{regime:<20}{tier:<6}" + "".join(f"{w[c]:>10.1e}" if c in w else f"{'-':>10}" for c in COLS))
    for tier in ("f32", "bf16"):
        print(f"\nworst per figure, {tier} tier (share of its gate):")
        gates = dict(L.GATES[tier], **(L.CE_PROBS_GATES if tier == "f32" else {}))
        def gate(e, r, c):                               # ce_probs on rand + 1000: the one-float bound on top (test_ce_probs_against_float64)
            return gates[c] + (2.0 ** -15 if (e, r) == ("ce_probs", "shifted") else 0.0)
        for c in COLS:
            if c not in gates:
                continue
            best = max(((w[c] / gate(e, r, c) if gates[c] else w[c], w[c], e, r) for (e, r, t), w in worst.items() if t == tier and c in w),
                       default=None)
            if best:
                share = f"{best[0]:.2f} of {gate(best[2], best[3], c):.1e}" if gates[c] else "gate 0"
                print(f"  {c:<9}{best[1]:.1e}  {best[2]} / {best[3]}  ({share})")


def timing(lib_path, T=1024, V=64001, ld=64256, reps=50, windows=5):
    """forward + backward per call, the median and the spread of `windows` windows of `reps` calls; lse is sized [T, 2], which also
    holds the [T] of a build that keeps logsumexp in one float"""
    import torch
    assert torch.cuda.is_available()
    lib = ctypes.CDLL(lib_path)
    i64, vp = ctypes.c_int64, ctypes.c_void_p
    lib.meant_softmax_ce_fwd.argtypes = [vp, i64, vp, i64, i64, i64, vp, vp, ctypes.c_int, vp]
    lib.meant_softmax_ce_bwd.argtypes = [vp, i64, vp, vp, i64, i64, i64, vp, vp, ctypes.c_int, vp]
    lib.meant_softmax_ce_fwd.restype = lib.meant_softmax_ce_bwd.restype = ctypes.c_int
    from meant_amd import ops
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    x = (torch.randn(T, ld, generator=gen) * 3).bfloat16().to(dev)
    tg = torch.randint(0, V, (T,), generator=gen).to(dev)
    row_loss, lse = torch.empty(T, device=dev), torch.empty(T, 2, device=dev)
    g, dl = torch.ones(1, device=dev), torch.empty_like(x)
    stream, dt = ops._stream(), ops._dt(x)

    def fwd():
        assert lib.meant_softmax_ce_fwd(x.data_ptr(), ld, tg.data_ptr(), T, V, -100, row_loss.data_ptr(), lse.data_ptr(), dt, stream) == 0

    def bwd():
        assert lib.meant_softmax_ce_bwd(x.data_ptr(), ld, tg.data_ptr(), lse.data_ptr(), T, V, -100, g.data_ptr(), dl.data_ptr(), dt, stream) == 0

    def both():
        fwd()
        bwd()
    print(f"softmax_ce [{T}, {V}] ld {ld} bf16, {os.path.relpath(lib_path, ROOT)}, median (min .. max) of {windows} windows of {reps} calls")
    for name, call, nbytes in (("fwd + bwd", both, T * (4 * V + 2 * ld)), ("fwd", fwd, T * 2 * V), ("bwd", bwd, T * (2 * V + 2 * ld))):
        for _ in range(10):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / reps)
        ms.sort()
        print(f"  {name:<10}{ms[len(ms) // 2]:.4f} ms ({ms[0]:.4f} .. {ms[-1]:.4f}), {nbytes / ms[len(ms) // 2] * 1e-9:.2f} TB/s")
    print(f"  mean row loss {row_loss.mean().item():.6f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("log", nargs="?")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--lib", default=os.path.join(ROOT, "meant_amd", "libmeant_hip.so"))
    a = ap.parse_args()
    if a.time:
        timing(os.path.abspath(a.lib))
    else:
        collect(a.log)
