"""Worst error per route, regime and tier of tests/test_gpu_norm_regimes.py, from the lines the tests print:
    pytest tests/test_gpu_norm_regimes.py -q -s > LOG; python tools/norm_regimes_errors.py LOG
(profiles/norm_regimes_errors.txt).  A route is a kernel family and an entry, the worst taken over its widths.  Columns as
norm_ref.check takes them: fwd = y / the pooled features (row-normalised / per tensor), xm the pooled input, stat = rinv, rstd
(relative) and the LayerNorm mean (in units of the row's deviation), dx row-normalised, the parameter gradients per tensor."""
import collections
import re
import sys

COLS = collections.OrderedDict([("fwd", ("y", "hm")), ("xm", ("xm",)), ("stat", ("rinv", "rstd", "mean")), ("dx", ("dx",)),
                                ("dgain", ("dgain", "dgamma")), ("dbias", ("db", "dbeta", "doffset")), ("dW", ("dW",)), ("dgain3", ("dgain3",))])
BOUND = {"f32": {"fwd": 1e-3, "xm": 1e-3, "stat": 1e-3, "grad": 2e-3}, "bf16": {"fwd": 4e-2, "xm": 4e-2, "stat": 1e-3, "grad": 6e-2}}


def main(path):
    worst, cases = {}, 0
    for line in open(path):
        at = line.find("norm-regime-errors")
        if at < 0:
            continue
        cases += 1
        kv = dict(p.split("=", 1) for p in line[at:].split()[1:])
        route = re.sub(r"_d\d+(_p\d+)?$", "", kv.pop("route"))
        w = worst.setdefault((route, kv.pop("regime"), kv.pop("tier")), {})
        for col, names in COLS.items():
            for n in names:
                if n in kv:
                    w[col] = max(w.get(col, 0.0), float(kv[n]))
    print(f"{cases} cases")
    print(f"{'route':<22}{'regime':<11}{'tier':<6}" + "".join(f"{c:>9}" for c in COLS))
    for (route, regime, tier), w in sorted(worst.items()):
        print(f"{route:<22}{regime:<11}{tier:<6}" + "".join(f"{w[c]:>9.1e}" if c in w else f"{'-':>9}" for c in COLS))
    for tier in ("f32", "bf16"):
        print(f"\nworst per figure, {tier} tier (share of its bound):")
        for c in COLS:
            best = max(((w[c], r, g) for (r, g, t), w in worst.items() if t == tier and c in w), default=None)
            if best:
                b = BOUND[tier].get(c, BOUND[tier]["grad"])
                print(f"  {c:<8}{best[0]:.1e}  {best[1]} / {best[2]}  ({best[0] / b:.2f} of {b:.0e})")


if __name__ == "__main__":
    main(sys.argv[1])
