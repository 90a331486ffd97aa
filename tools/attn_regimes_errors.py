"""Worst error per route and regime of tests/test_gpu_attn_regimes.py, from the lines the tests print:
    pytest tests/test_gpu_attn_regimes.py -q -rP > LOG; python tools/attn_regimes_errors.py LOG
(profiles/attn_regimes_errors.txt).  Columns as attn_ref._check takes them: o against the reference's largest value, p (temporal
core) absolute, m / l the two halves of the statistics pair, dq / dk / dv element errors over the block's largest value, *_norm
the relative norm difference."""
import collections
import sys

COLS = ["o", "p", "m", "l", "dq", "dk", "dv", "dq_norm", "dk_norm", "dv_norm"]


def main(path):
    worst = {}
    for line in open(path):
        if not line.startswith("regime-errors"):
            continue
        kv = dict(p.split("=", 1) for p in line.split()[1:])
        w = worst.setdefault((kv.pop("route"), kv.pop("regime")), {})
        for k, v in kv.items():
            w[k] = max(w.get(k, 0.0), float(v))
    print(f"{'route':<20}{'regime':<9}" + "".join(f"{c:>10}" for c in COLS))
    for (route, regime), w in sorted(worst.items()):
        print(f"{route:<20}{regime:<9}" + "".join(f"{w[c]:>10.1e}" if c in w else f"{'-':>10}" for c in COLS))
    tiers = collections.OrderedDict()
    for (route, regime), w in sorted(worst.items()):
        t = tiers.setdefault("f32" if "f32" in route else "bf16", {})
        for k, v in w.items():
            if v > t.get(k, (0.0,))[0]:
                t[k] = (v, route, regime)
    for tier, t in tiers.items():
        print(f"\nworst per figure, {tier} tier:")
        for c in COLS:
            if c in t:
                print(f"  {c:<8}{t[c][0]:.1e}  {t[c][1]} / {t[c][2]}")


if __name__ == "__main__":
    main(sys.argv[1])
