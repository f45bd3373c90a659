"""The record tests/test_gpu_composite_limits.py holds the engine's gradient to: composite_limits_ratios.json, made from the
output of

    python -m pytest -s -m gpu tests/test_gpu_composite_limits.py > log

on one MI355X (its ``RATIO <case> <route> <block> <err_p / max(e64_p, floor_p), worst p of the block>`` lines; every comparison
prints one, failing or not): one ratio per case, route and parameter block.  Run it again, and review the diff of the record,
whenever a change to the engine is MEANT to move its accuracy on these cases.  A block whose ratio exceeds the largest gradient
ratio of conditioning_ratios.json (10.4, on ill-conditioned tables) on these well-conditioned problems is not to be recorded
as it stands: this script refuses to, naming the block.

Usage:  python tests/golden/make_composite_limits_ratios.py log
"""
import json
import sys
from pathlib import Path

OUT = Path(__file__).resolve().parent / "composite_limits_ratios.json"
THRESHOLD = 10.4


def main(log):
    ratio = {}
    for line in Path(log).read_text().splitlines():
        at = line.find("RATIO ")
        f = line[at:].split() if at >= 0 else []  # (pytest's progress letters may precede a test's first line)
        if len(f) == 5 and f[0] == "RATIO":
            d = ratio.setdefault(f[1], {}).setdefault(f[2], {})
            d[f[3]] = max(d.get(f[3], 0.0), float(f[4]))
    over = [(c, r, b, v) for c, routes in ratio.items() for r, blocks in routes.items() for b, v in blocks.items() if not v <= THRESHOLD]
    if over:
        sys.exit("not recorded: " + "; ".join(f"{c} {r} {b} = {v:.3g}" for c, r, b, v in over) + f" exceed {THRESHOLD}")
    OUT.write_text(json.dumps({"ratio": ratio}, indent=1, sort_keys=True) + "\n")
    worst = {}
    for routes in ratio.values():
        for blocks in routes.values():
            for b, v in blocks.items():
                b = b.split(".")[-1].rstrip("0123456789")
                worst[b] = max(worst.get(b, 0.0), v)
    print(f"wrote {OUT}: {sum(len(b) for r in ratio.values() for b in r.values())} ratios; largest per block: "
          + ", ".join(f"{b} {v:.3g}" for b, v in worst.items()))


if __name__ == "__main__":
    main(sys.argv[1])
