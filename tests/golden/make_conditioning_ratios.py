"""The record tests/test_gpu_conditioning.py holds the engine to: conditioning_ratios.json, made from the output of

    python -m pytest -s -m gpu tests/test_gpu_conditioning.py > log

on one MI355X (its ``RATIO <case> <path> <quantity> <err / e64>`` and ``BACKWARD <case> <path> <err / host>`` lines; every
comparison prints one, failing or not).  Run it again, and review the diff of the record, whenever a change to the engine is
MEANT to move its accuracy on these cases.

Usage:  python tests/golden/make_conditioning_ratios.py log
"""
import json
import sys
from pathlib import Path

OUT = Path(__file__).resolve().parent / "conditioning_ratios.json"


def main(log):
    ratio, backward = {}, {}
    for line in Path(log).read_text().splitlines():
        at = min((i for i in (line.find("RATIO "), line.find("BACKWARD ")) if i >= 0), default=-1)
        f = line[at:].split() if at >= 0 else []  # (pytest's progress letters may precede a test's first line)
        if len(f) == 5 and f[0] == "RATIO":
            d = ratio.setdefault(f[1], {}).setdefault(f[2], {})
            d[f[3]] = max(d.get(f[3], 0.0), float(f[4]))
        elif len(f) == 4 and f[0] == "BACKWARD":
            backward.setdefault(f[1], {})[f[2]] = max(backward.get(f[1], {}).get(f[2], 0.0), float(f[3]))
    OUT.write_text(json.dumps({"ratio": ratio, "backward": backward}, indent=1, sort_keys=True) + "\n")
    print(f"wrote {OUT}: {sum(len(p) for c in ratio.values() for p in c.values())} ratios, "
          f"{sum(len(c) for c in backward.values())} backward errors")


if __name__ == "__main__":
    main(sys.argv[1])
