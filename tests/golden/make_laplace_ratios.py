"""The record of the Laplace path's accuracy: laplace_ratios.json, made from the output of

    python -m pytest -s -m gpu tests/test_gpu_laplace.py > log

on one MI355X (its ``LAPLACE <problem> <quantity> <engine error> <host error> <ratio>`` lines; every comparison prints one, failing
or not).  The test's bars do not read the record -- they are 8 x the float64 host's error with the suite's floors -- it is what
DESIGN 3.18's error table is made from.  Run it again whenever a change to the engine is MEANT to move its accuracy there.

Usage:  python tests/golden/make_laplace_ratios.py log
"""
import json
import sys
from pathlib import Path

OUT = Path(__file__).resolve().parent / "laplace_ratios.json"


def main(log):
    record = {}
    for line in Path(log).read_text().splitlines():
        at = line.find("LAPLACE ")
        f = line[at:].split() if at >= 0 else []  # (pytest's progress letters may precede a test's first line)
        if len(f) != 6 or f[0] != "LAPLACE":
            continue
        record.setdefault(f[1], {})[f[2]] = {"engine": float(f[3]), "host": float(f[4]), "ratio": float(f[5])}
    OUT.write_text(json.dumps(record, indent=1, sort_keys=True) + "\n")
    print(f"wrote {OUT}: {sum(len(q) for q in record.values())} comparisons of {len(record)} problems")


if __name__ == "__main__":
    main(sys.argv[1])
