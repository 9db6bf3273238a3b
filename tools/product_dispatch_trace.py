#!/usr/bin/env python3
"""Distil a rocprofv3 kernel trace of tests/test_product_dispatch_gpu.py to the launches of the
product library's kernels: one line per kernel of profiles/product_kernels.txt that was launched,
`<normalised name>\\t<calls>`, sorted by name (torch's own kernels are dropped).  Reads every
`*kernel_stats.csv` (Name, Calls) under the output directory, or, where there is none, counts the
rows of `*kernel_trace.csv` (Kernel_Name).
Usage: tools/product_dispatch_trace.py TRACE_DIR > profiles/product_dispatch_trace.txt"""

import csv
import sys
from collections import Counter
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from product_kernels import ROOT, normalise  # noqa: E402


def launches(trace_dir: Path) -> Counter:
    calls = Counter()
    stats = sorted(trace_dir.rglob("*kernel_stats.csv"))
    if stats:
        for p in stats:
            for r in csv.DictReader(open(p, newline="")):
                calls[normalise(r["Name"])] += int(r["Calls"])
        return calls
    for p in sorted(trace_dir.rglob("*kernel_trace.csv")):
        for r in csv.DictReader(open(p, newline="")):
            calls[normalise(r["Kernel_Name"])] += 1
    return calls


def main():
    calls = launches(Path(sys.argv[1]))
    if not calls:
        sys.exit(f"{sys.argv[1]}: no *kernel_stats.csv or *kernel_trace.csv with rows")
    product = {ln.strip() for ln in (ROOT / "profiles" / "product_kernels.txt").read_text().splitlines() if ln.strip()}
    for name in sorted(product & set(calls)):
        print(f"{name}\t{calls[name]}")


if __name__ == "__main__":
    main()
