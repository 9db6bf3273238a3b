"""Wall time of one Scaffold aggregation on the multi-device routes (host inputs, PCIe-inclusive;
report only): K clients x M parameters in three layers, one of them (1,)-shaped, every client
holding the same ``c`` list.

* fp32 through the one-call C entry (``NativeMultiScaffold``: two ``fedagg_multi_scaffold_bucket``
  calls) beside ``MultiDeviceEngine.scaffold`` on the same arrays;
* bf16 (the fp32 values' upper halves) through ``MultiDeviceEngine.scaffold_per_bucket`` beside the
  one-device ``AggregationEngine.scaffold_per_bucket``.

Best of ``--reps`` after one warm-up call; one JSON line.

    python3 tests/perf/multi_scaffold_bench.py --clients 16 --params 25000000 --devices 0,0
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def best(fn, reps: int) -> float:
    fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t)
    return round(min(out), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=16)
    ap.add_argument("--params", type=int, default=25_000_000)
    ap.add_argument("--devices", default="0,0")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from substrafl_amd import wire
    from substrafl_amd.engine import AggregationEngine
    from substrafl_amd.multi_device import MultiDeviceEngine, NativeMultiScaffold

    K, M = args.clients, args.params
    devices = [int(d) for d in args.devices.split(",")]
    shapes = [(M - M // 25 - 1,), (1,), (M // 25,)]
    rng = np.random.default_rng(0)
    mk = lambda: [rng.random(s, dtype=np.float32) - 0.5 for s in shapes]  # noqa: E731
    half = lambda row: [np.ascontiguousarray((a.view(np.uint32) >> 16).astype(np.uint16)).view(wire.BF16)  # noqa: E731
                        for a in row]
    pu, cv, c = [mk() for _ in range(K)], [mk() for _ in range(K)], mk()
    pu16, cv16, c16 = [half(r) for r in pu], [half(r) for r in cv], half(c)
    ns = [int(v) for v in rng.integers(1, 5000, K)]
    line = {"clients": K, "params": M, "devices": devices, "reps": args.reps}
    nat = NativeMultiScaffold(devices)
    line["fp32_native_multi_s"] = best(lambda: nat.scaffold(pu, cv, [c] * K, ns, 0.7), args.reps)
    nat.close()
    md = MultiDeviceEngine(devices)
    line["fp32_multi_device_scaffold_s"] = best(lambda: md.scaffold(pu, cv, [c] * K, ns, 0.7), args.reps)
    line["bf16_multi_device_per_bucket_s"] = best(lambda: md.scaffold_per_bucket(pu16, cv16, [c16] * K, ns, 0.7),
                                                  args.reps)
    line["bf16_sub_ranges_per_shard"] = [len(r) for r in md.last_timing["ranges"]]
    one = AggregationEngine(device=devices[0])
    line["bf16_one_device_per_bucket_s"] = best(lambda: one.scaffold_per_bucket(pu16, cv16, [c16] * K, ns, 0.7),
                                                args.reps)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
