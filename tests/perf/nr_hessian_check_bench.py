"""The Hessian check at the end of a NewtonRaphson client's ``train``
(torch_newton_raphson_algo.py:346-352) by the reference's rule (``check="host"``: ``np.linalg.eig``
of the whole matrix) and with the Cholesky certificate on the device first (``check="device"``:
``fedagg_dense_potrf_f64``), on the same host array in the same process: a Gram Hessian
X^T D X / m + l2 I with m = P / 2 and l2 = 1e-3, positive definite, so the device leg never
reaches the host rule.  The device leg is split into staging (the symmetry test on the host is
timed separately: it is part of the route), the factorisation (session events) and the fetch of
``info``.  One JSON line per P, appended to ``--out`` when given.

    python3 tests/perf/nr_hessian_check_bench.py --sizes 1024,2048,4096 --out profiles/nr_hessian_check_bench.jsonl
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _rng(vals, nd=4):
    return [round(min(vals), nd), round(max(vals), nd)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,2048,4096")
    ap.add_argument("--reps", type=int, default=3, help="runs of the device leg")
    ap.add_argument("--host-reps", type=int, default=2, help="runs of the host leg (cubic in P, ~25 P^3 flops)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from test_dense_potrf_gpu import _gram

    from substrafl_amd.engine import engine_for, equals_transpose
    from substrafl_amd.integration import newton_raphson_hessian_check

    for P in (int(v) for v in args.sizes.split(",")):
        H = _gram(P, P // 2, 1e-3)
        assert newton_raphson_hessian_check(H, 1e-3, check="device") == "device"  # warm: session, buffers, code
        t = {"host": [], "device": []}
        split = {k: [] for k in ("stage_s", "factor_ms", "fetch_s", "total_s")}
        sym = []
        for r in range(max(args.reps, args.host_reps)):
            if r < args.host_reps:
                t0 = time.perf_counter()
                assert newton_raphson_hessian_check(H, 1e-3, check="host") == "host"
                t["host"].append(time.perf_counter() - t0)
            if r < args.reps:
                t0 = time.perf_counter()
                assert newton_raphson_hessian_check(H, 1e-3, check="device") == "device"
                t["device"].append(time.perf_counter() - t0)
                tm = engine_for(None).last_timing
                for k in split:
                    split[k].append(tm[k])
                t0 = time.perf_counter()
                assert equals_transpose(H)
                sym.append(time.perf_counter() - t0)
        factor_s = min(split["factor_ms"]) / 1e3
        line = {"params": P, "host_runs": len(t["host"]), "device_runs": len(t["device"]),
                "host_eig_s": _rng(t["host"]), "device_total_s": _rng(t["device"], 5),
                "speedup_min_over_min": round(min(t["host"]) / min(t["device"]), 1),
                "device_symmetry_test_s": _rng(sym, 5), "device_stage_s": _rng(split["stage_s"], 5),
                "device_factor_ms": _rng(split["factor_ms"], 3), "device_fetch_s": _rng(split["fetch_s"], 6),
                "potrf_fp64_tflops": round(P ** 3 / 3.0 / factor_s / 1e12, 3),
                "device_faster": bool(max(t["device"]) < min(t["host"]))}
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
