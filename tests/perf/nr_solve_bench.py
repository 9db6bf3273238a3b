"""NewtonRaphson's whole ``compute_averaged_states`` (newton_raphson.py:151-216) with the Newton
system solved on the host (``solve="host"``: the default, the reference's ``np.linalg.solve``) and
on the device (``solve="device"``: ``fedagg_dense_solve_f64``), host inputs in both cases: K
clients' P x P float64 Hessians (standard normal, so the factorisation interchanges rows at
nearly every step) + P float32 gradients.  The two legs alternate in one process; every figure is
a range over the alternations.  The device leg is split by the session's events into the sums
(staging included), the factorisation, the substitution, and the fetch of x.  One JSON line per
(K, P), appended to ``--out`` when given.

    python3 tests/perf/nr_solve_bench.py --configs 8x2048,8x4096,16x4096,4x8192 --out profiles/nr_solve_bench.jsonl
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


class _Algo:
    pass


def _rng(vals, nd=4):
    return [round(min(vals), nd), round(max(vals), nd)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="8x2048,8x4096,16x4096,4x8192")
    ap.add_argument("--reps", type=int, default=3, help="alternations of host and device (at least 3)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    reps = max(3, args.reps)
    import standin_substrafl.strategies as ss
    from standin_substrafl.strategies.schemas import NewtonRaphsonSharedState
    from substrafl_amd.engine import engine_for
    from substrafl_amd.integration import accelerate

    legs = {m: accelerate(ss.NewtonRaphson, solve=m)(algo=_Algo(), damping_factor=1.0) for m in ("host", "device")}
    for cfg in args.configs.split(","):
        K, P = (int(v) for v in cfg.split("x"))
        rng = np.random.default_rng(K + P)
        grads = [[rng.standard_normal(P).astype(np.float32)] for _ in range(K)]
        hess = [rng.standard_normal((P, P)) for _ in range(K)]
        ns = [int(v) for v in rng.integers(1, 1000, K)]
        states = [NewtonRaphsonSharedState(gradients=g, hessian=h, n_samples=n) for g, h, n in zip(grads, hess, ns)]
        legs["device"].compute_averaged_states(shared_states=states, _skip=True)  # warm: session, ring, buffers, code
        t = {"host": [], "device": []}
        split = {k: [] for k in ("sums_ms", "factor_ms", "substitute_ms", "fetch_s")}
        out = {}
        for _ in range(reps):
            for mode in ("host", "device"):
                t0 = time.perf_counter()
                out[mode] = legs[mode].compute_averaged_states(shared_states=states, _skip=True).parameters_update
                t[mode].append(time.perf_counter() - t0)
                tm = engine_for(None).last_timing
                assert tm["solve"] == mode, tm["solve"]
                if mode == "device":
                    for k in split:
                        split[k].append(tm[k])
        xh, xd = (np.concatenate([np.asarray(a).reshape(-1) for a in out[m]]) for m in ("host", "device"))
        factor_s = min(split["factor_ms"]) / 1e3
        line = {"clients": K, "params": P, "alternations": reps,
                "host_total_s": _rng(t["host"]), "device_total_s": _rng(t["device"]),
                "speedup_min_over_min": round(min(t["host"]) / min(t["device"]), 2),
                "device_sums_ms": _rng(split["sums_ms"], 2), "device_factor_ms": _rng(split["factor_ms"], 2),
                "device_substitute_ms": _rng(split["substitute_ms"], 2), "device_fetch_s": _rng(split["fetch_s"], 5),
                "getrf_fp64_tflops": round(2.0 / 3.0 * P ** 3 / factor_s / 1e12, 3),
                "rel_diff_device_vs_host": float(np.abs(xd - xh).max() / np.abs(xh).max()),
                "device_faster": bool(max(t["device"]) < min(t["host"]))}
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
