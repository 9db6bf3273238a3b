"""``FedPCA.avg_shared_states_with_qr`` (fed_pca.py:261-299) by both routes of the orthonormalisation,
beside each other in the same process on the same shared states: ``qr="host"`` (the reference's
``np.linalg.qr`` of the averaged matrix) and ``qr="device"`` (``fedagg_dense_gelqf_f64`` +
``fedagg_dense_orglq_f64``).  K clients of one fp32 ``(n_components, n_features)`` layer each.  The
average (the bucket kernel, either route) is timed by a plain ``avg_shared_states``; the device leg
is split into staging, the factorisation with Q (session events) and the fetch.  One JSON line per
shape, appended to ``--out`` when given.

    python3 tests/perf/fedpca_qr_bench.py --shapes 64x4096,256x8192,512x16384 --out profiles/fedpca_qr_bench.jsonl
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
    ap.add_argument("--shapes", default="64x4096,256x8192,512x16384")
    ap.add_argument("--clients", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3, help="runs of each leg")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from conftest import DummyAlgo

    from substrafl_amd.engine import engine_for
    from substrafl_amd.schemas import FedPCASharedState
    from substrafl_amd.strategies import FedPCA

    K = args.clients
    legs = {"host": FedPCA(algo=DummyAlgo(), qr="host"), "device": FedPCA(algo=DummyAlgo(), qr="device")}
    for n, m in (tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")):
        rng = np.random.default_rng([n, m])
        states = [FedPCASharedState(n_samples=int(rng.integers(1, 5000)),
                                    parameters_update=[rng.standard_normal((n, m)).astype(np.float32)]) for _ in range(K)]
        q = {k: s.avg_shared_states_with_qr(shared_states=states, _skip=True).avg_parameters_update[0]
             for k, s in legs.items()}  # warm: session, buffers, code objects
        assert engine_for(None).last_timing["qr"] == "device"
        t = {"host": [], "device": [], "average": []}
        split = {k: [] for k in ("stage_s", "factor_ms", "fetch_s", "total_s")}
        for _ in range(args.reps):
            t0 = time.perf_counter()
            legs["host"].avg_shared_states(shared_states=states, _skip=True)
            t["average"].append(time.perf_counter() - t0)
            for k, s in legs.items():
                t0 = time.perf_counter()
                s.avg_shared_states_with_qr(shared_states=states, _skip=True)
                t[k].append(time.perf_counter() - t0)
            tm = engine_for(None).last_timing
            for k in split:
                split[k].append(tm[k])
        qd, qh = np.asarray(q["device"], np.float64), np.asarray(q["host"], np.float64)
        line = {"clients": K, "n": n, "m": m, "dtype": "float32", "runs": args.reps,
                "average_alone_s": _rng(t["average"], 5),
                "host_route_total_s": _rng(t["host"], 5), "device_route_total_s": _rng(t["device"], 5),
                "host_qr_s": round(min(t["host"]) - min(t["average"]), 5),
                "device_qr_s": _rng(split["total_s"], 5), "device_stage_s": _rng(split["stage_s"], 5),
                "device_factor_ms": _rng(split["factor_ms"], 3), "device_fetch_s": _rng(split["fetch_s"], 5),
                "speedup_min_over_min": round(min(t["host"]) / min(t["device"]), 2),
                "device_faster": bool(max(t["device"]) < min(t["host"])),
                "max_abs_q_difference": float(np.abs(qd - qh).max()),
                "q_elements_not_bit_identical": int(np.count_nonzero(qd != qh)),
                "orthogonality_device": float(np.linalg.norm(qd @ qd.T - np.eye(n))),
                "orthogonality_host": float(np.linalg.norm(qh @ qh.T - np.eye(n)))}
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
