"""NewtonRaphson's whole ``compute_averaged_states`` (newton_raphson.py:151-216) from host arrays with
the Newton system solved three ways in one process, alternated: ``solve="host"`` (the default, the
reference's ``np.linalg.solve``), ``solve="device"`` (the fp64 LU with partial pivoting) and
``solve="cholesky"`` (symmetry test, Cholesky factorisation and solve on the device; the LU only
for a sum that is not symmetric positive definite).

Rows ``KxP`` have Gram Hessians X^T D X / m + l2 I with m = P / 2 and l2 = 1e-3 (the shape
tests/perf/nr_hessian_check_bench.py uses), so the Cholesky is accepted; rows ``KxP:normal`` have
standard normal Hessians, whose sum is not symmetric: they show what the failed attempt costs
ahead of the LU.  Every figure is a range over the alternations; the device legs are split by the
session's events (``last_timing``).  Each row runs in a child process of its own under ``timeout``,
and the first row that fails ends the run.  One JSON line per row, appended to ``--out`` when given.

    python3 tests/perf/nr_cholesky_bench.py --out profiles/nr_cholesky_bench.jsonl
"""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEGS = ("host", "device", "cholesky")
SPLIT = ("sums_ms", "symcopy_ms", "factor_ms", "substitute_ms", "lu_factor_ms", "lu_substitute_ms", "fetch_s")


class _Algo:
    pass


def _rng(vals, nd=4):
    return [round(min(vals), nd), round(max(vals), nd)]


def _row(row: str, reps: int) -> dict:
    import standin_substrafl.strategies as ss
    from standin_substrafl.strategies.schemas import NewtonRaphsonSharedState
    from test_dense_potrf_gpu import _gram

    from substrafl_amd.engine import engine_for
    from substrafl_amd.integration import accelerate

    shape, _, family = row.partition(":")
    family = family or "gram"
    K, P = (int(v) for v in shape.split("x"))
    rng = np.random.default_rng(K + P)
    grads = [[rng.standard_normal(P).astype(np.float32)] for _ in range(K)]
    hess = [_gram(P, P // 2, 1e-3, seed=k) if family == "gram" else rng.standard_normal((P, P)) for k in range(K)]
    ns = [int(v) for v in rng.integers(1, 1000, K)]
    states = [NewtonRaphsonSharedState(gradients=g, hessian=h, n_samples=n) for g, h, n in zip(grads, hess, ns)]
    legs = {m: accelerate(ss.NewtonRaphson, solve=m)(algo=_Algo(), damping_factor=1.0) for m in LEGS}
    for m in ("device", "cholesky"):  # warm: session, ring, buffers, code
        legs[m].compute_averaged_states(shared_states=states, _skip=True)
    t = {m: [] for m in LEGS}
    split = {m: {k: [] for k in SPLIT} for m in ("device", "cholesky")}
    out, route = {}, {}
    for _ in range(reps):
        for m in LEGS:
            t0 = time.perf_counter()
            out[m] = legs[m].compute_averaged_states(shared_states=states, _skip=True).parameters_update
            t[m].append(time.perf_counter() - t0)
            tm = engine_for(None).last_timing
            route[m] = tm["solve"]
            for k in SPLIT:
                if m != "host" and k in tm:
                    split[m][k].append(tm[k])
    assert route["host"] == "host" and route["device"] == "device", route
    assert (route["cholesky"] == "device: cholesky") == (family == "gram"), route
    x = {m: np.concatenate([np.asarray(a).reshape(-1) for a in out[m]]) for m in LEGS}
    line = {"clients": K, "params": P, "hessians": family, "alternations": reps, "cholesky_route": route["cholesky"],
            **{f"{m}_total_s": _rng(t[m]) for m in LEGS},
            "cholesky_over_device_min_over_min": round(min(t["device"]) / min(t["cholesky"]), 2),
            "cholesky_faster_than_device": bool(max(t["cholesky"]) < min(t["device"])),
            **{f"{m}_{k}": _rng(v, 5 if k.endswith("_s") else 2) for m in split for k, v in split[m].items() if v},
            "device_solve_ms": _rng([f + s for f, s in zip(split["device"]["factor_ms"], split["device"]["substitute_ms"])], 2),
            "cholesky_solve_ms": _rng([sum(v) for v in zip(*(split["cholesky"][k] for k in SPLIT[1:6] if split["cholesky"][k]))], 2),
            **{f"rel_diff_{m}_vs_host": float(np.abs(x[m] - x["host"]).max() / np.abs(x["host"]).max())
               for m in ("device", "cholesky")}}
    if route["cholesky"] == "device: cholesky":
        line["potrf_fp64_tflops"] = round(P ** 3 / 3.0 / (min(split["cholesky"]["factor_ms"]) / 1e3) / 1e12, 3)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="8x2048,8x4096,4x8192,8x4096:normal")
    ap.add_argument("--reps", type=int, default=3, help="alternations of the three legs (at least 3)")
    ap.add_argument("--timeout", type=int, default=420, help="seconds one row's child process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--row", default=None, help="run this one row in this process and print its line")
    args = ap.parse_args()
    reps = max(3, args.reps)
    if args.row:
        print(json.dumps(_row(args.row, reps)), flush=True)
        return 0
    for row in args.rows.split(","):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--row", row,
               "--reps", str(reps)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(done.stdout)
        sys.stdout.flush()
        if done.returncode != 0:  # nothing more is started on the device after a failure
            print(f"row {row}: exit status {done.returncode}", file=sys.stderr)
            return done.returncode
        if args.out:
            with open(args.out, "a") as f:
                f.write(done.stdout.strip().splitlines()[-1] + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
