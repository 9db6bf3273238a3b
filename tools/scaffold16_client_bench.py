#!/usr/bin/env python3
"""The weight moves of a round >= 2 Scaffold client of an fp16 / bf16 model on one MI355X
(algorithms/accelerate.py ``train``): the aggregator's fp64 ``avg_parameters_update`` and
``server_control_variate`` have come back, so every move mixes the model's 16-bit kind with fp64.
With the promoted flat ops (libfedagg_promote.so) against ``FEDAGG_FLAT_PROMOTE=0`` on the same
build, which keeps those operand sets on the reference's per-layer torch loops -- the package's
behaviour before the promoted ops.

The ops, in the order of ``train``: ``update`` (increment by the fp64 host layers),
``delta_variate`` (c_i - c), ``hook`` (w += lr * delta_variate, --steps times, each timed),
``delta`` (after - before, 16-bit: the same launch on both paths), ``cv_update``
(-c - delta / (lr n)), ``ci_add`` (c_i + cv_update), and the three exports.  The client's state
is that of round 2 (c_i of the model's kind, c fp64) and is put back after every round.
Wall time per op with a device synchronisation before and after (host work included: that is
what a client pays), --warmup rounds, then --iters timed rounds; median and min-max.  One JSON
line per (dtype, path), then one per op comparing the two medians with the torch path's spread."""

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from half_client_ops_bench import shapes_many, stats  # noqa: E402

PROMOTED = ("update", "delta_variate", "hook", "cv_update", "ci_add")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=25_000_000)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--dtypes", default="float16,bfloat16")
    ap.add_argument("--paths", default="promote,torch", help="promote: the flat kernels; torch: FEDAGG_FLAT_PROMOTE=0")
    args = ap.parse_args()
    import torch

    from substrafl_amd.algorithms import weight_manager as wm

    dev = torch.device("cuda", 0)
    lr = 0.05
    shapes = shapes_many(args.M)
    numel = [int(np.prod(s)) for s in shapes]
    M = sum(numel)

    class Net(torch.nn.Module):
        def __init__(self, dtype):
            super().__init__()
            self.ps = torch.nn.ParameterList(
                [torch.nn.Parameter(torch.randn(s).to(dtype), requires_grad=False) for s in shapes])

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def layers(flat):
        return [v.reshape(s) for v, s in zip(np.split(flat, np.cumsum(numel)[:-1]), shapes)]

    rng = np.random.default_rng(0)
    avg = layers(rng.standard_normal(M) * 1e-3)  # the aggregator's fp64 outputs: views of one host array each
    c_host = layers(rng.standard_normal(M) * 1e-2)

    def one_round(model, c_i, c):
        t = {}
        t["update"], _ = timed(lambda: wm.increment_parameters(model, avg, with_batch_norm_parameters=False))
        before = wm.get_parameters(model, False)
        t["delta_variate"], dv = timed(lambda: wm.subtract_parameters(c_i, c))
        hooks = []
        for _ in range(args.steps):
            with torch.no_grad():
                for p in model.parameters():
                    p.mul_(1.0009765625)  # stands for the optimizer step: the weights change
            dt, _ = timed(lambda: wm.increment_parameters(model, dv, with_batch_norm_parameters=False,
                                                          updates_multiplier=lr))
            hooks.append(dt)
        t["hook"] = float(np.median(hooks))
        after = wm.get_parameters(model, False)
        t["delta"], delta = timed(lambda: wm.subtract_parameters(after, before))
        t["cv_update"], cv = timed(lambda: wm.weighted_sum_parameters([c, delta], [-1.0, -1.0 / (lr * args.steps)]))
        t["ci_add"], new_ci = timed(lambda: wm.add_parameters(c_i, cv))
        wm.set_parameters(model, before, False)
        t["export_delta"], h1 = timed(lambda: wm.export_numpy(delta, wire=False, tag="export"))
        t["export_cv"], h2 = timed(lambda: wm.export_numpy(cv, wire=False, tag="export_cv"))
        t["export_c"], h3 = timed(lambda: wm.export_numpy(c, wire=False, tag="export_c"))
        t["all_hooks"] = float(np.sum(hooks))
        t["round"] = sum(v for k, v in t.items() if k not in ("hook", "round"))
        assert all(x.dtype == torch.float64 for x in dv + cv + new_ci)
        return t

    for dtype in [getattr(torch, d) for d in args.dtypes.split(",")]:
        name = str(dtype).replace("torch.", "")
        results = {}
        for path in args.paths.split(","):
            os.environ["FEDAGG_FLAT_PROMOTE"] = "1" if path == "promote" else "0"
            torch.manual_seed(0)
            model = Net(dtype).to(dev)
            # round-2 state: c_i of the model's kind (round 1's c_i + cv_update), c as it arrives
            c_i = wm.add_parameters(wm.zeros_like_parameters(model, False, dev),
                                    [torch.randn(s, device=dev).to(dtype) * 1e-2 for s in shapes])
            c = wm.to_device(c_host, dev)
            rounds = []
            for i in range(args.warmup + args.iters):
                t = one_round(model, c_i, c)
                if i >= args.warmup:
                    rounds.append(t)
            results[path] = {k: stats([r[k] for r in rounds]) for k in rounds[0]}
            print(json.dumps({"bench": "scaffold16_client", "layers": len(shapes), "params": M, "dtype": name,
                              "steps": args.steps, "path": path, **results[path]}), flush=True)
            del model, c_i, c
            torch.cuda.empty_cache()
        if "promote" in results and "torch" in results:
            for op in PROMOTED + ("round",):
                a, b = results["torch"][op], results["promote"][op]
                spread = a["max_ms"] - a["min_ms"]
                print(json.dumps({"bench": "scaffold16_client", "dtype": name, "op": op,
                                  "torch_median_ms": a["median_ms"], "promote_median_ms": b["median_ms"],
                                  "torch_spread_ms": round(spread, 3),
                                  "speedup": round(a["median_ms"] / max(b["median_ms"], 1e-6), 1),
                                  "faster_by_more_than_spread": bool(a["median_ms"] - b["median_ms"] > spread)}),
                      flush=True)
    os.environ.pop("FEDAGG_FLAT_PROMOTE", None)


if __name__ == "__main__":
    main()
