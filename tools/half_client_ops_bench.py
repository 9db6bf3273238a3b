#!/usr/bin/env python3
"""One client round of weight moves on an fp16 / bf16 model on one MI355X: the flat-bucket path of
substrafl_amd.algorithms.weight_manager against the per-layer torch path the package took for
16-bit models before the flat kernels carried them (the reference's loops,
weight_manager.py:79-212: a clone per layer, ``sum(param * coeff)``, ``w += m * u`` per layer, and
one ``.cpu().numpy()`` per layer for the export -- which raises for bf16, so the bf16 baseline
stops before the export).

The round: ``increment_parameters`` (the averaged update: host layers of the model's kind for fp16,
the engine's fp32 average for bf16), ``get_parameters``, ``subtract_parameters``, ``export_numpy``.
Wall time per step with a device synchronisation before and after (host work included: that is
what a client pays), --warmup rounds, then --iters timed rounds; median and min-max spread.  Also
the share of elements on the element-by-element path of the 16-bit kernels (layers whose slice
of the bucket is not 16-B aligned), and with --engine the host-path rate of ``engine.fedavg`` for
8 x 25M wire.BF16 inputs next to 8 x 25M fp32.  One JSON line per result."""

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def shapes_many(total):
    """About 300 layers: 100 blocks of (weight matrix, bias, a norm vector of odd length)."""
    blocks = 100
    side = int((total / blocks) ** 0.5) // 8 * 8
    out = []
    for _ in range(blocks):
        out += [(side, side), (side,), (side - 1,)]
    return out


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(ts.min()), 3),
            "max_ms": round(float(ts.max()), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=25_000_000)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--engine", action="store_true")
    args = ap.parse_args()
    import torch

    from substrafl_amd import wire
    from substrafl_amd.algorithms import weight_manager as wm

    dev = torch.device("cuda", 0)

    class Net(torch.nn.Module):
        def __init__(self, shapes, dtype):
            super().__init__()
            self.ps = torch.nn.ParameterList(
                [torch.nn.Parameter(torch.randn(s).to(dtype), requires_grad=False) for s in shapes])

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for model_name, shapes in (("many_layers", shapes_many(args.M)), ("one_layer", [(args.M,)])):
        for dtype in (torch.float16, torch.bfloat16):
            torch.manual_seed(0)
            numel = [int(np.prod(s)) for s in shapes]
            M = sum(numel)
            rng = np.random.default_rng(0)
            avg32 = (rng.standard_normal(M) * 1e-3).astype(np.float32)
            if dtype == torch.float16:
                avg = avg32.astype(np.float16)
            else:
                avg = avg32  # a bf16 federation receives the engine's fp32 average
            avg_layers = [v.reshape(s) for v, s in zip(np.split(avg, np.cumsum(numel)[:-1]), shapes)]

            def train_step(model):
                with torch.no_grad():
                    for p in model.parameters():
                        p.mul_(1.0009765625)  # stands for the local training: the weights change

            def round_flat(model):
                t = {}
                t["increment"], _ = timed(lambda: wm.increment_parameters(model, avg_layers,
                                                                          with_batch_norm_parameters=False))
                t["get_parameters"], before = timed(lambda: wm.get_parameters(model, False))
                train_step(model)
                after = wm.get_parameters(model, False)
                t["subtract"], delta = timed(lambda: wm.subtract_parameters(after, before))
                wm.set_parameters(model, before, False)
                t["export_numpy"], host = timed(lambda: wm.export_numpy(delta, wire=True, tag="bench"))
                return t, host

            def round_torch(model):
                params = list(model.parameters())
                t = {}

                def inc():
                    with torch.no_grad():
                        for w, u in zip(params, avg_layers):
                            w.data += 1.0 * torch.from_numpy(u).to(w.device)

                t["increment"], _ = timed(inc)
                t["get_parameters"], before = timed(lambda: [p.detach().clone() for p in params])
                train_step(model)
                after = [p.detach().clone() for p in params]

                def sub():
                    with torch.no_grad():
                        return [sum(a * c for a, c in zip(pair, [1, -1])) for pair in zip(after, before)]

                t["subtract"], delta = timed(sub)
                with torch.no_grad():
                    for p, b in zip(params, before):
                        p.data = b.data
                if dtype == torch.float16:
                    t["export_numpy"], host = timed(lambda: [d.cpu().detach().numpy() for d in delta])
                else:
                    host = None  # .numpy() raises for bf16: the per-layer path ends here
                return t, host

            results = {}
            for path, fn in (("torch_per_layer", round_torch), ("flat_bucket", round_flat)):
                model = Net(shapes, dtype).to(dev)
                rounds = []
                for i in range(args.warmup + args.iters):
                    t, host = fn(model)
                    if i >= args.warmup:
                        rounds.append(t)
                    del host
                steps = {k: stats([r[k] for r in rounds]) for k in rounds[0]}
                common = [k for k in rounds[0] if k != "export_numpy"]
                steps["round_without_export"] = stats([sum(r[k] for k in common) for r in rounds])
                if "export_numpy" in rounds[0]:
                    steps["round"] = stats([sum(r.values()) for r in rounds])
                results[path] = steps
                print(json.dumps({"model": model_name, "layers": len(shapes), "params": M,
                                  "dtype": str(dtype).replace("torch.", ""), "path": path, **steps}), flush=True)
            key = "round" if dtype == torch.float16 else "round_without_export"
            a, b = results["torch_per_layer"][key], results["flat_bucket"][key]
            spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
            print(json.dumps({"model": model_name, "dtype": str(dtype).replace("torch.", ""), "compared": key,
                              "torch_per_layer_median_ms": a["median_ms"], "flat_bucket_median_ms": b["median_ms"],
                              "larger_spread_ms": round(spread, 3),
                              "faster_by_more_than_spread": bool(a["median_ms"] - b["median_ms"] > spread)}),
                  flush=True)
        # elements whose layer's slice of the bucket is not 16-B aligned (the element-by-element path
        # once the layers are views of a bucket), and the odd-offset share among them
        off, slow, odd = 0, 0, 0
        for n in numel:
            if off % 8:
                slow += n
            if off % 2:
                odd += n
            off += n
        print(json.dumps({"model": model_name, "elements": M, "share_not_16B_aligned": round(slow / M, 4),
                          "share_odd_offset": round(odd / M, 4)}), flush=True)

    if args.engine:
        from substrafl_amd.engine import AggregationEngine

        K, M = 8, args.M
        rng = np.random.default_rng(1)
        eng = AggregationEngine(device=0)
        ns = [int(v) for v in rng.integers(1, 5000, K)]
        base = rng.standard_normal(M).astype(np.float32)
        for name, rows in (("bf16", [wire.bucket_views(wire.float32_to_bf16(base * (k + 1)), [(M,)]) for k in range(K)]),
                           ("f32", [wire.bucket_views(base * (k + 1), [(M,)]) for k in range(K)])):
            ts = []
            for i in range(args.warmup + args.iters):
                t0 = time.perf_counter()
                out = eng.fedavg(rows, ns)
                dt = time.perf_counter() - t0
                if i >= args.warmup:
                    ts.append(dt)
                del out
            nbytes = K * M * rows[0][0].dtype.itemsize + M * 4
            print(json.dumps({"engine_fedavg": f"{K}x{M // 1_000_000}M {name}", **stats(ts),
                              "GBps_in_plus_out": round(nbytes / float(np.median(ts)) / 1e9, 1),
                              "layout": eng.last_timing.get("layout")}), flush=True)


if __name__ == "__main__":
    main()
