#!/usr/bin/env python3
"""Scaffold over 16-bit buckets on one MI355X, device-resident, HIP-event times.

Two legs over the same K x M fp16 / bf16 delta and control-variate rows and a 16-bit c:

  (a) the promoted route the engine took before ``fedagg_scaffold_bucket``: cast both [K, M]
      blocks and c to fp64 (``fedagg_cast``, what ``Session.cast`` calls), then
      ``fedagg_scaffold_f64``.  ``fedagg_cast`` has no bf16 input, so for bf16 the rows are first
      upcast to fp32 by torch (exact, outside the timed window) and the cast reads 4-byte
      elements; this leg never existed for bf16 in the engine, which refused bf16 Scaffold.
  (b) two ``fedagg_scaffold_bucket`` calls on the 2-byte rows.

The legs alternate --alternations times in one process, each window --iters back-to-back calls
between two events after --warmup untimed ones; the outputs of (a) and (b) are compared bit for
bit at the timed size.  Leg (b)'s algorithmic bytes (2 K M per bucket + c + 8 M out each) per
second are set beside those of ``fedagg_scaffold_f32`` on fp32 rows of the same shape, as
fractions of 8 TB/s.  --engine times the engine call behind ``Scaffold.avg_shared_states`` from fp16
host arrays at 16 x M (``scaffold_per_bucket``; ``scaffold`` on a tree from before it: run this
file against either tree with --engine-only --repo PATH).  One JSON line per result."""

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

HBM_PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=25_000_000)
    ap.add_argument("--K", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--engine", action="store_true")
    ap.add_argument("--engine-only", action="store_true")
    ap.add_argument("--repo", default=str(Path(__file__).resolve().parents[1]), help="tree whose package is timed")
    args = ap.parse_args()
    sys.path.insert(0, args.repo)
    import torch

    from substrafl_amd import _native

    lib = _native.load()
    if not args.engine_only:
        device_legs(args, torch, lib, _native)
    if args.engine or args.engine_only:
        engine_leg(args)


def device_legs(args, torch, lib, _native):
    from substrafl_amd.engine import ScaffoldBucketPlan, ScaffoldPlan

    F16, F32, F64 = _native.FEDAGG_F16, _native.FEDAGG_F32, _native.FEDAGG_F64
    M = args.M
    stream = torch.cuda.current_stream()
    sh = int(stream.cuda_stream)

    def window(fn):
        for _ in range(args.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.iters):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.iters  # ms per call

    def cast(src, kind_in, dst, n):
        _native.check(lib.fedagg_cast(src.data_ptr(), kind_in, dst.data_ptr(), F64, n, sh), "cast")

    for K in args.K:
        w = np.random.default_rng(K).integers(1, 5000, K)
        w = (w / w.sum()).astype(np.float64)
        for kind, tdt in (("f16", torch.float16), ("bf16", torch.bfloat16)):
            torch.manual_seed(K)
            d16 = torch.randn(K, M, device="cuda", dtype=torch.float32).to(tdt)
            cv16 = torch.randn(K, M, device="cuda", dtype=torch.float32).to(tdt)
            c16 = torch.randn(M, device="cuda", dtype=torch.float32).to(tdt)
            # leg (a): fp64 blocks written by the cast inside the window
            src_d, src_cv, src_c, kin = (d16, cv16, c16, F16) if kind == "f16" else (d16.float(), cv16.float(),
                                                                                       c16.float(), F32)
            d64 = torch.empty(K, M, device="cuda", dtype=torch.float64)
            cv64 = torch.empty(K, M, device="cuda", dtype=torch.float64)
            c64 = torch.empty(M, device="cuda", dtype=torch.float64)
            out_a = [torch.empty(M, device="cuda", dtype=torch.float64) for _ in range(2)]
            out_b = [torch.empty(M, device="cuda", dtype=torch.float64) for _ in range(2)]
            plan_a = ScaffoldPlan("f64", d64, cv64, c64, w, M, 0.7, out_a[0], out_a[1])
            plan_b = [ScaffoldBucketPlan(kind, d16, 0, None, None, w, M, 0.7, out_b[0]),
                      ScaffoldBucketPlan(kind, cv16, 1, c16, kind, w, M, 0.7, out_b[1])]

            def leg_a():
                cast(src_d, kin, d64, K * M)
                cast(src_cv, kin, cv64, K * M)
                cast(src_c, kin, c64, M)
                plan_a.launch(sh)

            def leg_b():
                plan_b[0].launch(sh)
                plan_b[1].launch(sh)

            ta, tb = [], []
            for _ in range(args.alternations):
                ta.append(window(leg_a))
                tb.append(window(leg_b))
            same = all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(out_a, out_b))
            bytes_b = sum(p.bytes_alg() for p in plan_b)
            spread = max(max(ta) - min(ta), max(tb) - min(tb))
            print(json.dumps({
                "shape": f"{K}x{M // 1_000_000}M", "kind": kind, "a_cast_f64_ms": [round(t, 3) for t in ta],
                "b_bucket16_ms": [round(t, 3) for t in tb], "a_median_ms": round(float(np.median(ta)), 3),
                "b_median_ms": round(float(np.median(tb)), 3), "larger_spread_ms": round(spread, 3),
                "b_faster_beyond_spread": bool(min(ta) - max(tb) > spread), "outputs_bit_identical": bool(same),
                "b_alg_bytes": bytes_b, "b_alg_TBps": round(bytes_b / (float(np.median(tb)) * 1e-3) / 1e12, 3),
                "b_fraction_of_8TBps": round(bytes_b / (float(np.median(tb)) * 1e-3) / HBM_PEAK, 3),
                "a_note": "rows upcast to fp32 by torch outside the window; never an engine path" if kind == "bf16"
                else "the engine's route before fedagg_scaffold_bucket"}), flush=True)
            del d16, cv16, c16, src_d, src_cv, src_c, d64, cv64, c64, plan_a, plan_b
            torch.cuda.empty_cache()
        # the fp32 Scaffold kernel on fp32 rows of the same shape, same session
        d32 = torch.randn(K, M, device="cuda")
        cv32 = torch.randn(K, M, device="cuda")
        c32 = torch.randn(M, device="cuda")
        outs = [torch.empty(M, device="cuda", dtype=torch.float64) for _ in range(2)]
        plan = ScaffoldPlan("f32", d32, cv32, c32, w, M, 0.7, outs[0], outs[1])
        ts = [window(lambda: plan.launch(sh)) for _ in range(args.alternations)]
        print(json.dumps({"shape": f"{K}x{M // 1_000_000}M", "kind": "f32", "scaffold_f32_ms": [round(t, 3) for t in ts],
                          "alg_bytes": plan.bytes_alg(),
                          "fraction_of_8TBps": round(plan.bytes_alg() / (float(np.median(ts)) * 1e-3) / HBM_PEAK, 3)}),
              flush=True)
        del d32, cv32, c32, plan
        torch.cuda.empty_cache()


def engine_leg(args):
    from substrafl_amd.engine import AggregationEngine

    K, M = 16, args.M
    rng = np.random.default_rng(3)
    base = rng.standard_normal(M).astype(np.float32)
    pus = [[(base * (1 + k / 64)).astype(np.float16)] for k in range(K)]
    cvs = [[(base * (2 - k / 64)).astype(np.float16)] for k in range(K)]
    c = [base.astype(np.float16)]
    ns = [int(v) for v in rng.integers(1, 5000, K)]
    eng = AggregationEngine(device=0)
    ts = []
    for i in range(args.warmup + args.iters):
        t0 = time.perf_counter()
        out = getattr(eng, "scaffold_per_bucket", eng.scaffold)(pus, cvs, [c] * K, ns, 0.7)  # what the strategy calls
        dt = time.perf_counter() - t0
        if i >= args.warmup:
            ts.append(dt * 1e3)
        check = float(out[2][0][:8].sum())
        del out
    print(json.dumps({"engine_scaffold": f"{K}x{M // 1_000_000}M f16 host arrays", "repo": args.repo,
                      "call_ms": [round(t, 1) for t in ts], "median_ms": round(float(np.median(ts)), 1),
                      "bucket_kinds": eng.last_timing.get("bucket_kinds"), "checksum": check}), flush=True)


if __name__ == "__main__":
    main()
