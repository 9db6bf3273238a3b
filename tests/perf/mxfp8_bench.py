"""``fedagg_mx_fedavg_e4m3`` next to ``fedagg_fedavg_bf16``, device-resident, in ONE process at the
same (K, M), alternated window by window, plus the quantiser's time.  Not ``bench.py``.

Per row: every kernel is warmed at the row's shape, then ``--windows`` windows per kernel are timed
alternately (MXFP8, bf16, MXFP8, ...) with device events around ``--steps`` back-to-back launches
(enough launches that a window lasts a good fraction of a second); the figure is the median window
and the range over the windows is kept beside it.  Algorithmic bytes are what the reduction must
move, computed from the shape: ``K M + K ceil(M / 32) + 4 M`` (MXFP8) and ``2 K M + 4 M`` (bf16);
TB/s and the fraction of the 8 TB/s HBM peak follow from them.  One JSON line per row, appended to
``--out`` when given.

    python3 tests/perf/mxfp8_bench.py --out profiles/mxfp8_bench.jsonl
"""

from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
ROWS = ("8x25000000", "64x125000000", "128x350000000")
QUANT = (25_000_000, 350_000_000)


def _windows(fn, steps: int, windows: int, torch):
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / steps)
    return out


def _stat(ms, nbytes: int) -> dict:
    med = statistics.median(ms)
    return {"ms": round(med, 4), "ms_range": [round(min(ms), 4), round(max(ms), 4)], "bytes": nbytes,
            "TBps": round(nbytes / med / 1e9, 3), "of_8TBps": round(nbytes / (med * 1e-3) / HBM_PEAK, 3)}


def _row(row: str, windows: int, target_s: float) -> dict:
    import numpy as np
    import torch

    from substrafl_amd import _native, _native_mx

    K, M = (int(v) for v in row.split("x"))
    lib, mx = _native.load(), _native_mx.load()
    nb = -(-M // 32)
    ldc, lds, ldb = -(-M // 256) * 256, -(-nb // 256) * 256, -(-M // 128) * 128
    gen = torch.Generator(device="cuda").manual_seed(K + M % 1000)
    codes = torch.randint(0, 0x7F, (K, ldc), dtype=torch.uint8, device="cuda", generator=gen)  # finite codes, both signs below
    codes |= torch.randint(0, 2, (K, ldc), dtype=torch.uint8, device="cuda", generator=gen) << 7
    scales = torch.randint(120, 131, (K, lds), dtype=torch.uint8, device="cuda", generator=gen)
    rows16 = torch.empty((K, ldb), dtype=torch.bfloat16, device="cuda")
    for k in range(K):  # row by row: no fp32 temporary of the whole bucket
        rows16[k] = torch.randn(ldb, device="cuda", generator=gen).to(torch.bfloat16)
    out = torch.empty(ldc, dtype=torch.float32, device="cuda")
    w = (np.random.default_rng(K).integers(100, 10000, K)).astype(np.float64)
    w = (w / w.sum()).astype(np.float32)
    h_w = (ctypes.c_float * K)(*[float(v) for v in w])
    idx = (ctypes.c_uint64 * 1)(0)
    cp = _native.ptr_array([codes.data_ptr() + k * ldc for k in range(K)])
    sp = _native.ptr_array([scales.data_ptr() + k * lds for k in range(K)])
    bp = _native.ptr_array([rows16.data_ptr() + k * ldb * 2 for k in range(K)])
    stream = int(torch.cuda.current_stream().cuda_stream)

    def run_mx():
        rc = mx.fedagg_mx_fedavg_e4m3(cp, sp, h_w, K, M, idx, 0, out.data_ptr(), stream)
        assert rc == 0, mx.fedagg_mx_last_error()

    def run_bf16():
        rc = lib.fedagg_fedavg_bf16(bp, h_w, K, M, idx, 0, None, out.data_ptr(), stream)
        assert rc == 0, lib.fedagg_last_error()

    for fn in (run_mx, run_bf16):  # warm-up at this shape: code objects, clocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    once = {name: _windows(fn, 2, 1, torch)[0] for name, fn in (("mx", run_mx), ("bf16", run_bf16))}
    steps = {name: max(3, min(20000, int(target_s * 1e3 / ms))) for name, ms in once.items()}
    t = {"mx": [], "bf16": []}
    for _ in range(windows):  # alternated: both kernels see the same machine
        t["mx"] += _windows(run_mx, steps["mx"], 1, torch)
        t["bf16"] += _windows(run_bf16, steps["bf16"], 1, torch)
    res = {"row": row, "K": K, "M": M, "windows": windows, "steps_per_window": steps,
           "mxfp8": _stat(t["mx"], K * M + K * nb + 4 * M), "bf16": _stat(t["bf16"], 2 * K * M + 4 * M)}
    res["mxfp8_over_bf16_time"] = round(res["mxfp8"]["ms"] / res["bf16"]["ms"], 3)
    del codes, scales, rows16, out
    torch.cuda.empty_cache()
    return res


def _quantize(M: int, windows: int, target_s: float) -> dict:
    import torch

    from substrafl_amd import _native, _native_mx

    mx = _native_mx.load()
    nb = -(-M // 32)
    x = torch.randn(M, device="cuda") * 0.01
    dst = torch.empty(M + nb, dtype=torch.uint8, device="cuda")
    stream = int(torch.cuda.current_stream().cuda_stream)
    res = {"quantize_M": M}
    for name, kind, src in (("f32", _native.FEDAGG_F32, x), ("bf16", _native.FEDAGG_BF16, x.to(torch.bfloat16))):
        def run():
            rc = mx.fedagg_mx_quantize(src.data_ptr(), kind, M, dst.data_ptr(), dst.data_ptr() + M, stream)
            assert rc == 0, mx.fedagg_mx_last_error()

        for _ in range(3):
            run()
        torch.cuda.synchronize()
        once = _windows(run, 2, 1, torch)[0]
        steps = max(3, min(20000, int(target_s * 1e3 / once)))
        ms = [_windows(run, steps, 1, torch)[0] for _ in range(windows)]
        res[name] = _stat(ms, M * src.element_size() + M + nb)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", nargs="*", default=list(ROWS))
    ap.add_argument("--quantize", nargs="*", type=int, default=list(QUANT))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-seconds", type=float, default=0.4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "mxfp8_bench.py needs an MI355X: a time measured elsewhere says nothing"
    jobs = [lambda r=r: _row(r, args.windows, args.window_seconds) for r in args.rows]
    jobs += [lambda m=m: _quantize(m, args.windows, args.window_seconds) for m in args.quantize]
    for job in jobs:  # written row by row: a run that is cut short keeps what it measured
        line = json.dumps(job())
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
