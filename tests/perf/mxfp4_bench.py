"""``fedagg_mx4_fedavg_e2m1`` next to ``fedagg_mx_fedavg_e4m3`` and ``fedagg_fedavg_bf16``,
device-resident, in ONE process at the same (K, M), alternated window by window; then the MXFP4
quantiser (plain and with the residual) next to the MXFP8 one, the fused mxef one and a ``copy_`` of
the same byte counts.  Not ``bench.py``.

Per row: every kernel is warmed at the row's shape, then ``--windows`` windows per kernel are timed
alternately with device events around enough back-to-back launches that a window lasts a good
fraction of a second; the figure is the median window, the range over the windows is kept beside
it, and ``spread`` is that range over the median.  Algorithmic bytes are what a kernel must move:
``K (M/2 + M/32) + 4 M`` (MXFP4), ``K (M + M/32) + 4 M`` (MXFP8), ``2 K M + 4 M`` (bf16); TB/s and
the fraction of the 8 TB/s HBM peak follow from them.  ``mxfp4_faster_than_mxfp8`` is the bar: the
MXFP4 median below the MXFP8 median by more than the larger of the two ranges.  One JSON line per
row, appended to ``--out`` when given.

    python3 tests/perf/mxfp4_bench.py --out profiles/mxfp4_bench.jsonl
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
QUANT = (25_000_000, 125_000_000, 350_000_000)


def _window(fn, steps: int, torch) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def _stat(ms, nbytes: int) -> dict:
    med = statistics.median(ms)
    return {"ms": round(med, 4), "ms_range": [round(min(ms), 4), round(max(ms), 4)],
            "spread": round((max(ms) - min(ms)) / med, 4), "bytes": nbytes,
            "TBps": round(nbytes / med / 1e9, 3), "of_8TBps": round(nbytes / (med * 1e-3) / HBM_PEAK, 3)}


def _alternate(fns: dict, windows: int, target_s: float, torch) -> dict:
    """name -> the per-launch milliseconds of ``windows`` windows, the kernels taking turns."""
    for fn in fns.values():  # warm-up at this shape: code objects, clocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    steps = {n: max(3, min(20000, int(target_s * 1e3 / _window(fn, 2, torch)))) for n, fn in fns.items()}
    t = {n: [] for n in fns}
    for _ in range(windows):
        for n, fn in fns.items():
            t[n].append(_window(fn, steps[n], torch))
    return t


def _row(row: str, windows: int, target_s: float) -> dict:
    import numpy as np
    import torch

    from substrafl_amd import _native, _native_mx, _native_mx4

    K, M = (int(v) for v in row.split("x"))
    lib, mx, mx4 = _native.load(), _native_mx.load(), _native_mx4.load()
    nb = -(-M // 32)
    ldc, lds, ldb = -(-M // 256) * 256, -(-nb // 256) * 256, -(-M // 128) * 128
    gen = torch.Generator(device="cuda").manual_seed(K + M % 1000)
    # one code buffer serves both wires: finite e4m3 codes are also 2 finite e2m1 codes per byte
    codes = torch.randint(0, 0x7F, (K, ldc), dtype=torch.uint8, device="cuda", generator=gen)
    codes |= torch.randint(0, 2, (K, ldc), dtype=torch.uint8, device="cuda", generator=gen) << 7
    scales = torch.randint(120, 131, (K, lds), dtype=torch.uint8, device="cuda", generator=gen)
    rows16 = torch.empty((K, ldb), dtype=torch.bfloat16, device="cuda")
    for k in range(K):  # row by row: no fp32 temporary of the whole bucket
        rows16[k] = torch.randn(ldb, device="cuda", generator=gen).to(torch.bfloat16)
    out = torch.empty(ldc, dtype=torch.float32, device="cuda")
    w = (np.random.default_rng(K).integers(100, 10000, K)).astype(np.float64)
    h_w = (ctypes.c_float * K)(*[float(v) for v in (w / w.sum()).astype(np.float32)])
    idx = (ctypes.c_uint64 * 1)(0)
    cp = _native.ptr_array([codes.data_ptr() + k * ldc for k in range(K)])
    sp = _native.ptr_array([scales.data_ptr() + k * lds for k in range(K)])
    bp = _native.ptr_array([rows16.data_ptr() + k * ldb * 2 for k in range(K)])
    stream = int(torch.cuda.current_stream().cuda_stream)

    def run_mx4():
        assert mx4.fedagg_mx4_fedavg_e2m1(cp, sp, h_w, K, M, idx, 0, out.data_ptr(), stream) == 0

    def run_mx8():
        assert mx.fedagg_mx_fedavg_e4m3(cp, sp, h_w, K, M, idx, 0, out.data_ptr(), stream) == 0

    def run_bf16():
        assert lib.fedagg_fedavg_bf16(bp, h_w, K, M, idx, 0, None, out.data_ptr(), stream) == 0

    t = _alternate({"mxfp4": run_mx4, "mxfp8": run_mx8, "bf16": run_bf16}, windows, target_s, torch)
    res = {"row": row, "K": K, "M": M, "windows": windows,
           "mxfp4": _stat(t["mxfp4"], K * (-(-M // 2) + nb) + 4 * M), "mxfp8": _stat(t["mxfp8"], K * (M + nb) + 4 * M),
           "bf16": _stat(t["bf16"], 2 * K * M + 4 * M)}
    res["mxfp4_over_mxfp8_time"] = round(res["mxfp4"]["ms"] / res["mxfp8"]["ms"], 3)
    rng = max(r["ms_range"][1] - r["ms_range"][0] for r in (res["mxfp4"], res["mxfp8"]))
    res["mxfp4_faster_than_mxfp8"] = bool(res["mxfp8"]["ms"] - res["mxfp4"]["ms"] > rng)
    del codes, scales, rows16, out
    torch.cuda.empty_cache()
    return res


def _quantize(M: int, windows: int, target_s: float) -> dict:
    import torch

    from substrafl_amd import _native, _native_mx, _native_mx4, _native_mxef

    mx, mx4, mxef = _native_mx.load(), _native_mx4.load(), _native_mxef.load()
    nb, nc = -(-M // 32), -(-M // 2)
    x = torch.randn(M, device="cuda") * 0.01
    resid = torch.zeros(M, device="cuda")
    dst = torch.empty(M + nb, dtype=torch.uint8, device="cuda")
    stream = int(torch.cuda.current_stream().cuda_stream)
    res = {"quantize_M": M}
    for name, kind, src in (("f32", _native.FEDAGG_F32, x), ("bf16", _native.FEDAGG_BF16, x.to(torch.bfloat16))):
        esz = src.element_size()
        byte_counts = {"mxfp4": M * esz + nc + nb, "mxfp4_ef": M * esz + 8 * M + nc + nb, "mxfp8": M * esz + M + nb,
                       "mxfp8_ef": M * esz + 8 * M + M + nb}
        a = {n: torch.empty(b // 2, dtype=torch.uint8, device="cuda") for n, b in byte_counts.items() if "mxfp4" in n}
        b = {n: torch.empty_like(t) for n, t in a.items()}
        p = (src.data_ptr(), kind, M)
        fns = {
            "mxfp4": lambda: mx4.fedagg_mx4_quantize(*p, None, dst.data_ptr(), dst.data_ptr() + nc, stream),
            "mxfp4_ef": lambda: mx4.fedagg_mx4_quantize(*p, resid.data_ptr(), dst.data_ptr(), dst.data_ptr() + nc, stream),
            "mxfp8": lambda: mx.fedagg_mx_quantize(*p, dst.data_ptr(), dst.data_ptr() + M, stream),
            "mxfp8_ef": lambda: mxef.fedagg_mxef_quantize(*p, resid.data_ptr(), dst.data_ptr(), dst.data_ptr() + M, stream),
            "copy_mxfp4": lambda: b["mxfp4"].copy_(a["mxfp4"]),  # a copy that moves the same bytes (half read, half written)
            "copy_mxfp4_ef": lambda: b["mxfp4_ef"].copy_(a["mxfp4_ef"]),
        }
        for n in ("mxfp4", "mxfp4_ef", "mxfp8", "mxfp8_ef"):
            assert fns[n]() == 0, n
        t = _alternate(fns, windows, target_s, torch)
        res[name] = {n: _stat(ms, byte_counts[n.replace("copy_", "")]) for n, ms in t.items()}
        del a, b
        torch.cuda.empty_cache()
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

    assert torch.cuda.is_available(), "mxfp4_bench.py needs an MI355X: a time measured elsewhere says nothing"
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
