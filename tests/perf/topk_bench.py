"""The top-k wire's kernels next to what they replace, device-resident, in ONE process, alternated
window by window (the form of ``mxfp4_bench.py``).  Not ``bench.py``.

Client, per M and density: ``fedagg_topk_select`` + the read of nnz + ``fedagg_topk_compact`` as the
export runs them, next to the MXFP4 quantiser with its residual on the same update and to a
``copy_`` of the bytes the top-k path moves (pass 1 reads x and res and writes res, three passes and
the compaction read res once each: ``28 M + 8 nnz`` for an fp32 update).  Aggregator, per (K, M) and
density: ``fedagg_topk_fedavg`` over K stratified random rows next to ``fedagg_mx4_fedavg_e2m1`` and,
where the K fp32 rows fit ``--fp32-limit`` bytes, ``fedagg_fedavg_f32`` at the same (K, M).  The
top-k kernel's bytes are ``8 K nnz`` of rows, ``8 K M / sub_tile`` of bounds and ``4 M`` out.

Every kernel is warmed at its shape, then ``--windows`` windows per kernel are timed alternately
with device events; the figure is the median window, the range is kept beside it and ``spread`` is
the range over the median.  One JSON line per row, appended to ``--out`` when given.

    python3 tests/perf/topk_bench.py --out profiles/topk_bench.jsonl
"""

from __future__ import annotations

import argparse
import ctypes
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mxfp4_bench import _alternate, _stat  # noqa: E402  (the same windows and statistics)

ROWS = ("8x25000000", "64x125000000", "128x350000000")
SELECT = (25_000_000, 125_000_000, 350_000_000)
DENSITIES = (0.001, 0.01)


def _select(M: int, density: float, windows: int, target_s: float) -> dict:
    import torch

    from substrafl_amd import _native, _native_mx4, _native_topk

    mx4, k = _native_mx4.load(), max(1, min(M, math.ceil(density * M)))
    x = torch.randn(M, device="cuda") * 0.01
    resid = torch.zeros(M, device="cuda")
    resid4 = torch.zeros(M, device="cuda")
    ws_bytes = _native_topk.workspace(M)[0]
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    state = torch.empty(_native_topk.STATE_WORDS, dtype=torch.int32, device="cuda")
    out = torch.empty(8 * M // 4, dtype=torch.uint8, device="cuda")  # room for ties and the residual's build-up
    dst = torch.empty(-(-M // 2) + -(-M // 32), dtype=torch.uint8, device="cuda")
    stream = int(torch.cuda.current_stream().cuda_stream)
    seen = []

    def topk():
        _native_topk.select(_native.FEDAGG_F32, x.data_ptr(), resid.data_ptr(), M, k, ws.data_ptr(), ws_bytes,
                            state.data_ptr(), stream)
        nnz = int(state.cpu()[_native_topk.STATE_NNZ].item())  # the export's one read
        assert 8 * nnz <= out.numel()
        _native_topk.compact(resid.data_ptr(), M, ws.data_ptr(), state.data_ptr(), nnz, out.data_ptr(),
                             out.data_ptr() + 4 * nnz, stream)
        seen.append(nnz)

    def mxfp4_ef():
        assert mx4.fedagg_mx4_quantize(x.data_ptr(), _native.FEDAGG_F32, M, resid4.data_ptr(), dst.data_ptr(),
                                       dst.data_ptr() + -(-M // 2), stream) == 0

    moved = 28 * M + 8 * k
    a = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    t = _alternate({"topk": topk, "mxfp4_ef": mxfp4_ef, "copy_topk": lambda: b.copy_(a)}, windows, target_s, torch)
    res = {"select_M": M, "density": density, "k": k, "nnz_last": seen[-1], "windows": windows,
           "topk": _stat(t["topk"], moved), "mxfp4_ef": _stat(t["mxfp4_ef"], 12 * M + dst.numel()),
           "copy_topk": _stat(t["copy_topk"], moved)}
    res["topk_over_mxfp4_ef_time"] = round(res["topk"]["ms"] / res["mxfp4_ef"]["ms"], 3)
    res["topk_over_copy_time"] = round(res["topk"]["ms"] / res["copy_topk"]["ms"], 3)
    return res


def _row(row: str, density: float, windows: int, target_s: float, fp32_limit: int) -> dict:
    import numpy as np
    import torch

    from substrafl_amd import _native, _native_mx4, _native_topk

    K, M = (int(v) for v in row.split("x"))
    lib, mx4, tk = _native.load(), _native_mx4.load(), _native_topk.load()
    sub = _native_topk.blocking()[1]
    gen = torch.Generator(device="cuda").manual_seed(K + M % 1000)
    nnz = max(1, int(density * M))
    stride = M // nnz
    idx = torch.empty((K, nnz), dtype=torch.int32, device="cuda")
    val = torch.empty((K, nnz), dtype=torch.float32, device="cuda")
    base = torch.arange(nnz, device="cuda", dtype=torch.int64) * stride
    for k in range(K):  # stratified: ascending and unique, one index in every stride
        idx[k] = (base + torch.randint(0, stride, (nnz,), device="cuda", generator=gen)).to(torch.int32)
        val[k] = torch.randn(nnz, device="cuda", generator=gen) * 0.01
    nb, nc = -(-M // 32), -(-M // 2)
    ldc, lds = -(-nc // 256) * 256, -(-nb // 256) * 256
    codes = torch.randint(0, 256, (K, ldc), dtype=torch.uint8, device="cuda", generator=gen)
    scales = torch.randint(120, 131, (K, lds), dtype=torch.uint8, device="cuda", generator=gen)
    ldo = -(-M // 256) * 256
    out = torch.empty(ldo, dtype=torch.float32, device="cuda")
    fed_bytes = _native_topk.workspace(M, K)[1]
    ws = torch.empty(fed_bytes, dtype=torch.uint8, device="cuda")
    w = (np.random.default_rng(K).integers(100, 10000, K)).astype(np.float64)
    h_w = (ctypes.c_float * K)(*[float(v) for v in (w / w.sum()).astype(np.float32)])
    none = (ctypes.c_uint64 * 1)(0)
    h_nnz = (ctypes.c_uint64 * K)(*[nnz] * K)
    ip = _native.ptr_array([idx.data_ptr() + 4 * k * nnz for k in range(K)])
    vp = _native.ptr_array([val.data_ptr() + 4 * k * nnz for k in range(K)])
    cp = _native.ptr_array([codes.data_ptr() + k * ldc for k in range(K)])
    sp = _native.ptr_array([scales.data_ptr() + k * lds for k in range(K)])
    stream = int(torch.cuda.current_stream().cuda_stream)

    def run_topk():
        assert tk.fedagg_topk_fedavg(ip, vp, h_nnz, h_w, K, M, none, 0, ws.data_ptr(), fed_bytes, out.data_ptr(), stream) == 0

    def run_mx4():
        assert mx4.fedagg_mx4_fedavg_e2m1(cp, sp, h_w, K, M, none, 0, out.data_ptr(), stream) == 0

    fns = {"topk": run_topk, "mxfp4": run_mx4}
    dense = None
    if 4 * K * ldo <= fp32_limit:
        dense = torch.empty((K, ldo), dtype=torch.float32, device="cuda")
        for k in range(K):
            dense[k] = torch.randn(ldo, device="cuda", generator=gen)
        fp = _native.ptr_array([dense.data_ptr() + 4 * k * ldo for k in range(K)])
        fns["fp32"] = lambda: lib.fedagg_fedavg_f32(fp, h_w, K, M, none, 0, None, out.data_ptr(), stream)
        assert fns["fp32"]() == 0
    t = _alternate(fns, windows, target_s, torch)
    res = {"row": row, "K": K, "M": M, "density": density, "nnz": nnz, "windows": windows,
           "topk": _stat(t["topk"], 8 * K * nnz + 8 * K * (-(-M // sub) + 1) + 4 * M),
           "mxfp4": _stat(t["mxfp4"], K * (nc + nb) + 4 * M),
           "fp32": _stat(t["fp32"], 4 * K * M + 4 * M) if dense is not None else None}
    res["topk_over_mxfp4_time"] = round(res["topk"]["ms"] / res["mxfp4"]["ms"], 3)
    if dense is not None:
        res["topk_over_fp32_time"] = round(res["topk"]["ms"] / res["fp32"]["ms"], 3)
    del idx, val, codes, scales, out, ws, dense
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", nargs="*", default=list(ROWS))
    ap.add_argument("--select", nargs="*", type=int, default=list(SELECT))
    ap.add_argument("--densities", nargs="*", type=float, default=list(DENSITIES))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-seconds", type=float, default=0.4)
    ap.add_argument("--fp32-limit", type=int, default=96 << 30, help="skip the fp32 kernel where its K rows need more bytes")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "topk_bench.py needs an MI355X: a time measured elsewhere says nothing"
    jobs = [lambda m=m, d=d: _select(m, d, args.windows, args.window_seconds) for m in args.select for d in args.densities]
    jobs += [lambda r=r, d=d: _row(r, d, args.windows, args.window_seconds, args.fp32_limit)
             for r in args.rows for d in args.densities]
    for job in jobs:  # written row by row: a run that is cut short keeps what it measured
        line = json.dumps(job())
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
