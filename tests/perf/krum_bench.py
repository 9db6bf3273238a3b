"""``fedagg_krum_gram`` next to ``fedagg_fedavg_f32`` / ``fedagg_fedavg_bf16`` and ``fedagg_robust_mean``
(t = 0) on the same device-resident rows, in ONE process, alternated window by window (``_alternate``
/ ``_stat`` of ``mxfp4_bench.py``: the median of the windows, the range kept beside it).  Not ``bench.py``.

The Gram kernel reads ``esz K M`` bytes once and issues ``nb (nb + 1) / 2`` tiles of 16 x 16 per
element column, ``nb = ceil(K / 16)``: ``2 * 256 * tiles * M`` flops on v_mfma_f64_16x16x4_f64.
``of_8TBps`` is its share of 8 TB/s on those bytes, ``of_mfma`` its share of the fp64 matrix rate
(``--mfma-tflops``, the datasheet's 78.6), and ``bound`` names the larger of the two shares.  One JSON
line per row, appended to ``--out`` when given; a row that cannot be run is reported with its reason.

    python3 tests/perf/krum_bench.py --out profiles/krum_bench.jsonl
"""

from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mxfp4_bench import ROOT, _alternate, _stat  # noqa: E402  (puts the repository root on sys.path)

ROWS = ("8x25000000xf32", "32x125000000xf32", "64x125000000xf32", "128x350000000xbf16")


def _row(row: str, windows: int, target_s: float, mfma_tflops: float) -> dict:
    import numpy as np
    import torch

    from substrafl_amd import _native, _native_krum, _native_robust

    K, M, kind = row.split("x")
    K, M = int(K), int(M)
    lib, rb, kr = _native.load(), _native_robust.load(), _native_krum.load()
    dt, esz, code = ((torch.float32, 4, _native.FEDAGG_F32) if kind == "f32"
                     else (torch.bfloat16, 2, _native.FEDAGG_BF16))
    ld = -(-M // 128) * 128
    gen = torch.Generator(device="cuda").manual_seed(K + M % 1000)
    rows = torch.empty((K, ld), dtype=dt, device="cuda")
    for k in range(K):  # row by row: no temporary of the whole bucket
        rows[k] = torch.randn(ld, device="cuda", generator=gen).to(dt)
    out = torch.empty(ld, dtype=torch.float32, device="cuda")
    nws = _native_krum.ws_bytes(K, M)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    G = torch.empty(K * K, dtype=torch.float64, device="cuda")
    w = np.random.default_rng(K).integers(100, 10000, K).astype(np.float64)
    h_w = (ctypes.c_float * K)(*[float(v) for v in (w / w.sum()).astype(np.float32)])
    idx = (ctypes.c_uint64 * 1)(0)
    rp = _native.ptr_array([rows.data_ptr() + k * ld * esz for k in range(K)])
    stream = int(torch.cuda.current_stream().cuda_stream)
    fedavg = lib.fedagg_fedavg_f32 if kind == "f32" else lib.fedagg_fedavg_bf16

    def run_fedavg():
        assert fedavg(rp, h_w, K, M, idx, 0, None, out.data_ptr(), stream) == 0

    def run_robust():
        assert rb.fedagg_robust_mean(rp, code, K, 0, M, out.data_ptr(), stream) == 0

    def run_gram():
        assert kr.fedagg_krum_gram(rp, code, K, M, ws.data_ptr(), nws, G.data_ptr(), stream) == 0

    t = _alternate({"fedavg": run_fedavg, "robust_t0": run_robust, "gram": run_gram}, windows, target_s, torch)
    nb = -(-K // 16)
    flops = 2 * 256 * (nb * (nb + 1) // 2) * M
    res = {"row": row, "K": K, "M": M, "kind": kind, "windows": windows, "ws_bytes": nws,
           "fedavg": _stat(t["fedavg"], esz * K * M + 4 * M), "robust_t0": _stat(t["robust_t0"], esz * K * M + 4 * M),
           "gram": _stat(t["gram"], esz * K * M)}
    g = res["gram"]
    g["flops"] = flops
    g["of_mfma"] = round(flops / (g["ms"] * 1e-3) / (mfma_tflops * 1e12), 3)
    res["over_fedavg"] = round(g["ms"] / res["fedavg"]["ms"], 3)
    res["bound"] = "MFMA" if g["of_mfma"] > g["of_8TBps"] else "memory"
    del rows, out, ws
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", nargs="*", default=list(ROWS))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--target-s", type=float, default=0.3, help="seconds one timed window should last")
    ap.add_argument("--mfma-tflops", type=float, default=78.6, help="the fp64 matrix rate the shares are taken of")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file (relative to the repository)")
    a = ap.parse_args()
    for row in a.rows:
        try:
            res = _row(row, a.windows, a.target_s, a.mfma_tflops)
        except RuntimeError as e:  # a shape that does not fit this GPU: said, not skipped
            res = {"row": row, "not_run": str(e).splitlines()[0][:200]}
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
