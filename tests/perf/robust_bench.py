"""``fedagg_robust_mean`` at ``t = 0``, ``t = floor(0.1 K)`` and the median next to ``fedagg_fedavg_f32``
/ ``fedagg_fedavg_bf16`` on the same device-resident rows, in ONE process, alternated window by
window (``_alternate`` / ``_stat`` of ``mxfp4_bench.py``: the median of the windows, the range kept
beside it).  Not ``bench.py``.

Both kernels must move the same bytes, ``esz K M + 4 M``; ``over_fedavg`` is the robust median time
over the FedAvg median time.  ``bound`` calls a row memory-bound when the robust kernel stays within
1.25 x of the FedAvg kernel, which streams the same rows at HBM rate, and VALU-bound beyond (the
sorting network is all the difference between the two).  One JSON line per row, appended to
``--out`` when given; a row that cannot be run is reported with its reason in place of figures.

    python3 tests/perf/robust_bench.py --out profiles/robust_bench.jsonl
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


def _row(row: str, windows: int, target_s: float) -> dict:
    import numpy as np
    import torch

    from substrafl_amd import _native, _native_robust

    K, M, kind = row.split("x")
    K, M = int(K), int(M)
    lib, rb = _native.load(), _native_robust.load()
    dt, esz, code = ((torch.float32, 4, _native.FEDAGG_F32) if kind == "f32"
                     else (torch.bfloat16, 2, _native.FEDAGG_BF16))
    ld = -(-M // 128) * 128
    gen = torch.Generator(device="cuda").manual_seed(K + M % 1000)
    rows = torch.empty((K, ld), dtype=dt, device="cuda")
    for k in range(K):  # row by row: no temporary of the whole bucket
        rows[k] = torch.randn(ld, device="cuda", generator=gen).to(dt)
    out = torch.empty(ld, dtype=torch.float32, device="cuda")
    w = np.random.default_rng(K).integers(100, 10000, K).astype(np.float64)
    h_w = (ctypes.c_float * K)(*[float(v) for v in (w / w.sum()).astype(np.float32)])
    idx = (ctypes.c_uint64 * 1)(0)
    rp = _native.ptr_array([rows.data_ptr() + k * ld * esz for k in range(K)])
    stream = int(torch.cuda.current_stream().cuda_stream)
    fedavg = lib.fedagg_fedavg_f32 if kind == "f32" else lib.fedagg_fedavg_bf16

    def run_fedavg():
        assert fedavg(rp, h_w, K, M, idx, 0, None, out.data_ptr(), stream) == 0

    def robust(t):
        def run():
            assert rb.fedagg_robust_mean(rp, code, K, t, M, out.data_ptr(), stream) == 0
        return run

    ts = {"t0": 0, "t10pct": K // 10, "median": (K - 1) // 2}
    t = _alternate({"fedavg": run_fedavg, **{n: robust(v) for n, v in ts.items()}}, windows, target_s, torch)
    nbytes = esz * K * M + 4 * M
    res = {"row": row, "K": K, "M": M, "kind": kind, "windows": windows, "t": ts,
           **{n: _stat(ms, nbytes) for n, ms in t.items()}}
    res["over_fedavg"] = {n: round(res[n]["ms"] / res["fedavg"]["ms"], 3) for n in ts}
    res["bound"] = "memory" if max(res["over_fedavg"].values()) <= 1.25 else "VALU"
    del rows, out
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", nargs="*", default=list(ROWS))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--target-s", type=float, default=0.3, help="seconds one timed window should last")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file (relative to the repository)")
    a = ap.parse_args()
    for row in a.rows:
        try:
            res = _row(row, a.windows, a.target_s)
        except RuntimeError as e:  # a shape that does not fit this GPU: said, not skipped
            res = {"row": row, "not_run": str(e).splitlines()[0][:200]}
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
