"""The MXFP8 downlink's kernels next to what they replace, device-resident, in ONE process at the
same shapes, alternated window by window (the method and helpers of ``mxfp4_bench.py``).  Not
``bench.py``.

Aggregator, per (K, M) row and input kind: ``fedagg_mxdl_fedavg`` (``fused``) against the existing
fedavg entry followed by ``fedagg_mx_quantize`` (``two_step``) and against the existing fedavg entry
alone (``fedavg``, which leaves an fp32 row nobody has encoded yet).  Algorithmic bytes with
``c`` the code bytes of a row (M for e4m3, M/2 for e2m1): ``K (c + M/32) + M + M/32`` fused,
``K (c + M/32) + 4 M`` alone, ``K (c + M/32) + 9 M + M/32`` two-step.  Client, per M:
``fedagg_mxdl_increment`` over a model's tensors (``9 M + M/32`` bytes) against ``fedagg_mxdl_decode``
into an fp32 bucket followed by ``fedagg_flat_increment`` (``17 M + M/32``).  The bars of each line:
``fused_not_slower_than_fedavg`` (medians within the larger range, or fused below),
``fused_faster_than_two_step`` and ``fused_increment_faster`` (below by more than the larger range).

    python3 tests/perf/mxdl_bench.py --out profiles/mxdl_bench.jsonl
"""

from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

from mxfp4_bench import QUANT, ROWS, _alternate, _stat  # noqa: E402


def _range(*stats) -> float:
    return max(s["ms_range"][1] - s["ms_range"][0] for s in stats)


def _row(row: str, windows: int, target_s: float) -> dict:
    import numpy as np
    import torch

    from substrafl_amd import _native, _native_mx, _native_mx4, _native_mxdl

    K, M = (int(v) for v in row.split("x"))
    mx, mx4, dl = _native_mx.load(), _native_mx4.load(), _native_mxdl.load()
    nb = -(-M // 32)
    ldc, lds = -(-M // 256) * 256, -(-nb // 256) * 256
    gen = torch.Generator(device="cuda").manual_seed(K + M % 1000)
    # one code buffer serves both kinds: finite e4m3 codes are also 2 finite e2m1 codes per byte
    codes = torch.randint(0, 0x7F, (K, ldc), dtype=torch.uint8, device="cuda", generator=gen)
    codes |= torch.randint(0, 2, (K, ldc), dtype=torch.uint8, device="cuda", generator=gen) << 7
    scales = torch.randint(120, 131, (K, lds), dtype=torch.uint8, device="cuda", generator=gen)
    out32 = torch.empty(ldc, dtype=torch.float32, device="cuda")
    q = torch.empty(ldc + lds, dtype=torch.uint8, device="cuda")
    w = (np.random.default_rng(K).integers(100, 10000, K)).astype(np.float64)
    h_w = (ctypes.c_float * K)(*[float(v) for v in (w / w.sum()).astype(np.float32)])
    idx = (ctypes.c_uint64 * 1)(0)
    cp = _native.ptr_array([codes.data_ptr() + k * ldc for k in range(K)])
    sp = _native.ptr_array([scales.data_ptr() + k * lds for k in range(K)])
    stream = int(torch.cuda.current_stream().cuda_stream)
    res = {"row": row, "K": K, "M": M, "windows": windows}
    for name, kind, entry, c in (("e4m3", _native_mxdl.E4M3, mx.fedagg_mx_fedavg_e4m3, M),
                                 ("e2m1", _native_mxdl.E2M1, mx4.fedagg_mx4_fedavg_e2m1, -(-M // 2))):
        def fedavg():
            assert entry(cp, sp, h_w, K, M, idx, 0, out32.data_ptr(), stream) == 0

        def two_step():
            fedavg()
            assert mx.fedagg_mx_quantize(out32.data_ptr(), _native.FEDAGG_F32, M, q.data_ptr(), q.data_ptr() + ldc,
                                         stream) == 0

        def fused():
            assert dl.fedagg_mxdl_fedavg(kind, cp, sp, h_w, K, M, idx, 0, q.data_ptr(), q.data_ptr() + ldc, stream) == 0

        t = _alternate({"fused": fused, "two_step": two_step, "fedavg": fedavg}, windows, target_s, torch)
        rows = K * (c + nb)
        r = {"fused": _stat(t["fused"], rows + M + nb), "two_step": _stat(t["two_step"], rows + 9 * M + nb),
             "fedavg": _stat(t["fedavg"], rows + 4 * M)}
        r["fused_not_slower_than_fedavg"] = bool(r["fused"]["ms"] - r["fedavg"]["ms"] <= _range(r["fused"], r["fedavg"]))
        r["fused_faster_than_two_step"] = bool(r["two_step"]["ms"] - r["fused"]["ms"] > _range(r["fused"], r["two_step"]))
        res[name] = r
    del codes, scales, out32, q
    torch.cuda.empty_cache()
    return res


def _client(M: int, windows: int, target_s: float) -> dict:
    import torch

    from substrafl_amd import _native, _native_mxdl
    from substrafl_amd.layout import synthetic_state_dict_shapes

    lib, dl = _native.load(), _native_mxdl.load()
    nb = -(-M // 32)
    numels = [int(torch.Size(s).numel()) for s in synthetic_state_dict_shapes(M)]  # bench.py's model
    model = torch.zeros(M, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(M % 1000)
    upd = torch.randint(0, 0x7F, (M + nb,), dtype=torch.uint8, device="cuda", generator=gen)
    upd[M:] = 120
    bucket = torch.empty(M, device="cuda")
    offs = [0]
    for n in numels:
        offs.append(offs[-1] + n)
    ptrs = _native.ptr_array([model.data_ptr() + 4 * o for o in offs[:-1]])
    n_arr = (ctypes.c_uint64 * len(numels))(*numels)
    stream = int(torch.cuda.current_stream().cuda_stream)

    def fused():
        assert dl.fedagg_mxdl_increment(ptrs, n_arr, len(numels), upd.data_ptr(), upd.data_ptr() + M, M, 0.5, stream) == 0

    def two_step():
        assert dl.fedagg_mxdl_decode(upd.data_ptr(), upd.data_ptr() + M, M, bucket.data_ptr(), stream) == 0
        assert lib.fedagg_flat_increment(ptrs, n_arr, len(numels), bucket.data_ptr(), _native.FEDAGG_F32, 0.5, stream) == 0

    t = _alternate({"fused": fused, "two_step": two_step}, windows, target_s, torch)
    res = {"client_M": M, "tensors": len(numels), "windows": windows,
           "fused": _stat(t["fused"], 9 * M + nb), "two_step": _stat(t["two_step"], 17 * M + nb)}
    res["fused_increment_faster"] = bool(res["two_step"]["ms"] - res["fused"]["ms"] > _range(res["fused"], res["two_step"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", nargs="*", default=list(ROWS))
    ap.add_argument("--client", nargs="*", type=int, default=list(QUANT))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-seconds", type=float, default=0.4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "mxdl_bench.py needs an MI355X: a time measured elsewhere says nothing"
    jobs = [lambda r=r: _row(r, args.windows, args.window_seconds) for r in args.rows]
    jobs += [lambda m=m: _client(m, args.windows, args.window_seconds) for m in args.client]
    for job in jobs:  # written row by row: a run that is cut short keeps what it measured
        line = json.dumps(job())
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
