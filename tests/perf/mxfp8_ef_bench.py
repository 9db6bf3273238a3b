"""``fedagg_mxef_quantize`` (the fused error-feedback quantiser) next to ``fedagg_mx_quantize`` (the
plain one) and a device-to-device ``copy_`` of the fused kernel's byte count, device-resident, in
ONE process, alternated window by window.  Not ``bench.py``.

Per size and kind: every candidate is warmed at the shape, then ``--windows`` windows per candidate
are timed alternately (fused, plain, copy, fused, ...) with device events around enough back-to-back
launches that a window lasts a good fraction of a second; the figure is the median window and the
range over the windows is kept beside it.  Algorithmic bytes, computed from the shape:
``(esz + 4 + 4 + 1) M + ceil(M / 32)`` for the fused kernel (13.03 M for fp32, 11.03 M for bf16),
``(esz + 1) M + ceil(M / 32)`` for the plain one; the copy reads and writes half of the fused
kernel's count each, so its bytes per second are what a kernel of that traffic can reach on the
machine.  ``--round``: one round-level figure, the ``train`` of a 25M-parameter
``accelerate_algo(TorchFedAvgAlgo, wire="mxfp8")`` client with and without ``error_feedback``
(host clock around calls that end in the export's device synchronise).  One JSON line per row,
appended to ``--out`` when given.

    python3 tests/perf/mxfp8_ef_bench.py --round --out profiles/mxef_bench.jsonl
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HBM_PEAK = 8.0e12
SIZES = (25_000_000, 125_000_000, 350_000_000)


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
    return {"ms": round(med, 4), "ms_range": [round(min(ms), 4), round(max(ms), 4)], "bytes": nbytes,
            "TBps": round(nbytes / med / 1e9, 3), "of_8TBps": round(nbytes / (med * 1e-3) / HBM_PEAK, 3)}


def _size(M: int, windows: int, target_s: float) -> dict:
    import torch

    from substrafl_amd import _native, _native_mx, _native_mxef

    mx, ef = _native_mx.load(), _native_mxef.load()
    nb = -(-M // 32)
    x32 = torch.randn(M, device="cuda") * 0.01
    res = torch.zeros(M, device="cuda")  # the kernel's own residual from the warm-up on: a steady state
    dst = torch.empty(M + 15 + nb, dtype=torch.uint8, device="cuda")
    d_scales = dst.data_ptr() + (M + 15) // 16 * 16  # 16-B aligned, as a caller who can choose would place it
    stream = int(torch.cuda.current_stream().cuda_stream)
    row = {"M": M, "windows": windows}
    for name, kind, src in (("f32", _native.FEDAGG_F32, x32), ("bf16", _native.FEDAGG_BF16, x32.to(torch.bfloat16))):
        esz = src.element_size()
        fused_bytes = (esz + 9) * M + nb
        half = torch.empty(fused_bytes // 2, dtype=torch.uint8, device="cuda")
        half2 = torch.empty_like(half)

        def fused():
            assert ef.fedagg_mxef_quantize(src.data_ptr(), kind, M, res.data_ptr(), dst.data_ptr(), d_scales, stream) == 0

        def plain():
            assert mx.fedagg_mx_quantize(src.data_ptr(), kind, M, dst.data_ptr(), d_scales, stream) == 0

        def copy():
            half2.copy_(half)

        cands = {"fused": (fused, fused_bytes), "plain": (plain, (esz + 1) * M + nb), "copy": (copy, 2 * half.numel())}
        steps = {}
        for key, (fn, _) in cands.items():  # warm-up at this shape: code objects, clocks
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            steps[key] = max(3, min(20000, int(target_s * 1e3 / _window(fn, 2, torch))))
        t = {key: [] for key in cands}
        for _ in range(windows):  # alternated: every candidate sees the same machine
            for key, (fn, _) in cands.items():
                t[key].append(_window(fn, steps[key], torch))
        r = {key: _stat(t[key], nbytes) for key, (_, nbytes) in cands.items()}
        r["fused_over_copy_rate"] = round(r["fused"]["TBps"] / r["copy"]["TBps"], 3)
        r["fused_over_plain_time"] = round(r["fused"]["ms"] / r["plain"]["ms"], 3)
        r["steps_per_window"] = steps
        row[name] = r
        del half, half2
    return row


def _round(params: int, rounds: int) -> dict:
    """``train`` of a client whose model holds ``params`` parameters (one Linear layer), one
    optimizer step per round, with and without error feedback, alternated."""
    import numpy as np
    import torch
    from standin_substrafl.algorithms.pytorch import TorchFedAvgAlgo
    from standin_substrafl.index_generator import NpIndexGenerator

    from substrafl_amd.integration import accelerate_algo

    width = 5000
    rows = params // width

    class XY(torch.utils.data.Dataset):
        def __init__(self, data_from_opener, is_inference=False):
            self.x, self.y = data_from_opener

        def __getitem__(self, i):
            return torch.from_numpy(self.x[i]), torch.from_numpy(self.y[i])

        def __len__(self):
            return len(self.x)

    def algo(ef):
        torch.manual_seed(3)
        model = torch.nn.Linear(width, rows, bias=False)

        class MyAlgo(TorchFedAvgAlgo):
            def __init__(self):
                super().__init__(model=model, criterion=torch.nn.MSELoss(), optimizer=torch.optim.SGD(model.parameters(), lr=0.01),
                                 index_generator=NpIndexGenerator(batch_size=8, num_updates=1, seed=1), dataset=XY,
                                 disable_gpu=False)

        return accelerate_algo(MyAlgo, wire="mxfp8", error_feedback=ef)()

    rng = np.random.default_rng(0)
    data = (rng.standard_normal((16, width)).astype(np.float32), rng.standard_normal((16, rows)).astype(np.float32))
    algos, t = {"plain": algo(False), "error_feedback": algo(True)}, {"plain": [], "error_feedback": []}
    avg = None
    for rnd in range(rounds + 1):  # round 0 warms both up
        for key, a in algos.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = a.train(data_from_opener=data, shared_state=avg, _skip=True)
            torch.cuda.synchronize()
            if rnd:
                t[key].append((time.perf_counter() - t0) * 1e3)
        avg = type("Avg", (), {"avg_parameters_update": [np.zeros((rows, width), np.float32)]})()
        del st
    out = {"round_params": rows * width, "rounds": rounds}
    for key, ms in t.items():
        out[key] = {"train_ms": round(statistics.median(ms), 3), "train_ms_range": [round(min(ms), 3), round(max(ms), 3)]}
    out["error_feedback_over_plain"] = round(out["error_feedback"]["train_ms"] / out["plain"]["train_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", type=int, default=list(SIZES))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-seconds", type=float, default=0.4)
    ap.add_argument("--round", action="store_true", help="also time a 25M-parameter client's train")
    ap.add_argument("--round-params", type=int, default=25_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "mxfp8_ef_bench.py needs an MI355X: a time measured elsewhere says nothing"
    jobs = [lambda m=m: _size(m, args.windows, args.window_seconds) for m in args.sizes]
    if args.round:
        jobs.append(lambda: _round(args.round_params, 7))
    for job in jobs:  # written row by row: a run that is cut short keeps what it measured
        line = json.dumps(job())
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
