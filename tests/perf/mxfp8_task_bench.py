#!/usr/bin/env python3
"""Subprocess-mode aggregate task over MXFP8 pickles next to fp32 flat-wire pickles, same run (the
shape of ``task_probe.py``): a FRESH Python process per task that unpickles K shared-state files,
runs ``FedAvg.avg_shared_states`` on the engine and pickles the result.

  parent: writes the K client updates once in both forms -- fp32 ``wire.BucketArray`` layers, and
          the same values as MXFP8 (``wire.float32_to_mxfp8``, packed into one bucket per client) --
          then runs ``--reps`` fresh children per form, alternated, and prints one JSON line per
          form: the children's wall times (measured by the parent), the phases a child reports and
          the bytes of the K pickles.
  child:  ``pickle.load`` of the K files, the strategy call, ``pickle.dump`` of the averaged state.

    python3 tests/perf/mxfp8_task_bench.py --out profiles/mxfp8_bench.jsonl
"""

import argparse
import json
import pickle
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))


class _Algo:
    strategies = ["Federated Averaging"]


def child(d: Path, form: str, K: int) -> None:
    t0 = time.perf_counter()
    from substrafl_amd.strategies import FedAvg

    t1 = time.perf_counter()
    states = []
    for k in range(K):
        with open(d / f"{form}_{k}", "rb") as f:
            states.append(pickle.load(f))
    t2 = time.perf_counter()
    avg = FedAvg(algo=_Algo(), device=0).avg_shared_states(shared_states=states, _skip=True)
    t3 = time.perf_counter()
    with open(d / f"out_{form}", "wb") as f:
        pickle.dump(avg, f, protocol=pickle.HIGHEST_PROTOCOL)
    t4 = time.perf_counter()
    print(json.dumps({"import_s": t1 - t0, "load_s": t2 - t1, "aggregate_s": t3 - t2, "dump_s": t4 - t3}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--M", type=int, default=25_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, default=None)
    args = ap.parse_args()
    if args.child:
        return child(Path(args.child[0]), args.child[1], args.K)

    import numpy as np

    from substrafl_amd import wire
    from substrafl_amd.layout import synthetic_state_dict_shapes
    from substrafl_amd.schemas import FedAvgSharedState

    shapes = synthetic_state_dict_shapes(args.M)
    cuts = np.cumsum([0] + [int(np.prod(s)) for s in shapes])
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as tmp:
        d = Path(tmp)
        size = {"fp32": 0, "mxfp8": 0}
        for k in range(args.K):
            flat = (rng.standard_normal(args.M, dtype=np.float32) * np.float32(0.01))
            layers = [flat[a:b].reshape(s) for a, b, s in zip(cuts, cuts[1:], shapes)]
            codes, scales = wire.float32_to_mxfp8(layers)
            forms = {"fp32": wire.bucket_views(flat, shapes), "mxfp8": wire.pack(list(codes) + [scales])}
            for form, pu in forms.items():
                with open(d / f"{form}_{k}", "wb") as f:
                    pickle.dump(FedAvgSharedState(n_samples=100 + k, parameters_update=pu), f,
                                protocol=pickle.HIGHEST_PROTOCOL)
                size[form] += (d / f"{form}_{k}").stat().st_size
        res = {form: {"wall_s": [], "phases": []} for form in size}
        for _ in range(args.reps):
            for form in size:  # alternated
                t0 = time.perf_counter()
                r = subprocess.run([sys.executable, __file__, "--K", str(args.K), "--child", str(d), form],
                                   capture_output=True, text=True, timeout=600)
                wall = time.perf_counter() - t0
                assert r.returncode == 0, r.stderr[-2000:]
                res[form]["wall_s"].append(round(wall, 3))
                res[form]["phases"].append({k: round(v, 3) for k, v in json.loads(r.stdout.strip().splitlines()[-1]).items()})
        for form in size:
            line = json.dumps({"task": f"aggregate {args.K}x{args.M} subprocess", "form": form, "pickle_bytes": size[form],
                               **res[form]})
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
