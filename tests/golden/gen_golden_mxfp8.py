"""Golden vectors for FedAvg over the MXFP8 wire, produced by the REFERENCE itself.

CONTAINER-ONLY, like ``gen_golden.py`` (whose reference import and ``substra`` stubs it uses): it
refuses to run without the reference, never writes bytecode into it, and writes only data:
``golden_mxfp8.npz`` and ``golden_mxfp8_meta.json``.  A case is K clients' MXFP8 updates (codes and
scales as ``wire.float32_to_mxfp8`` encodes random fp32 layers), their ``n_samples`` and what the
reference's own ``FedAvg.avg_shared_states`` (``_skip=True``) returned on the exactly decoded fp32
inputs (``wire.mxfp8_to_float32``) -- the contract of the MXFP8 route.

Archive members per case ``{key}``: ``codes`` uint8 [K, M] (the raveled layers end to end),
``scales`` uint8 [K, ceil(M / 32)], ``n_samples`` int64 [K], ``out`` float32 [M];
``meta["cases"]`` lists the keys and the layer shapes.  Fixed zip timestamps: a second run
reproduces the archive byte for byte.  Run:  python tests/golden/gen_golden_mxfp8.py
"""

from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

sys.dont_write_bytecode = True  # never write into the reference
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parents[1]))
from gen_golden import _import_reference  # noqa: E402
from gen_golden_dtypes import save_npz  # noqa: E402

from substrafl_amd import wire  # noqa: E402

SMALL = [(3, 5), (1,), (1, 1), (11,)]
EDGE = [(1,), (4099,), (1, 1)]  # a whole workgroup step of the kernel, a tail, numel == 1 at both ends
SPAN = [(31,), (1,), (1,), (70,), (1,)]  # numel == 1 layers at flat positions 31, 32 and last


def main():
    FedAvg, _Scaffold, FedAvgSharedState, _ScaffoldSharedState, DummyAlgo = _import_reference()
    fedavg = FedAvg(algo=DummyAlgo())
    meta = {"numpy": np.__version__, "reference": "Substra/substrafl v1.0.0 @ 2024-10-16", "cases": []}
    arrays = {}

    def counts(K, seed):
        return [int(v) for v in np.random.default_rng(seed).integers(1, 5000, K)]

    def add(kind, K, shapes, n_samples, seed):
        key = f"mxfp8_{len(meta['cases']):03d}"
        rng = np.random.default_rng(seed)
        codes, scales, decoded = [], [], []
        for _ in range(K):
            layers = [(rng.standard_normal(s) * 10.0 ** rng.integers(-3, 3)).astype(np.float32) for s in shapes]
            c, s = wire.float32_to_mxfp8(layers)
            decoded.append(wire.mxfp8_to_float32(c, s))
            codes.append(np.concatenate([a["e4m3fn"].reshape(-1) for a in c]))
            scales.append(s["e8m0"])
        states = [FedAvgSharedState(n_samples=n, parameters_update=list(d)) for n, d in zip(n_samples, decoded)]
        res = fedavg.avg_shared_states(shared_states=states, _skip=True).avg_parameters_update
        assert [o.shape for o in res] == [tuple(s) for s in shapes] and all(o.dtype == np.float32 for o in res), key
        assert all(np.isfinite(o).all() for o in res), key
        arrays[f"{key}/codes"] = np.stack(codes)
        arrays[f"{key}/scales"] = np.stack(scales)
        arrays[f"{key}/n_samples"] = np.array(n_samples, dtype=np.int64)
        arrays[f"{key}/out"] = np.concatenate([o.reshape(-1) for o in res])
        meta["cases"].append({"key": key, "kind": kind, "K": K, "shapes": [list(s) for s in shapes]})

    for K in (1, 3, 7, 8, 9, 129, 200):
        add("table", K, SMALL, counts(K, 17 + K), 9000 + K)
    add("edge", 8, EDGE, counts(8, 23), 9100)
    add("span", 5, SPAN, counts(5, 29), 9200)
    add("negative-weight", 4, SMALL, [10, -9, 5, -5], 9300)
    add("huge-counts", 3, SMALL, [2 ** 53 + 1, 2 ** 60 + 12345, 2 ** 53 + 3], 9400)

    save_npz(HERE / "golden_mxfp8.npz", arrays)
    (HERE / "golden_mxfp8_meta.json").write_text(json.dumps(meta, indent=1, sort_keys=True) + "\n")
    size = (HERE / "golden_mxfp8.npz").stat().st_size
    print(f"wrote {len(arrays)} arrays, {len(meta['cases'])} cases, {size / 1e3:.1f} kB")
    assert size < 1 << 20


if __name__ == "__main__":
    main()
