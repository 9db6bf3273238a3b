"""fp16 plumbing fixtures: every aggregation of ``gen_plumbing.py``'s 2-org linear FedAvg and
Scaffold simulations with the model and the data in float16, captured from the REFERENCE.

CONTAINER-ONLY (``gen_plumbing.harness`` imports the reference and refuses to run without it).
What the calls pin is the 16-bit Scaffold contract of DESIGN.md §2: round 1 ships
(parameters_update, control_variate_update, server_control_variate) as (fp16, fp16, fp16), from
round 2 on the control variates come back as the float64 the aggregation returned, (fp16, fp64,
fp64); every output is float64 (Scaffold) or float16 (FedAvg).  ``kinds`` of every call is in the
meta.  Also recorded: a small fp16 CNN with BatchNorm running statistics when CPU torch trains it
(else the reason), the error a bfloat16 model raises in the reference, and each run's final
performance -- recorded, not a known answer.  Writes ``golden_plumbing_half.npz`` (fixed zip
timestamps: a second run reproduces it byte for byte) and ``golden_plumbing_half_meta.json``.  Run:
    python tests/golden/gen_plumbing_half.py
"""

from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

sys.dont_write_bytecode = True  # never write into the reference
sys.path.insert(0, str(Path(__file__).resolve().parent))
from gen_golden_dtypes import NAN_SHARE_CAP, nan_share, save_npz  # noqa: E402
from gen_plumbing import harness, linear_setup, small_cnn  # noqa: E402

OUT = Path(__file__).resolve().parent


def main():
    import torch

    h = harness(dtype=torch.float16)
    train, test, split, Perceptron = linear_setup(torch)
    tr, te = [split(d) for d in train], split(test)
    mse = torch.nn.MSELoss()
    torch.manual_seed(42)
    h.run("linear_fedavg_f16", h.RecFedAvg, h.TorchFedAvgAlgo, Perceptron().half(), mse, tr, te, h.mae_score, rounds=3)
    torch.manual_seed(42)
    h.run("linear_scaffold_f16", h.RecScaffold, h.TorchScaffoldAlgo, Perceptron().half(), mse, tr, te, h.mae_score,
          rounds=3)

    # a small fp16 model with BatchNorm running statistics, if CPU torch trains it
    g = np.random.default_rng(2024)
    mk = lambda n: (g.standard_normal((n, 1, 28, 28)).astype(np.float32), g.integers(0, 10, n))  # noqa: E731
    try:
        torch.manual_seed(7)
        h.run("cnn_fedavg_f16", h.RecFedAvg, h.TorchFedAvgAlgo, small_cnn(torch)().half(), torch.nn.CrossEntropyLoss(),
              [mk(64), mk(48)], mk(32), h.acc_score, rounds=2, lr=0.05, updates=4, batch=16,
              algo_kwargs={"with_batch_norm_parameters": True})
        h.meta["cnn_fedavg_f16"] = "recorded"
    except Exception as e:  # noqa: BLE001 - the reason is the recorded result
        h.meta["cnn_fedavg_f16"] = f"left out: CPU torch does not train it ({type(e).__name__}: {e})"[:300]
        h.meta["configs"].pop("cnn_fedavg_f16", None)
        for k in [k for k in h.arrays if k.startswith("cnn_fedavg_f16/")]:
            del h.arrays[k]

    # a bfloat16 model: the reference has no NumPy form for it
    n_arrays = len(h.arrays)
    h.cfg["dtype"] = torch.bfloat16
    try:
        torch.manual_seed(42)
        h.run("linear_fedavg_bf16", h.RecFedAvg, h.TorchFedAvgAlgo, Perceptron().bfloat16(), mse, tr, te, h.mae_score,
              rounds=1)
        h.meta["bf16_model_error"] = None
    except Exception as e:  # noqa: BLE001
        h.meta["bf16_model_error"] = type(e).__name__
        h.meta["bf16_model_error_message"] = str(e)[:200]
    h.meta["configs"].pop("linear_fedavg_bf16", None)
    assert len(h.arrays) == n_arrays, "the bfloat16 run recorded an aggregation"

    # self-checks: the linear runs stay finite; any other run keeps its NaN share under the cap
    for name, cfg in h.meta["configs"].items():
        outs = [h.arrays[k] for k in h.arrays if k.startswith(name + "/") and "/out_" in k]
        cfg["nan_share"] = nan_share(outs)
        if name.startswith("linear"):
            assert all(np.isfinite(o).all() for o in outs), name
        assert cfg["nan_share"] <= NAN_SHARE_CAP, (name, cfg["nan_share"])
    save_npz(OUT / "golden_plumbing_half.npz", h.arrays)
    (OUT / "golden_plumbing_half_meta.json").write_text(json.dumps(h.meta, indent=1, sort_keys=True) + "\n")
    raw = sum(a.nbytes for a in h.arrays.values())
    size = (OUT / "golden_plumbing_half.npz").stat().st_size
    print(f"wrote {len(h.arrays)} arrays: {raw / 1e6:.3f} MB raw, {size / 1e6:.3f} MB compressed; "
          f"bf16 model: {h.meta['bf16_model_error']}; cnn: {h.meta['cnn_fedavg_f16']}")
    assert size <= min(1 << 20, (OUT / "golden_aggregation.npz").stat().st_size)


if __name__ == "__main__":
    main()
