"""bench.py's multi-rank contract on CPU: ``python3 bench.py --gpus N`` (no torchrun) starts N rank
processes itself and the line reports ``"n_gpus": N``; a WORLD_SIZE that disagrees with --gpus
exits non-zero.  ``--rehearse-cpu`` runs the launcher / rank / barrier / max-over-ranks plumbing
with no GPU and reports no value (the driver's plain command must not silently run
one rank)."""

import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], capture_output=True, text=True, env=env,
                          timeout=240, cwd=str(ROOT))


def _line(stdout):
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, stdout
    return json.loads(lines[0])


CLIENT_SHARD_FIELDS = ("combine", "scaling", "clients", "clients_per_gpu", "params", "layout", "steps", "ms_per_step",
                       "GBps", "frac_of_n_x_hbm_peak", "block_kernel_ms", "exchange_and_tail_ms", "single_gpu_ms",
                       "weak_efficiency", "bit_exact_by_construction", "schedule", "parity")


def test_gpus_2_without_full_runs_no_leg():
    """Without --full the N > 1 command is the parameter-range line alone: two ranks, no leg."""
    r = _run(["--gpus", "2", "--rehearse-cpu", "--steps", "3", "--warmup", "1"])
    assert r.returncode == 0, r.stderr[-3000:]
    line = _line(r.stdout)
    assert line["n_gpus"] == 2 and line["ranks_seen"] == 2 and line["steps"] == 3 and line["ms_per_step"] > 0
    assert 0 < line["process_group"]["timeout_s"] <= 600
    assert not {"client_shard", "legs_order", "param_range_strong_gather"} & set(line)


def test_plain_gpus_2_launches_two_ranks():
    """The N > 1 command with --full: one line with the parameter-range fields AND the client-shard leg
    (the north-star mode: lockstep schedule over one communicator, here gloo on a tiny problem),
    and a process group with a finite timeout."""
    r = _run(["--full", "--gpus", "2", "--rehearse-cpu", "--steps", "3", "--warmup", "1"])
    assert r.returncode == 0, r.stderr[-3000:]
    line = _line(r.stdout)
    assert line["n_gpus"] == 2 and line["ranks_seen"] == 2 and line["rehearsal"] is True
    assert line["value"] is None  # a rehearsal is never a measurement
    assert 0 < line["process_group"]["timeout_s"] <= 600
    cs = line["client_shard"]
    assert all(k in cs for k in CLIENT_SHARD_FIELDS)
    assert cs["combine"] == "striped" and cs["scaling"] == "weak" and cs["bit_exact_by_construction"]
    assert cs["parity"]["mismatches"] == 0 and cs["schedule"]["steps"] == 4
    probe = cs["xgmi_p2p"]  # the link-rate probe the N > 1 GPU line carries (here over gloo)
    assert probe["ring"]["GBps_per_direction"] > 0 and probe["all_peers"]["peers"] == 1
    # VERDICT r03 "make the N > 1 line self-validating and its headline honest":
    # the parameter-range value is labelled per GPU ...
    assert line["config"]["workload"] == "fedavg_fp32_64x125M_per_gpu"
    # ... the decisive legs run first ...
    assert line["legs_order"][:3] == ["client_shard_push", "client_shard", "param_range_strong_gather"]
    # ... the client-shard output is compared in full against a second, independent path ...
    fc = cs["full_compare"]
    assert fc["elements"] == cs["params"] and fc["mismatches"] == 0 and "native RCCL" in fc["against"]
    assert "late_landing_tags" in cs and cs["rccl_comm_count"] == 2
    assert cs["checksum_comparable"] and len(cs["output_checksum"]) == 2
    assert line["client_shard_output_checksums"] == {"legs": ["client_shard"], "agree": None}  # one leg: no claim
    # ... and C3 as written (M split over the ranks, result gathered to rank 0) is its own leg
    g = line["param_range_strong_gather"]
    assert g["scaling"] == "strong" and g["params_per_gpu"] * 2 >= g["params"]
    assert g["parity"] == {"mismatches": 0, "gathered_slice_checksum_mismatches": 0}
    for k in ("ms_per_step", "GBps", "kernel_ms", "gather_ms", "speedup", "strong_efficiency"):
        assert k in g
    # its pipelined variant gathers chunk by chunk into views of the same buffer: the same result
    assert g["pipelined"]["chunks"] > 1 and g["pipelined"]["mismatches_vs_whole_gather"] == 0


def test_single_gpu_line_keeps_its_workload_name():
    """N = 1: the line is the workload itself (no per-GPU suffix, no legs)."""
    r = _run(["--rehearse-cpu", "--steps", "2", "--warmup", "0"])
    assert r.returncode == 0, r.stderr[-3000:]
    line = _line(r.stdout)
    assert line["config"]["workload"] == "fedavg_fp32_64x125M" and "legs_order" not in line


def test_pg_kwargs_has_a_timeout():
    """Every multi-rank process group the bench creates (RCCL or gloo) has a finite timeout."""
    sys.path.insert(0, str(ROOT))
    import bench

    t = bench.pg_kwargs()["timeout"].total_seconds()
    assert 0 < t <= 600 and bench.CLIENT_SHARD_DEADLINE_S < t and bench.MULTI_DEVICE_DEADLINE_S < t


def test_line_budget_bounds_the_legs(monkeypatch):
    """The N > 1 line finishes under the driver's 600 s limit whatever its legs do: every leg's
    deadline fits in what is left of LINE_BUDGET_S after the legs behind it, and a leg with less
    than LEG_MIN_S left is skipped (deadline 0), not started."""
    import time

    sys.path.insert(0, str(ROOT))
    import bench

    assert bench.LINE_BUDGET_S + bench.PG_TIMEOUT_S / 10 < 600
    monkeypatch.setattr(bench, "_T_START", time.monotonic())
    d = bench.leg_deadline(bench.CLIENT_SHARD_DEADLINE_S, 100)
    assert d == bench.CLIENT_SHARD_DEADLINE_S
    monkeypatch.setattr(bench, "_T_START", time.monotonic() - (bench.LINE_BUDGET_S - 200))
    d = bench.leg_deadline(bench.CLIENT_SHARD_DEADLINE_S, 100)
    assert 95 <= d <= 100  # 200 s left, 100 kept for what follows
    monkeypatch.setattr(bench, "_T_START", time.monotonic() - (bench.LINE_BUDGET_S - 60))
    assert bench.leg_deadline(bench.CLIENT_SHARD_DEADLINE_S, 30) == 0.0  # 30 s < LEG_MIN_S: skipped


def test_default_rounds_follow_the_executor():
    """Three rounds for the native executor over >= 2 ranks, else one; --rounds overrides both."""
    import argparse

    sys.path.insert(0, str(ROOT))
    import bench
    from substrafl_amd import lockstep, sharding

    ns = argparse.Namespace
    assert bench._rounds(ns(rounds="", executor="native", gpus=8)) == lockstep.NATIVE_ROUNDS == (0.5, 0.3, 0.2)
    assert bench._rounds(ns(rounds="", executor="native", gpus=1)) == lockstep.DEFAULT_ROUNDS == (1.0,)
    assert bench._rounds(ns(rounds="", executor="torch", gpus=8)) == lockstep.DEFAULT_ROUNDS
    assert bench._rounds(ns(rounds="0.75,0.25", executor="native", gpus=8)) == (0.75, 0.25)
    assert sharding.default_rounds(type("T", (), {"native": True, "world": 4})()) == lockstep.NATIVE_ROUNDS
    assert sharding.default_rounds(type("T", (), {"native": True, "world": 1})()) == lockstep.DEFAULT_ROUNDS
    assert sharding.default_rounds(object()) == lockstep.DEFAULT_ROUNDS


def test_plain_gpus_3_launches_three_ranks():
    r = _run(["--full", "--gpus", "3", "--rehearse-cpu", "--steps", "2", "--warmup", "0", "--combine", "relay"])
    assert r.returncode == 0, r.stderr[-3000:]
    line = _line(r.stdout)
    assert line["n_gpus"] == 3 and line["client_shard"]["combine"] == "relay"
    assert line["client_shard"]["parity"]["mismatches"] == 0


def test_world_size_mismatch_is_an_error():
    r = _run(["--gpus", "2", "--rehearse-cpu"], {"WORLD_SIZE": "3", "RANK": "0"})
    assert r.returncode == 2
    assert "refusing" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_single_rank_default():
    r = _run(["--rehearse-cpu", "--steps", "2", "--warmup", "0"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert _line(r.stdout)["n_gpus"] == 1


def test_cpu_threaded_variant_is_labelled():
    """The optional multi-core CPU figure is labelled as not the reference and
    splits the layers into chunks of >= 2 elements (numel == 1 layers whole)."""
    import numpy as np

    sys.path.insert(0, str(ROOT))
    import bench

    rng = np.random.default_rng(0)
    shapes = [(1,), (7,), (3, 5), (1000,), (1, 1)]
    pus = [[rng.standard_normal(s).astype(np.float32) for s in shapes] for _ in range(5)]
    from oracle import fedavg_reference_structure

    res = bench._cpu_threaded(fedavg_reference_structure, pus, [3, 1, 4, 1, 5], 10**9, 3)  # nominal bytes: value > 0 at any speed
    assert "not the reference" in res["kind"] and 1 <= res["cores"] <= 3 and res["value"] > 0


def test_client_shard_block_data_is_element_addressed():
    """The client-shard legs' row buffers hold a hash of (client, element) wherever a plan puts the
    element, so two plans (round splits, executors) hold the same values and their outputs are
    comparable bit for bit (bench._synth_block_elems, the legs' output checksums)."""
    import numpy as np
    import torch

    sys.path.insert(0, str(ROOT))
    import bench
    from substrafl_amd.sharding import client_blocks, striped_plan

    M, G, K = 40_000, 4, 12
    seen = []
    for rounds in ((1.0,), (0.5, 0.3, 0.2)):
        vals = np.full((K, M), np.nan, np.float32)
        for r in range(G):
            plan = striped_plan(M, G, r, None, rounds)
            for b, segs in plan.blocks.items():
                k0, k1 = client_blocks(K, G)[b]
                t = bench._synth_block_elems(torch, "f32", k0, k1 - k0, plan.block_len[b], segs, torch.device("cpu"))
                for lo, hi, col in segs:
                    vals[k0:k1, lo:hi] = t[:, col: col + hi - lo].numpy()
        assert not np.isnan(vals).any() and np.abs(vals).max() <= 1.0
        seen.append(vals)
    assert np.array_equal(seen[0].view(np.uint32), seen[1].view(np.uint32))
    out = torch.from_numpy(seen[0][0].copy())
    assert bench._output_checksum(torch, out, M) == bench._output_checksum(torch, out.clone(), M)


def test_tiled_client_shard_blocks_hold_the_row_values():
    """VERDICT r04 "Next 3": a tiled leg's blocks hold the same (client, element) values as the row
    legs (bench._synth_tiled_elems == TiledBlock.from_rows of bench._synth_block_elems), so the
    tiled legs' output checksums compare with the row legs'."""
    import torch

    sys.path.insert(0, str(ROOT))
    import bench
    from substrafl_amd.sharding import TiledBlock, client_blocks, striped_plan

    M, G, K = 50_003, 3, 7
    for kind, tv in (("f32", 64), ("bf16", 32)):
        for r in range(G):
            plan = striped_plan(M, G, r, None, (0.5, 0.5))
            for b, segs in plan.blocks.items():
                k0, k1 = client_blocks(K, G)[b]
                ext = TiledBlock.run_extents(plan, b)
                rows = bench._synth_block_elems(torch, kind, k0, k1 - k0, plan.block_len[b], segs, torch.device("cpu"))
                ref = TiledBlock.from_rows(torch, kind, rows, tv, ext)
                got = bench._synth_tiled_elems(torch, kind, k0, k1 - k0, plan.block_len[b], segs, tv, ext,
                                               torch.device("cpu"))
                assert sorted(ref.buckets) == sorted(got.buckets)
                for c0 in ref.buckets:
                    assert torch.equal(ref.buckets[c0][0], got.buckets[c0][0]), (kind, r, b, c0)


LEG_FIELDS = ("combine", "scaling", "clients", "params", "ms_per_step", "parity", "full_compare", "output_checksum")


import pytest  # noqa: E402


@pytest.mark.parametrize("phase,expect", [("connect", "did not connect"), ("timed", "did not finish within")])
def test_a_hanging_leg_keeps_the_legs_before_it(phase, expect):
    """VERDICT r04 "Next 6": the N > 1 line's legs run as child processes; a third leg that hangs
    (in its set-up / RCCL connect, or in its timed steps) is killed at its own deadline, the line
    still carries the first two legs' fields, the legs after it still run, and the line exits 0
    within its budget.  (--rehearse-legs: the real leg mechanism over gloo, 2 ranks.)"""
    import time

    budget = 150
    env = {"BENCH_LINE_BUDGET_S": str(budget), "BENCH_LEG_MIN_S": "10", "BENCH_LEG_DEADLINE_S": "40",
           "BENCH_LEG_CONNECT_S": "10", "BENCH_REHEARSE_HANG": f"param_range_strong_gather:{phase}"}
    t0 = time.monotonic()
    r = _run(["--gpus", "2", "--rehearse-cpu", "--rehearse-legs", "--multi-device-leg", "off", "--steps", "2",
              "--warmup", "1"], env)
    wall = time.monotonic() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    line = _line(r.stdout)
    order = line["legs_order"]
    assert order[:3] == ["client_shard_push", "client_shard", "param_range_strong_gather"]
    for key in order[:2]:  # the legs gathered before the hang keep their results
        assert "error" not in line[key], line[key]
        assert all(k in line[key] for k in LEG_FIELDS), (key, line[key])
        assert line[key]["parity"]["mismatches"] == 0
    hung = line["param_range_strong_gather"]
    assert expect in hung["error"], hung
    assert hung["wall_s"] < (12 if phase == "connect" else 42), hung  # its own deadline, not the line's
    for key in order[3:]:  # the legs after it still ran (or were skipped by the budget, never lost)
        assert key in line and ("ms_per_step" in line[key] or "skipped" in line[key]), (key, line.get(key))
    agree = line["client_shard_output_checksums"]
    assert len(agree["legs"]) >= 2 and agree["agree"] is True
    assert wall < budget


def test_shared_gpu_lines_carry_no_scaling_claim():
    """ranks sharing one GPU report physical_gpus and null aggregate-rate fields."""
    import types

    sys.path.insert(0, str(ROOT))
    import bench

    rec = {"value": 6695.9, "frac_of_n_x_hbm_peak": 0.4, "weak_efficiency": 0.877, "ms_per_step": 11.0}
    bench._label_shared_gpu(types.SimpleNamespace(world=2, physical_gpus=1), rec,
                            ("value", "frac_of_n_x_hbm_peak", "weak_efficiency"))
    assert rec["physical_gpus"] == 1 and "no scaling information" in rec["shared_gpu"]
    assert rec["value"] is None and rec["weak_efficiency"] is None and rec["ms_per_step"] == 11.0
    own = {"value": 1.0}
    bench._label_shared_gpu(types.SimpleNamespace(world=2, physical_gpus=2), own, ("value",))
    assert own == {"value": 1.0}


@pytest.mark.parametrize("n", [4, 8])
def test_rehearsed_n_gpu_line_with_every_leg(n, tmp_path):
    """VERDICT r05 "Next 1": the N = 4 and N = 8 lines as the driver's node will run them, every leg
    on its CPU stand-in (--rehearse-legs: the legs' child processes per rank, their gloo groups,
    connect deadlines and result gathering at 4 / 8 ranks).  The line exits 0 inside
    LINE_BUDGET_S, reports the N, carries the decisive legs' fields with each leg's set-up time
    beside its deadline, and reads through tools/n_gt_1_report.py without a flag."""
    import time

    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tools"))
    import bench
    import n_gt_1_report as rep

    t0 = time.monotonic()
    r = _run(["--gpus", str(n), "--rehearse-cpu", "--rehearse-legs", "--steps", "3", "--warmup", "1"])
    wall = time.monotonic() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    assert wall < bench.LINE_BUDGET_S, wall
    line = _line(r.stdout)
    assert line["n_gpus"] == n and line["ranks_seen"] == n and line["value"] is None
    assert line["legs_order"] == [leg[2] for leg in bench.LEGS]
    for key in ("client_shard_push", "client_shard", "param_range_strong_gather"):
        leg = line[key]
        assert "error" not in leg and "skipped" not in leg, (key, leg)
        assert leg["parity"]["mismatches"] == 0, (key, leg)
        assert leg["connect_s"] is not None and leg["connect_s"] < leg["connect_deadline_s"], (key, leg)
    assert line["client_shard_push"]["full_compare"]["mismatches"] == 0
    assert line["client_shard"]["rccl_comm_count"] == n
    assert line["client_shard_output_checksums"]["agree"] is True
    p = tmp_path / f"line_n{n}.json"
    p.write_text(r.stdout)
    assert rep.main([str(p)]) == 0
    print(f"[N={n} rehearsal] wall {wall:.1f} s, legs' set-up "
          + ", ".join(f"{k} {line[k].get('connect_s')} s" for k in line["legs_order"]), file=sys.stderr)
