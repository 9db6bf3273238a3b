"""One entry per ``include/fedagg.h`` prototype whose last parameter is ``void* stream``: the ids of
the cases of ``tests/test_stream_contract_gpu.py`` that run the entry on a non-blocking side stream,
capture it into a graph and replay it, or the reason why the header's two promises ("asynchronous on
that stream", "capturable into a hipGraph") are not pinned for it.  Plain data, importable without
a GPU; ``tests/test_stream_contract_table.py`` keeps it in step with the header and the GPU file."""

# K = 3 with P = 2 (fused patch), P = 17 (separate path), P = 65 (two index batches); K = 129 (two chunks)
_PATCH = ["K3-P2", "K3-P17", "K3-P65", "K129-P2"]
_SCAFFOLD = ["K3-P2", "K17-P2", "K65-P1"]
_BUCKET = [f"scaffold_bucket-{kind}-c{c}-ph{phase}-{shape}"
           for kind, cs in (("f16", ("f16", "f64")), ("bf16", ("bf16", "f64")), ("f32", ("f32",)), ("f64", ("f64",)))
           for c in cs for phase in (0, 1) for shape in ("K3-P2", "K65-P1")]


def cases(*ids):
    return {"cases": list(ids)}


def excluded(reason):
    return {"excluded": reason}


TABLE = {
    # FedAvg
    "fedagg_fedavg_f32": cases(*[f"fedavg_f32-{s}" for s in _PATCH]),
    "fedagg_fedavg_bf16": cases(*[f"fedavg_bf16-{s}" for s in _PATCH]),
    "fedagg_fedavg_f64": cases(*[f"fedavg_f64-{s}" for s in _PATCH]),
    "fedagg_fedavg_f16": cases(*[f"fedavg_f16-{s}" for s in _PATCH]),
    "fedagg_fedavg_tiled_f32": cases(*[f"fedavg_tiled_f32-T{tv}-{s}" for tv in (8192, 2048) for s in _PATCH]),
    "fedagg_fedavg_tiled_bf16": cases(*[f"fedavg_tiled_bf16-T4096-{s}" for s in _PATCH]),
    "fedagg_fedavg_chain_f32": cases("fedavg_chain_f32"),
    "fedagg_fedavg_chain_bf16": cases("fedavg_chain_bf16"),
    "fedagg_fedavg_chain_f64": cases("fedavg_chain_f64"),
    "fedagg_fedavg_chain_f16": cases("fedavg_chain_f16"),
    "fedagg_fedavg_chain_tiled_f32": cases("fedavg_chain_tiled_f32-T8192", "fedavg_chain_tiled_f32-T2048"),
    "fedagg_fedavg_chain_tiled_bf16": cases("fedavg_chain_tiled_bf16-T4096"),
    "fedagg_fedavg_chain_push_f32": cases("fedavg_chain_push_f32"),
    "fedagg_fedavg_chain_push_bf16": cases("fedavg_chain_push_bf16"),
    # Scaffold
    "fedagg_scaffold_f32": cases(*[f"scaffold_f32-{s}" for s in _SCAFFOLD]),
    "fedagg_scaffold_f64": cases(*[f"scaffold_f64-{s}" for s in _SCAFFOLD]),
    "fedagg_scaffold_bucket": cases(*_BUCKET),
    "fedagg_scaffold_chain_f32": cases("scaffold_chain_f32"),
    "fedagg_scaffold_chain_f64": cases("scaffold_chain_f64"),
    "fedagg_scaffold_chain_push_f32": cases("scaffold_chain_push_f32-ph0", "scaffold_chain_push_f32-ph1"),
    "fedagg_scaffold_chain_push_f64": cases("scaffold_chain_push_f64-ph0", "scaffold_chain_push_f64-ph1"),
    "fedagg_scaffold_products_f32": cases("scaffold_pairwise_f32-P3", "scaffold_pairwise_f32-P65"),
    "fedagg_scaffold_products_f64": cases("scaffold_pairwise_f64-P3", "scaffold_pairwise_f64-P65"),
    "fedagg_scaffold_finish_f32": cases("scaffold_pairwise_f32-P3", "scaffold_pairwise_f32-P65"),
    "fedagg_scaffold_finish_f64": cases("scaffold_pairwise_f64-P3", "scaffold_pairwise_f64-P65"),
    # split numel == 1 trees (fedagg_pairwise_finish_f32 also serves bf16 buckets)
    "fedagg_pairwise_products_f32": cases("pairwise_f32-P3", "pairwise_f32-P65"),
    "fedagg_pairwise_products_bf16": cases("pairwise_bf16-P3", "pairwise_bf16-P65"),
    "fedagg_pairwise_products_f64": cases("pairwise_f64-P3", "pairwise_f64-P65"),
    "fedagg_pairwise_products_f16": cases("pairwise_f16-P3", "pairwise_f16-P65"),
    "fedagg_pairwise_finish_f32": cases("pairwise_f32-P3", "pairwise_f32-P65", "pairwise_bf16-P3", "pairwise_bf16-P65"),
    "fedagg_pairwise_finish_f64": cases("pairwise_f64-P3", "pairwise_f64-P65"),
    "fedagg_pairwise_finish_f16": cases("pairwise_f16-P3", "pairwise_f16-P65"),
    # equality check
    "fedagg_equal_count_f32": cases("equal_count_f32-K7", "equal_count_f32-K131"),
    "fedagg_equal_count_f64": cases("equal_count_f64-K7", "equal_count_f64-K131"),
    # client flat ops
    "fedagg_flat_gather_f32": cases("flat_gather_f32"),
    "fedagg_flat_scatter_f32": cases("flat_scatter_f32"),
    "fedagg_flat_wsum_f32": cases("flat_wsum_f32"),
    "fedagg_flat_increment_f32": cases("flat_increment_f32"),
    "fedagg_flat_gather": cases(*[f"flat_gather-{k}" for k in ("f16", "bf16", "f32", "f64")]),
    "fedagg_flat_wsum": cases("flat_wsum-f32-f32-to-f32", "flat_wsum-f32-f64-to-f64", "flat_wsum-f64-f32-to-f64",
                              "flat_wsum-f64-f64-to-f64", "flat_wsum-f16-f16-to-f16", "flat_wsum-bf16-bf16-to-bf16"),
    "fedagg_flat_increment": cases("flat_increment-f32", "flat_increment-f64"),
    "fedagg_flat_increment_kind": cases("flat_increment_kind-f16-f16", "flat_increment_kind-bf16-bf16",
                                        "flat_increment_kind-bf16-f32"),
    # casts and probes
    "fedagg_cast": cases("cast-i64-f64", "cast-f64-f16", "cast-f32-f64"),
    "fedagg_scale_cast": cases("scale_cast-f64-f16", "scale_cast-f32-f64"),
    "fedagg_read_probe_f32": cases("read_probe"),
    "fedagg_read_probe_tile_f32": cases("read_probe_tile-4", "read_probe_tile-8", "read_probe_tile-16"),
    # not covered by the promises
    "fedagg_lockstep_execute": excluded("drives the communicator's stream, RCCL and other ranks as well; its header text "
                                        "promises ordering on `stream` only at the end"),
    "fedagg_push_execute": excluded("forks onto the aux streams and waits for other processes' progress counters; its "
                                    "header text promises ordering on `stream` only at the end"),
    "fedagg_copy_async": excluded("exported by the FEDAGG_TUNING build only; the product library does not hold it"),
}
