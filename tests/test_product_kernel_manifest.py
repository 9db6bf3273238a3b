"""The product library's kernel list, the manifest that says which test launches each kernel, the
case table of tests/test_product_dispatch_gpu.py and the recorded kernel trace of that file, kept
in step.  A kernel added to ``libfedagg.so`` without an entry here turns check (c) red."""

import ast
import importlib.util
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "substrafl_amd" / "libfedagg.so"
ROW_FAMILIES = ("fedavg_kernel", "scaffold_kernel", "scaffold_bucket_kernel", "scaffold_push_kernel",
                "scaffold_rows_kernel")
# kernels whose only check may be an existing test: gather / tree, equal-count, cast, flat ops, probes
COVERED_BY_OK = ("pairwise_gather_kernel", "pairwise_tree_kernel", "scaffold_gather_kernel", "scaffold_tree_kernel",
                 "bucket_gather_kernel", "bucket_tree_kernel", "equal_count_kernel", "equal_count_vec_kernel",
                 "cast_kernel", "scale_cast_kernel", "flat_seg_kernel", "flat_typed_kernel", "read_probe_kernel",
                 "read_probe_tile_kernel", "push_copy_kernel", "push_signal_kernel", "push_stage_sum_kernel",
                 "push_wait_kernel")


def _load(path: Path, name: str):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def manifest():
    from product_dispatch_manifest import MANIFEST

    return MANIFEST


@pytest.fixture(scope="module")
def committed():
    return [ln.strip() for ln in (ROOT / "profiles" / "product_kernels.txt").read_text().splitlines() if ln.strip()]


def _family(name: str) -> str:
    return name.split("<")[0]


def test_manifest_keys_are_the_committed_kernel_list(manifest, committed):
    """(a) one entry per kernel, each of exactly one kind; rows where rows are required."""
    assert len(set(committed)) == len(committed) and committed == sorted(committed)
    assert set(manifest) == set(committed), (sorted(set(committed) - set(manifest)),
                                             sorted(set(manifest) - set(committed)))
    for name, e in manifest.items():
        assert len(e) == 1 and next(iter(e)) in ("rows", "covered_by", "unreachable"), name
        if "unreachable" in e:
            args = name[name.index("<") + 1: -1].split(", ")
            assert _family(name) == "scaffold_bucket_kernel" and args[6] == "2", name  # the PH = 2 pair
            assert "sc_2l" in e["unreachable"] and "FEDAGG_TUNING" in e["unreachable"]
        elif _family(name) in ROW_FAMILIES and name not in (
                "scaffold_rows_kernel<KF16, 2, 4, false>", "scaffold_rows_kernel<KBF16, 2, 4, false>"):
            # the tile-interleaved fedavg_kernel instantiations (last argument != 0) included
            assert e.get("rows"), f"{name} needs rows"
        elif "covered_by" in e:
            assert _family(name) in COVERED_BY_OK or _family(name) == "scaffold_rows_kernel", name
    assert sum("unreachable" in e for e in manifest.values()) == 2


def test_rows_and_covering_tests_exist(manifest):
    """(b) every row id is a case of the GPU test; every covered_by names a test function."""
    import test_product_dispatch_gpu as gpu_test

    ids = set(gpu_test.CASE_IDS)
    assert len(ids) == len(gpu_test.CASE_IDS)
    claimed = set()
    for name, e in manifest.items():
        for row in e.get("rows", []):
            assert row in ids, f"{name}: no case {row}"
            claimed.add(row)
        if "covered_by" in e:
            path, _, func = e["covered_by"].partition("::")
            assert (ROOT / path).is_file() and path.startswith("tests/"), e["covered_by"]
            tree = ast.parse((ROOT / path).read_text())
            assert any(isinstance(n, ast.FunctionDef) and n.name == func for n in tree.body), e["covered_by"]
    assert claimed == ids, f"cases no kernel claims: {sorted(ids - claimed)}"


def test_built_library_holds_exactly_the_committed_kernels(committed):
    """(c) the live symbol list of the built library against profiles/product_kernels.txt."""
    if not LIB.exists():
        pytest.skip("substrafl_amd/libfedagg.so is not built")
    tool = _load(ROOT / "tools" / "product_kernels.py", "product_kernels")
    live = tool.kernel_names(LIB)
    assert live == committed, ("libfedagg.so and profiles/product_kernels.txt differ -- a new kernel needs a case "
                               "in tests/test_product_dispatch_gpu.py and a manifest entry; only in the library: "
                               f"{sorted(set(live) - set(committed))}, only in the list: "
                               f"{sorted(set(committed) - set(live))}")


def test_trace_shows_every_kernel_with_rows(manifest):
    """(d) profiles/product_dispatch_trace.txt (rocprofv3 --kernel-trace of the GPU test, see
    profiles/README.md) lists every kernel that has rows, and only kernels of the list."""
    traced = {}
    for ln in (ROOT / "profiles" / "product_dispatch_trace.txt").read_text().splitlines():
        if ln.strip():
            name, calls = ln.rsplit("\t", 1)
            traced[name] = int(calls)
    assert set(traced) <= set(manifest), sorted(set(traced) - set(manifest))
    missing = [n for n, e in manifest.items() if "rows" in e and traced.get(n, 0) < 1]
    assert not missing, f"kernels with rows that the traced run never launched: {missing}"
    assert not [n for n, e in manifest.items() if "unreachable" in e and n in traced]
    # a FedAvg or two-bucket Scaffold case is one launch (K <= one argument chunk): as many calls as
    # rows, so no row was served by another kernel than the one the manifest files it under
    for n, e in manifest.items():
        if "rows" in e and _family(n) in ("fedavg_kernel", "scaffold_kernel"):
            assert traced[n] == len(e["rows"]), (n, traced[n], len(e["rows"]))
