"""Which test launches each kernel of the product ``libfedagg.so`` (profiles/product_kernels.txt,
``tools/product_kernels.py``).  Plain data, one entry per kernel name:

* ``rows``: ids of cases of ``tests/test_product_dispatch_gpu.py`` that launch it (every element
  against a reference that shares no code with the kernel);
* ``covered_by``: an existing test that launches it and checks it against a reference (read, not
  traced);
* ``unreachable``: no call of the product build launches it; the reason quotes the dispatch.

Every ``fedavg_kernel`` has rows, the three of the tile-interleaved layout (last template argument
8192, 2048, 4096) included.  Over ``tests/test_tiled_layout.py``, which keeps its cases (K > 128,
P = 17, the random sweep), their rows add: a grid-capped launch in which workgroups walk a second
tile; a tiled buffer built from the layout of ``include/fedagg.h`` instead of the engine's helpers,
with NaN in all padding; a guard band behind the output; planted +-0 / subnormal / largest-finite
values and all -0 columns; the r = ``(VPT - 1) * threads + 100`` remainder; a one-launch
``fedagg_fedavg_chain_tiled_*`` continuation of a known accumulator; the separate gather / tree
path with an index behind tile 0; and buckets of 1, L - 1, L, L + 1 and one tile -1 / 0 / +1 elements.

``tests/test_product_kernel_manifest.py`` keeps this file, the committed kernel list, the built
library and the kernel trace of the rows (profiles/product_dispatch_trace.txt) in step."""

MANIFEST = {
    "bucket_gather_kernel<KBF16>": dict(
        covered_by="tests/test_scaffold16_kernel_gpu.py::test_numel_one_patch"),
    "bucket_gather_kernel<KF16>": dict(
        covered_by="tests/test_scaffold16_kernel_gpu.py::test_numel_one_patch"),
    "bucket_gather_kernel<KF32>": dict(rows=[
        "sc-rows-f32-ph0-K65-r37", "sc-rows-f32-ph1-K65-r37",
    ]),
    "bucket_gather_kernel<KF64>": dict(rows=[
        "sc-rows-f64-ph0-K65-r37", "sc-rows-f64-ph1-K65-r37",
    ]),
    "bucket_tree_kernel": dict(
        covered_by="tests/test_scaffold16_kernel_gpu.py::test_numel_one_patch"),
    "cast_kernel": dict(
        covered_by="tests/test_dtype_plumbing_gpu.py::test_cast_every_pair_bit_exact"),
    "equal_count_kernel<double, 128>": dict(
        covered_by="tests/test_gpu_parity.py::test_equal_count_variants"),
    "equal_count_kernel<float, 128>": dict(
        covered_by="tests/test_gpu_parity.py::test_equal_count_variants"),
    "equal_count_vec_kernel<double, 128, 4>": dict(
        covered_by="tests/test_gpu_parity.py::test_equal_count_variants"),
    "equal_count_vec_kernel<float, 128, 4>": dict(
        covered_by="tests/test_gpu_parity.py::test_equal_count_variants"),
    "fedavg_kernel<BF16, 128, true, 1, 16, 2, false, true, 1, true, 256, 0>": dict(rows=[
        "fa-bf16-16x2-nt-K33-r0", "fa-bf16-16x2-nt-K33-r37-pw", "fa-bf16-16x2-nt-K33-rbig",
        "fa-bf16-16x2-nt-K33-cap500", "fa-bf16-16x2-nt-K33-r37-chain",
    ]),
    "fedavg_kernel<BF16, 128, true, 1, 16, 2, false, true, 1, true, 256, 4096>": dict(rows=[
        "fa-bf16-tiled4096-nt-K33-r0", "fa-bf16-tiled4096-nt-K33-r37-pw", "fa-bf16-tiled4096-nt-K33-rbig",
        "fa-bf16-tiled4096-nt-K33-cap3-pw", "fa-bf16-tiled4096-nt-K33-r37-chain", "fa-bf16-tiled4096-nt-K5-r0",
        "fa-bf16-tiled4096-nt-K5-r37-pw", "fa-bf16-tiled4096-nt-K5-rbig", "fa-bf16-tiled4096-nt-K5-cap3-pw",
        "fa-bf16-tiled4096-nt-K5-r37-chain", "fa-bf16-tiled4096-nt-K33-r37-unfused",
        "fa-bf16-tiled4096-nt-K1-small-M1", "fa-bf16-tiled4096-nt-K1-small-Lm1", "fa-bf16-tiled4096-nt-K1-small-L",
        "fa-bf16-tiled4096-nt-K1-small-Lp1", "fa-bf16-tiled4096-nt-K1-small-TLm1",
        "fa-bf16-tiled4096-nt-K1-small-TL", "fa-bf16-tiled4096-nt-K1-small-TLp1",
        "fa-bf16-tiled4096-nt-K5-small-M1", "fa-bf16-tiled4096-nt-K5-small-Lm1", "fa-bf16-tiled4096-nt-K5-small-L",
        "fa-bf16-tiled4096-nt-K5-small-Lp1", "fa-bf16-tiled4096-nt-K5-small-TLm1",
        "fa-bf16-tiled4096-nt-K5-small-TL", "fa-bf16-tiled4096-nt-K5-small-TLp1",
    ]),
    "fedavg_kernel<BF16, 128, true, 1, 2, 8, false, true, 1, false, 256, 0>": dict(rows=[
        "fa-bf16-2x8-nt-K33-r0", "fa-bf16-2x8-nt-K33-r37-pw", "fa-bf16-2x8-nt-K33-rbig", "fa-bf16-2x8-nt-K33-cap3",
        "fa-bf16-2x8-nt-K33-r37-chain", "fa-bf16-2x8-nt-K33-below-short", "fa-bf16-2x8-nt-K32-at-short-M",
    ]),
    "fedavg_kernel<BF16, 128, true, 1, 4, 4, false, true, 1, false, 256, 0>": dict(rows=[
        "fa-bf16-4x4-nt-K33-r0", "fa-bf16-4x4-nt-K33-r37-pw", "fa-bf16-4x4-nt-K33-rbig", "fa-bf16-4x4-nt-K33-cap100",
        "fa-bf16-4x4-nt-K33-r37-chain", "fa-bf16-4x4-nt-K33-below-mid",
    ]),
    "fedavg_kernel<BF16, 128, true, 1, 8, 4, false, true, 1, false, 256, 0>": dict(rows=[
        "fa-bf16-8x4-nt-K33-r0", "fa-bf16-8x4-nt-K33-r37-pw", "fa-bf16-8x4-nt-K33-rbig", "fa-bf16-8x4-nt-K33-cap100",
        "fa-bf16-8x4-nt-K33-r37-chain", "fa-bf16-8x4-nt-K5-r0", "fa-bf16-8x4-nt-K5-r37-pw", "fa-bf16-8x4-nt-K5-rbig",
        "fa-bf16-8x4-nt-K5-cap3", "fa-bf16-8x4-nt-K5-r37-chain", "fa-bf16-8x4-nt-K33-below-big",
        "fa-bf16-8x4-nt-K8-rbig",
    ]),
    "fedavg_kernel<BF16, 128, true, 2, 16, 2, false, true, 1, true, 256, 0>": dict(rows=[
        "fa-bf16-16x2-sc1-K33-r0", "fa-bf16-16x2-sc1-K33-r37-pw", "fa-bf16-16x2-sc1-K33-rbig",
        "fa-bf16-16x2-sc1-K33-cap500", "fa-bf16-16x2-sc1-K33-r37-chain",
    ]),
    "fedavg_kernel<BF16, 128, true, 2, 2, 8, false, true, 1, false, 256, 0>": dict(rows=[
        "fa-bf16-2x8-sc1-K33-r0", "fa-bf16-2x8-sc1-K33-r37-pw", "fa-bf16-2x8-sc1-K33-rbig",
        "fa-bf16-2x8-sc1-K33-cap3", "fa-bf16-2x8-sc1-K33-r37-chain",
    ]),
    "fedavg_kernel<BF16, 128, true, 2, 4, 4, false, true, 1, false, 256, 0>": dict(rows=[
        "fa-bf16-4x4-sc1-K33-r0", "fa-bf16-4x4-sc1-K33-r37-pw", "fa-bf16-4x4-sc1-K33-rbig",
        "fa-bf16-4x4-sc1-K33-cap100", "fa-bf16-4x4-sc1-K33-r37-chain",
    ]),
    "fedavg_kernel<BF16, 128, true, 2, 8, 4, false, true, 1, false, 256, 0>": dict(rows=[
        "fa-bf16-8x4-sc1-K33-r0", "fa-bf16-8x4-sc1-K33-r37-pw", "fa-bf16-8x4-sc1-K33-rbig",
        "fa-bf16-8x4-sc1-K33-cap100", "fa-bf16-8x4-sc1-K33-r37-chain", "fa-bf16-8x4-sc1-K5-r0",
        "fa-bf16-8x4-sc1-K5-r37-pw", "fa-bf16-8x4-sc1-K5-rbig", "fa-bf16-8x4-sc1-K5-cap3",
        "fa-bf16-8x4-sc1-K5-r37-chain", "fa-bf16-8x4-sc1-K33-below-big", "fa-bf16-8x4-sc1-K31-at-short-M",
        "fa-bf16-8x4-sc1-K8-r37-pw",
    ]),
    "fedavg_kernel<BF16, 128, true, 3, 16, 2, false, true, 1, true, 256, 0>": dict(rows=[
        "fa-bf16-16x2-sys-K33-r0-null", "fa-bf16-16x2-sys-K33-r37-sep", "fa-bf16-16x2-sys-K33-rbig-sep",
        "fa-bf16-16x2-sys-K33-cap500-null",
    ]),
    "fedavg_kernel<BF16, 128, true, 3, 2, 8, false, true, 1, false, 256, 0>": dict(rows=[
        "fa-bf16-2x8-sys-K33-r0-null", "fa-bf16-2x8-sys-K33-r37-sep", "fa-bf16-2x8-sys-K33-rbig-sep",
        "fa-bf16-2x8-sys-K33-cap3-null",
    ]),
    "fedavg_kernel<BF16, 128, true, 3, 4, 4, false, true, 1, false, 256, 0>": dict(rows=[
        "fa-bf16-4x4-sys-K33-r0-null", "fa-bf16-4x4-sys-K33-r37-sep", "fa-bf16-4x4-sys-K33-rbig-sep",
        "fa-bf16-4x4-sys-K33-cap100-null",
    ]),
    "fedavg_kernel<BF16, 128, true, 3, 8, 4, false, true, 1, false, 256, 0>": dict(rows=[
        "fa-bf16-8x4-sys-K33-r0-null", "fa-bf16-8x4-sys-K33-r37-sep", "fa-bf16-8x4-sys-K33-rbig-sep",
        "fa-bf16-8x4-sys-K33-cap100-null", "fa-bf16-8x4-sys-K5-r0-null", "fa-bf16-8x4-sys-K5-r37-sep",
        "fa-bf16-8x4-sys-K5-rbig-sep", "fa-bf16-8x4-sys-K5-cap3-null", "fa-bf16-8x4-sys-K8-r37-sep",
    ]),
    "fedavg_kernel<F16, 128, true, 1, 16, 2, false, true, 1, false, 256, 0>": dict(rows=[
        "fa-f16-16x2-nt-K33-r0", "fa-f16-16x2-nt-K33-r37-pw", "fa-f16-16x2-nt-K33-rbig", "fa-f16-16x2-nt-K33-cap500",
        "fa-f16-16x2-nt-K33-r37-chain", "fa-f16-16x2-nt-K32-at-big-M",
    ]),
    "fedavg_kernel<F16, 128, true, 1, 4, 4, false, true, 1, false, 256, 0>": dict(rows=[
        "fa-f16-4x4-nt-K5-r0", "fa-f16-4x4-nt-K5-r37-pw", "fa-f16-4x4-nt-K5-rbig", "fa-f16-4x4-nt-K5-cap3",
        "fa-f16-4x4-nt-K5-r37-chain", "fa-f16-4x4-nt-K33-r0", "fa-f16-4x4-nt-K33-r37-pw", "fa-f16-4x4-nt-K33-rbig",
        "fa-f16-4x4-nt-K33-cap3", "fa-f16-4x4-nt-K33-r37-chain", "fa-f16-4x4-nt-K33-below-big",
    ]),
    "fedavg_kernel<F16, 128, true, 2, 16, 2, false, true, 1, false, 256, 0>": dict(rows=[
        "fa-f16-16x2-sc1-K33-r0", "fa-f16-16x2-sc1-K33-r37-pw", "fa-f16-16x2-sc1-K33-rbig",
        "fa-f16-16x2-sc1-K33-cap500", "fa-f16-16x2-sc1-K33-r37-chain",
    ]),
    "fedavg_kernel<F16, 128, true, 2, 4, 4, false, true, 1, false, 256, 0>": dict(rows=[
        "fa-f16-4x4-sc1-K5-r0", "fa-f16-4x4-sc1-K5-r37-pw", "fa-f16-4x4-sc1-K5-rbig", "fa-f16-4x4-sc1-K5-cap3",
        "fa-f16-4x4-sc1-K5-r37-chain", "fa-f16-4x4-sc1-K33-r0", "fa-f16-4x4-sc1-K33-r37-pw",
        "fa-f16-4x4-sc1-K33-rbig", "fa-f16-4x4-sc1-K33-cap3", "fa-f16-4x4-sc1-K33-r37-chain",
        "fa-f16-4x4-sc1-K33-below-big", "fa-f16-4x4-sc1-K31-at-big-M", "fa-f16-4x4-sc1-K8-r37-pw",
    ]),
    "fedavg_kernel<F32, 128, true, 1, 16, 2, false, true, 1, false, 512, 0>": dict(rows=[
        "fa-f32-16x2-nt-K33-r0", "fa-f32-16x2-nt-K33-r37-pw", "fa-f32-16x2-nt-K33-rbig", "fa-f32-16x2-nt-K33-cap500",
        "fa-f32-16x2-nt-K33-r37-chain",
    ]),
    "fedavg_kernel<F32, 128, true, 1, 16, 2, false, true, 1, false, 512, 8192>": dict(rows=[
        "fa-f32-tiled8192-nt-K33-r0", "fa-f32-tiled8192-nt-K33-r37-pw", "fa-f32-tiled8192-nt-K33-rbig",
        "fa-f32-tiled8192-nt-K33-cap3-pw", "fa-f32-tiled8192-nt-K33-r37-chain", "fa-f32-tiled8192-nt-K5-r0",
        "fa-f32-tiled8192-nt-K5-r37-pw", "fa-f32-tiled8192-nt-K5-rbig", "fa-f32-tiled8192-nt-K5-cap3-pw",
        "fa-f32-tiled8192-nt-K5-r37-chain", "fa-f32-tiled8192-nt-K33-r37-unfused",
        "fa-f32-tiled8192-nt-K1-small-M1", "fa-f32-tiled8192-nt-K1-small-Lm1", "fa-f32-tiled8192-nt-K1-small-L",
        "fa-f32-tiled8192-nt-K1-small-Lp1", "fa-f32-tiled8192-nt-K1-small-TLm1", "fa-f32-tiled8192-nt-K1-small-TL",
        "fa-f32-tiled8192-nt-K1-small-TLp1", "fa-f32-tiled8192-nt-K5-small-M1", "fa-f32-tiled8192-nt-K5-small-Lm1",
        "fa-f32-tiled8192-nt-K5-small-L", "fa-f32-tiled8192-nt-K5-small-Lp1", "fa-f32-tiled8192-nt-K5-small-TLm1",
        "fa-f32-tiled8192-nt-K5-small-TL", "fa-f32-tiled8192-nt-K5-small-TLp1",
    ]),
    "fedavg_kernel<F32, 128, true, 1, 2, 8, false, true, 1, false, 256, 0>": dict(rows=[
        "fa-f32-2x8-nt-K33-r0", "fa-f32-2x8-nt-K33-r37-pw", "fa-f32-2x8-nt-K33-rbig", "fa-f32-2x8-nt-K33-cap3",
        "fa-f32-2x8-nt-K33-r37-chain", "fa-f32-2x8-nt-K33-below-short", "fa-f32-2x8-nt-K32-at-short-M",
    ]),
    "fedavg_kernel<F32, 128, true, 1, 4, 4, false, true, 1, false, 256, 0>": dict(rows=[
        "fa-f32-4x4-nt-K33-r0", "fa-f32-4x4-nt-K33-r37-pw", "fa-f32-4x4-nt-K33-rbig", "fa-f32-4x4-nt-K33-cap100",
        "fa-f32-4x4-nt-K33-r37-chain", "fa-f32-4x4-nt-K33-below-mid",
    ]),
    "fedavg_kernel<F32, 128, true, 1, 8, 4, false, true, 1, false, 256, 0>": dict(rows=[
        "fa-f32-8x4-nt-K33-r0", "fa-f32-8x4-nt-K33-r37-pw", "fa-f32-8x4-nt-K33-rbig", "fa-f32-8x4-nt-K33-cap100",
        "fa-f32-8x4-nt-K33-r37-chain", "fa-f32-8x4-nt-K5-r0", "fa-f32-8x4-nt-K5-r37-pw", "fa-f32-8x4-nt-K5-rbig",
        "fa-f32-8x4-nt-K5-cap3", "fa-f32-8x4-nt-K5-r37-chain", "fa-f32-8x4-nt-K33-below-big",
        "fa-f32-8x4-nt-K8-rbig",
    ]),
    "fedavg_kernel<F32, 128, true, 2, 16, 2, false, true, 1, false, 512, 0>": dict(rows=[
        "fa-f32-16x2-sc1-K33-r0", "fa-f32-16x2-sc1-K33-r37-pw", "fa-f32-16x2-sc1-K33-rbig",
        "fa-f32-16x2-sc1-K33-cap500", "fa-f32-16x2-sc1-K33-r37-chain",
    ]),
    "fedavg_kernel<F32, 128, true, 2, 2, 8, false, true, 1, false, 256, 0>": dict(rows=[
        "fa-f32-2x8-sc1-K33-r0", "fa-f32-2x8-sc1-K33-r37-pw", "fa-f32-2x8-sc1-K33-rbig", "fa-f32-2x8-sc1-K33-cap3",
        "fa-f32-2x8-sc1-K33-r37-chain",
    ]),
    "fedavg_kernel<F32, 128, true, 2, 4, 4, false, true, 1, false, 256, 0>": dict(rows=[
        "fa-f32-4x4-sc1-K33-r0", "fa-f32-4x4-sc1-K33-r37-pw", "fa-f32-4x4-sc1-K33-rbig", "fa-f32-4x4-sc1-K33-cap100",
        "fa-f32-4x4-sc1-K33-r37-chain",
    ]),
    "fedavg_kernel<F32, 128, true, 2, 8, 4, false, true, 1, false, 256, 0>": dict(rows=[
        "fa-f32-8x4-sc1-K33-r0", "fa-f32-8x4-sc1-K33-r37-pw", "fa-f32-8x4-sc1-K33-rbig", "fa-f32-8x4-sc1-K33-cap100",
        "fa-f32-8x4-sc1-K33-r37-chain", "fa-f32-8x4-sc1-K5-r0", "fa-f32-8x4-sc1-K5-r37-pw", "fa-f32-8x4-sc1-K5-rbig",
        "fa-f32-8x4-sc1-K5-cap3", "fa-f32-8x4-sc1-K5-r37-chain", "fa-f32-8x4-sc1-K33-below-big",
        "fa-f32-8x4-sc1-K31-at-short-M", "fa-f32-8x4-sc1-K8-r37-pw",
    ]),
    "fedavg_kernel<F32, 128, true, 2, 8, 4, false, true, 1, false, 256, 2048>": dict(rows=[
        "fa-f32-tiled2048-sc1-K5-r0", "fa-f32-tiled2048-sc1-K5-r37-pw", "fa-f32-tiled2048-sc1-K5-rbig",
        "fa-f32-tiled2048-sc1-K5-cap3-pw", "fa-f32-tiled2048-sc1-K5-r37-chain", "fa-f32-tiled2048-sc1-K33-r0",
        "fa-f32-tiled2048-sc1-K33-r37-pw", "fa-f32-tiled2048-sc1-K33-rbig", "fa-f32-tiled2048-sc1-K33-cap3-pw",
        "fa-f32-tiled2048-sc1-K33-r37-chain", "fa-f32-tiled2048-sc1-K5-r37-unfused",
        "fa-f32-tiled2048-sc1-K1-small-M1", "fa-f32-tiled2048-sc1-K1-small-Lm1", "fa-f32-tiled2048-sc1-K1-small-L",
        "fa-f32-tiled2048-sc1-K1-small-Lp1", "fa-f32-tiled2048-sc1-K1-small-TLm1",
        "fa-f32-tiled2048-sc1-K1-small-TL", "fa-f32-tiled2048-sc1-K1-small-TLp1",
        "fa-f32-tiled2048-sc1-K5-small-M1", "fa-f32-tiled2048-sc1-K5-small-Lm1", "fa-f32-tiled2048-sc1-K5-small-L",
        "fa-f32-tiled2048-sc1-K5-small-Lp1", "fa-f32-tiled2048-sc1-K5-small-TLm1",
        "fa-f32-tiled2048-sc1-K5-small-TL", "fa-f32-tiled2048-sc1-K5-small-TLp1",
    ]),
    "fedavg_kernel<F32, 128, true, 3, 16, 2, false, true, 1, false, 512, 0>": dict(rows=[
        "fa-f32-16x2-sys-K33-r0-null", "fa-f32-16x2-sys-K33-r37-sep", "fa-f32-16x2-sys-K33-rbig-sep",
        "fa-f32-16x2-sys-K33-cap500-null",
    ]),
    "fedavg_kernel<F32, 128, true, 3, 2, 8, false, true, 1, false, 256, 0>": dict(rows=[
        "fa-f32-2x8-sys-K33-r0-null", "fa-f32-2x8-sys-K33-r37-sep", "fa-f32-2x8-sys-K33-rbig-sep",
        "fa-f32-2x8-sys-K33-cap3-null",
    ]),
    "fedavg_kernel<F32, 128, true, 3, 4, 4, false, true, 1, false, 256, 0>": dict(rows=[
        "fa-f32-4x4-sys-K33-r0-null", "fa-f32-4x4-sys-K33-r37-sep", "fa-f32-4x4-sys-K33-rbig-sep",
        "fa-f32-4x4-sys-K33-cap100-null",
    ]),
    "fedavg_kernel<F32, 128, true, 3, 8, 4, false, true, 1, false, 256, 0>": dict(rows=[
        "fa-f32-8x4-sys-K33-r0-null", "fa-f32-8x4-sys-K33-r37-sep", "fa-f32-8x4-sys-K33-rbig-sep",
        "fa-f32-8x4-sys-K33-cap100-null", "fa-f32-8x4-sys-K5-r0-null", "fa-f32-8x4-sys-K5-r37-sep",
        "fa-f32-8x4-sys-K5-rbig-sep", "fa-f32-8x4-sys-K5-cap3-null", "fa-f32-8x4-sys-K8-r37-sep",
    ]),
    "fedavg_kernel<F64, 128, true, 1, 4, 4, true, true, 1, false, 256, 0>": dict(rows=[
        "fa-f64-4x4p-nt-K5-r0", "fa-f64-4x4p-nt-K5-r37-pw", "fa-f64-4x4p-nt-K5-rbig", "fa-f64-4x4p-nt-K5-cap3",
        "fa-f64-4x4p-nt-K5-r37-chain", "fa-f64-4x4p-nt-K33-r0", "fa-f64-4x4p-nt-K33-r37-pw",
        "fa-f64-4x4p-nt-K33-rbig", "fa-f64-4x4p-nt-K33-cap3", "fa-f64-4x4p-nt-K33-r37-chain",
        "fa-f64-4x4p-nt-K32-r37",
    ]),
    "fedavg_kernel<F64, 128, true, 2, 4, 4, true, true, 1, false, 256, 0>": dict(rows=[
        "fa-f64-4x4p-sc1-K5-r0", "fa-f64-4x4p-sc1-K5-r37-pw", "fa-f64-4x4p-sc1-K5-rbig", "fa-f64-4x4p-sc1-K5-cap3",
        "fa-f64-4x4p-sc1-K5-r37-chain", "fa-f64-4x4p-sc1-K33-r0", "fa-f64-4x4p-sc1-K33-r37-pw",
        "fa-f64-4x4p-sc1-K33-rbig", "fa-f64-4x4p-sc1-K33-cap3", "fa-f64-4x4p-sc1-K33-r37-chain",
        "fa-f64-4x4p-sc1-K8-r37-pw", "fa-f64-4x4p-sc1-K31-r37",
    ]),
    "flat_seg_kernel<0>": dict(rows=[
        "misc-flat-gather-f64",
    ]),
    "flat_seg_kernel<2>": dict(
        covered_by="tests/test_client_buckets.py::test_flat_wsum_three_and_four_lists_vs_torch_on_cpu"),
    "flat_seg_kernel<3>": dict(
        covered_by="tests/test_client_buckets.py::test_flat_increment_vs_torch_on_cpu"),
    "flat_typed_kernel<0, 0, false>": dict(
        covered_by="tests/test_half_client_ops_gpu.py::test_native_half_ops_bit_exact_with_guard_bands"),
    "flat_typed_kernel<0, 1, false>": dict(
        covered_by="tests/test_client_buckets.py::test_flat_gather_then_scatter_round_trips"),
    "flat_typed_kernel<1, 1, false>": dict(
        covered_by="tests/test_client_buckets.py::test_flat_gather_then_scatter_round_trips"),
    "flat_typed_kernel<2, 0, false>": dict(
        covered_by="tests/test_half_client_ops_gpu.py::test_native_half_ops_bit_exact_with_guard_bands"),
    "flat_typed_kernel<2, 1, false>": dict(
        covered_by="tests/test_client_buckets.py::test_flat_wsum_three_and_four_lists_vs_torch_on_cpu"),
    "flat_typed_kernel<2, 12, false>": dict(
        covered_by="tests/test_half_client_ops_gpu.py::test_native_half_ops_bit_exact_with_guard_bands"),
    "flat_typed_kernel<3, 0, false>": dict(
        covered_by="tests/test_half_client_ops_gpu.py::test_native_increment_same_kind_bit_exact"),
    "flat_typed_kernel<3, 1, false>": dict(
        covered_by="tests/test_client_buckets.py::test_flat_increment_vs_torch_on_cpu"),
    "flat_typed_kernel<3, 12, false>": dict(
        covered_by="tests/test_half_client_ops_gpu.py::test_native_increment_same_kind_bit_exact"),
    "flat_typed_kernel<3, 12, true>": dict(
        covered_by="tests/test_half_client_ops_gpu.py::test_native_increment_bf16_by_fp32_promoted_add"),
    "pairwise_gather_kernel<BF16, 128>": dict(rows=[
        "fa-bf16-tiled4096-nt-K33-r37-unfused",
    ]),
    "pairwise_gather_kernel<F16, 128>": dict(
        covered_by="tests/test_multi_abi_gpu.py::test_multi_entry_bit_exact"),
    "pairwise_gather_kernel<F32, 128>": dict(
        covered_by="tests/test_gpu_parity.py::test_many_numel1_layers_fused_and_separate"),
    "pairwise_gather_kernel<F64, 128>": dict(
        covered_by="tests/test_multi_abi_gpu.py::test_multi_entry_bit_exact"),
    "pairwise_tree_kernel<BF16>": dict(rows=[
        "fa-bf16-tiled4096-nt-K33-r37-unfused",
    ]),
    "pairwise_tree_kernel<F16>": dict(
        covered_by="tests/test_multi_abi_gpu.py::test_multi_entry_bit_exact"),
    "pairwise_tree_kernel<F32>": dict(
        covered_by="tests/test_gpu_parity.py::test_many_numel1_layers_fused_and_separate"),
    "pairwise_tree_kernel<F64>": dict(
        covered_by="tests/test_multi_abi_gpu.py::test_multi_entry_bit_exact"),
    "push_copy_kernel": dict(
        covered_by="tests/test_push_gpu.py::test_push_executor_processes_bit_exact"),
    "push_signal_kernel": dict(
        covered_by="tests/test_push_gpu.py::test_push_executor_processes_bit_exact"),
    "push_stage_sum_kernel<double>": dict(
        covered_by="tests/test_push_gpu.py::test_push_executor_processes_bit_exact"),
    "push_stage_sum_kernel<float>": dict(
        covered_by="tests/test_push_gpu.py::test_push_executor_processes_bit_exact"),
    "push_wait_kernel": dict(
        covered_by="tests/test_push_gpu.py::test_push_executor_processes_bit_exact"),
    "read_probe_kernel": dict(rows=[
        "misc-read-probe-stream",
    ]),
    "read_probe_tile_kernel<16>": dict(rows=[
        "misc-read-probe-tile-16",
    ]),
    "read_probe_tile_kernel<4>": dict(rows=[
        "misc-read-probe-tile-4",
    ]),
    "read_probe_tile_kernel<8>": dict(rows=[
        "misc-read-probe-tile-8",
    ]),
    "scaffold_bucket_kernel<double, 64, true, 1, 4, 2, 0, true>": dict(rows=[
        "sc-bucket2l-f64-K17-r0", "sc-bucket2l-f64-K17-r37", "sc-bucket2l-f64-K17-rbig", "sc-bucket2l-f64-K65-r0",
        "sc-bucket2l-f64-K65-r37", "sc-bucket2l-f64-K65-rbig", "sc-bucket2l-f64-K17-cap3",
    ]),
    "scaffold_bucket_kernel<double, 64, true, 1, 4, 2, 1, true>": dict(rows=[
        "sc-bucket2l-f64-K17-r0", "sc-bucket2l-f64-K17-r37", "sc-bucket2l-f64-K17-rbig", "sc-bucket2l-f64-K65-r0",
        "sc-bucket2l-f64-K65-r37", "sc-bucket2l-f64-K65-rbig", "sc-bucket2l-f64-K17-cap3",
    ]),
    "scaffold_bucket_kernel<double, 64, true, 1, 4, 2, 2, true>": dict(
        unreachable=(
            'fedagg_tune("sc_2l", 2) is refused by the product build (fedagg_tune: `else if (!strcmp(key, '
            '"sc_2l") && value <= 1)`; the value-2 branch is under `#if FEDAGG_TUNING`), and '
            'launch_scaffold_2l_variant launches PH = 2 only `if (g_sc_2l == 2)`'
        )),
    "scaffold_bucket_kernel<float, 64, true, 1, 8, 4, 0, false>": dict(rows=[
        "sc-bucket2l-f32-K17-r0", "sc-bucket2l-f32-K17-r37", "sc-bucket2l-f32-K17-rbig", "sc-bucket2l-f32-K65-r0",
        "sc-bucket2l-f32-K65-r37", "sc-bucket2l-f32-K65-rbig", "sc-bucket2l-f32-K17-cap3",
    ]),
    "scaffold_bucket_kernel<float, 64, true, 1, 8, 4, 1, false>": dict(rows=[
        "sc-bucket2l-f32-K17-r0", "sc-bucket2l-f32-K17-r37", "sc-bucket2l-f32-K17-rbig", "sc-bucket2l-f32-K65-r0",
        "sc-bucket2l-f32-K65-r37", "sc-bucket2l-f32-K65-rbig", "sc-bucket2l-f32-K17-cap3",
    ]),
    "scaffold_bucket_kernel<float, 64, true, 1, 8, 4, 2, false>": dict(
        unreachable=(
            'fedagg_tune("sc_2l", 2) is refused by the product build (fedagg_tune: `else if (!strcmp(key, '
            '"sc_2l") && value <= 1)`; the value-2 branch is under `#if FEDAGG_TUNING`), and '
            'launch_scaffold_2l_variant launches PH = 2 only `if (g_sc_2l == 2)`'
        )),
    "scaffold_gather_kernel<double, 64>": dict(rows=[
        "sc-bucket2l-f64-K65-r37",
    ]),
    "scaffold_gather_kernel<float, 64>": dict(rows=[
        "sc-bucket2l-f32-K65-r37",
    ]),
    "scaffold_kernel<double, 64, true, 1, 4, 4, false, false, false, false, 1, 256>": dict(rows=[
        "sc-two-f64-4x4-K5-r0", "sc-two-f64-4x4-K5-r37", "sc-two-f64-4x4-K5-rbig", "sc-two-f64-4x4-K5-cap3",
    ]),
    "scaffold_kernel<double, 64, true, 1, 8, 2, false, false, false, false, 1, 256>": dict(rows=[
        "sc-two-f64-8x2-K33-r0", "sc-two-f64-8x2-K33-r37", "sc-two-f64-8x2-K33-rbig", "sc-two-f64-8x2-K33-cap3",
        "sc-two-f64-8x2-K33-unaligned",
    ]),
    "scaffold_kernel<float, 64, true, 1, 4, 4, false, false, false, false, 1, 256>": dict(rows=[
        "sc-two-f32-4x4-K5-r0", "sc-two-f32-4x4-K5-r37", "sc-two-f32-4x4-K5-rbig", "sc-two-f32-4x4-K5-cap3",
    ]),
    "scaffold_kernel<float, 64, true, 1, 8, 4, false, false, true, false, 1, 256>": dict(rows=[
        "sc-two-f32-8x4buf-K33-r0", "sc-two-f32-8x4buf-K33-r37", "sc-two-f32-8x4buf-K33-rbig",
        "sc-two-f32-8x4buf-K33-cap3", "sc-two-f32-8x4buf-K33-unaligned",
    ]),
    "scaffold_push_kernel<double, 4, 2, 0, true, false>": dict(rows=[
        "sc-push-f64-ph0-null-K9-r0-finish", "sc-push-f64-ph0-null-K9-r37-sums",
        "sc-push-f64-ph0-null-K9-rbig-finish", "sc-push-f64-ph0-null-K65-r37-finish",
        "sc-push-f64-ph0-null-K9-cap3-sums",
    ]),
    "scaffold_push_kernel<double, 4, 2, 0, true, true>": dict(rows=[
        "sc-push-f64-ph0-sep-K9-r0-finish", "sc-push-f64-ph0-sep-K9-r37-sums", "sc-push-f64-ph0-sep-K9-rbig-finish",
        "sc-push-f64-ph0-sep-K65-r37-finish", "sc-push-f64-ph0-sep-K9-cap3-sums",
    ]),
    "scaffold_push_kernel<double, 4, 2, 1, true, false>": dict(rows=[
        "sc-push-f64-ph1-null-K9-r0-finish", "sc-push-f64-ph1-null-K9-r37-sums",
        "sc-push-f64-ph1-null-K9-rbig-finish", "sc-push-f64-ph1-null-K65-r37-finish",
        "sc-push-f64-ph1-null-K9-cap3-sums",
    ]),
    "scaffold_push_kernel<double, 4, 2, 1, true, true>": dict(rows=[
        "sc-push-f64-ph1-sep-K9-r0-finish", "sc-push-f64-ph1-sep-K9-r37-sums", "sc-push-f64-ph1-sep-K9-rbig-finish",
        "sc-push-f64-ph1-sep-K65-r37-finish", "sc-push-f64-ph1-sep-K9-cap3-sums",
    ]),
    "scaffold_push_kernel<float, 8, 4, 0, false, false>": dict(rows=[
        "sc-push-f32-ph0-null-K9-r0-finish", "sc-push-f32-ph0-null-K9-r37-sums",
        "sc-push-f32-ph0-null-K9-rbig-finish", "sc-push-f32-ph0-null-K65-r37-finish",
        "sc-push-f32-ph0-null-K9-cap3-sums",
    ]),
    "scaffold_push_kernel<float, 8, 4, 0, false, true>": dict(rows=[
        "sc-push-f32-ph0-sep-K9-r0-finish", "sc-push-f32-ph0-sep-K9-r37-sums", "sc-push-f32-ph0-sep-K9-rbig-finish",
        "sc-push-f32-ph0-sep-K65-r37-finish", "sc-push-f32-ph0-sep-K9-cap3-sums",
    ]),
    "scaffold_push_kernel<float, 8, 4, 1, false, false>": dict(rows=[
        "sc-push-f32-ph1-null-K9-r0-finish", "sc-push-f32-ph1-null-K9-r37-sums",
        "sc-push-f32-ph1-null-K9-rbig-finish", "sc-push-f32-ph1-null-K65-r37-finish",
        "sc-push-f32-ph1-null-K9-cap3-sums",
    ]),
    "scaffold_push_kernel<float, 8, 4, 1, false, true>": dict(rows=[
        "sc-push-f32-ph1-sep-K9-r0-finish", "sc-push-f32-ph1-sep-K9-r37-sums", "sc-push-f32-ph1-sep-K9-rbig-finish",
        "sc-push-f32-ph1-sep-K65-r37-finish", "sc-push-f32-ph1-sep-K9-cap3-sums",
    ]),
    "scaffold_rows_kernel<KBF16, 2, 4, false>": dict(
        covered_by="tests/test_scaffold16_kernel_gpu.py::test_sizes_alignment_and_grid_stride"),
    "scaffold_rows_kernel<KF16, 2, 4, false>": dict(
        covered_by="tests/test_scaffold16_kernel_gpu.py::test_sizes_alignment_and_grid_stride"),
    "scaffold_rows_kernel<KF32, 8, 4, false>": dict(rows=[
        "sc-rows-f32-ph0-K5-r0", "sc-rows-f32-ph0-K5-r37", "sc-rows-f32-ph0-K5-rbig", "sc-rows-f32-ph0-K65-r37",
        "sc-rows-f32-ph0-K5-cap3", "sc-rows-f32-ph0-K5-unaligned", "sc-rows-f32-ph1-K5-r0", "sc-rows-f32-ph1-K5-r37",
        "sc-rows-f32-ph1-K5-rbig", "sc-rows-f32-ph1-K65-r37", "sc-rows-f32-ph1-K5-cap3",
        "sc-rows-f32-ph1-K5-unaligned",
    ]),
    "scaffold_rows_kernel<KF64, 4, 2, true>": dict(rows=[
        "sc-rows-f64-ph0-K5-r0", "sc-rows-f64-ph0-K5-r37", "sc-rows-f64-ph0-K5-rbig", "sc-rows-f64-ph0-K65-r37",
        "sc-rows-f64-ph0-K5-cap3", "sc-rows-f64-ph0-K5-unaligned", "sc-rows-f64-ph1-K5-r0", "sc-rows-f64-ph1-K5-r37",
        "sc-rows-f64-ph1-K5-rbig", "sc-rows-f64-ph1-K65-r37", "sc-rows-f64-ph1-K5-cap3",
        "sc-rows-f64-ph1-K5-unaligned",
    ]),
    "scaffold_tree_kernel<double>": dict(rows=[
        "sc-bucket2l-f64-K65-r37",
    ]),
    "scaffold_tree_kernel<float>": dict(rows=[
        "sc-bucket2l-f32-K65-r37",
    ]),
    "scale_cast_kernel": dict(
        covered_by="tests/test_dtype_plumbing_gpu.py::test_scale_cast_every_pair_bit_exact"),
}
