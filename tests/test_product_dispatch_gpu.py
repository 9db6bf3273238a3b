"""Every reduction kernel the product ``libfedagg.so`` holds, launched through the default
dispatch (``shape_for`` / ``launch_fedavg_shape``, ``launch_scaffold`` / ``launch_scaffold_2l``,
the push entry points) and compared on EVERY output element, bit for bit, with a reference that
shares no code with the kernels.  ``tests/product_dispatch_manifest.py`` maps each kernel of
``profiles/product_kernels.txt`` to the ids of the cases below that launch it.

Shapes: the smallest at which dispatch picks each tile, ``nvec = n_full * tile + r`` 16-byte
vectors with r = 0, 37 and ``(VPT - 1) * threads + 100`` (the last tile then runs the full-tile
path in a wave that is not ``wave_full`` and the per-vector fallback side by side), and
``M = nvec * L + (L - 1)`` so the scalar remainder runs as well; both sides of every ``nvec`` and
client-count threshold; one grid-capped launch per shape (a workgroup walks several tiles); a
chain / push continuation of an accumulator (``first == 0``).

The three kernels of the tile-interleaved layout (``fedagg_fedavg_tiled_<kind>``,
``fedagg_fedavg_chain_tiled_<kind>``) get the same family per (tile, client count), at two tiles
plus the remainder, with a grid cap of 3 over five tiles (two workgroups walk a second tile, so
``t * pitch`` counts for ``it > 0``), the numel == 1 indices fused and through the separate
gather / tree path with its tiled index map, and the smallest buckets (M = 1, L - 1, L, L + 1,
one tile -1 / 0 / +1).  Their buffer is built from the layout ``include/fedagg.h`` publishes, not
with the engine's layout helpers, and everything in it that is no client's element [0, M) -- the
pad of the last tile, in every client -- is a quiet NaN: one pad read that reaches an output, or a
read from the next client's tile at the wrong pitch, shows.

References
  * fp32 / bf16 / fp64 FedAvg below 1M elements: the oracle (``fedavg_reference_structure``) on
    the exact upcast, the ``numel == 1`` indices as one-element layers; seeded continuations:
    ``acc = seed; acc = acc + x[k] * w[k]`` in NumPy.
  * from 1M elements: torch eager ops on the device, client by client in list order (one rounded
    IEEE operation each); the ``numel == 1`` indices from the oracle on the gathered columns.
  * fp16: NumPy float16 below 1M; above, each step emulated in fp32 on the device (the fp32
    product of two halves is exact, the fp32 sum double-rounds innocuously).  Before a device
    reference is used it is compared with NumPy on a strided sample (>= 2^20 elements for fp16)
    that contains every planted edge value.
  * Scaffold: fp64 NumPy on the exact upcast, ``acc = seed or +0; acc = acc + w[k] * x[k]``, then
    ``lr * acc`` / ``acc + c``; ``numel == 1`` indices by ``numpy_pairwise_sum``.

Inputs carry +-0, the smallest and largest subnormal, the largest finite value, the smallest
normal (its product with a weight is subnormal) and an all -0 column in the first full tile, the
partial tile and the scalar remainder of three clients.  Every output is longer than M and
pre-filled with a sentinel that must survive."""

from __future__ import annotations

import ctypes
from collections import namedtuple

import numpy as np
import pytest

from oracle import fedavg_reference_structure, numpy_pairwise_sum

pytestmark = pytest.mark.gpu

L_OF = {"f32": 4, "bf16": 8, "f16": 8, "f64": 2}
NP_STORE = {"f32": np.uint32, "bf16": np.uint16, "f16": np.uint16, "f64": np.uint64}
BIG = 16 * 256 * 2048  # shape_for: 16 x 2 tiles from this many vectors (K >= 32)
SHORT, MID = 384 * 1024, 768 * 1024  # shape_for: 2 x 8 below SHORT, 4 x 4 below MID (fp32 / bf16, K >= 32)
HOST_REF_MAX = 1_000_000  # below: NumPy / oracle references; from here on: the device reference
K_MAX = 33
RESET = dict(st_sc1=-1, grid_cap=0, sc_2l=-1, fuse_pairwise=1)
DEV = "cuda"

# edge bit patterns per stored kind: +0, -0, smallest / largest subnormal, largest finite,
# smallest normal (times a weight < 1: a subnormal product), -largest subnormal
EDGES = {
    "f32": [0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x7F7FFFFF, 0x00800000, 0x807FFFFF],
    "f16": [0x0000, 0x8000, 0x0001, 0x03FF, 0x7BFF, 0x0400, 0x83FF],
    "bf16": [0x0000, 0x8000, 0x0001, 0x007F, 0x7F7F, 0x0080, 0x807F],
    "f64": [0x0, 0x8000000000000000, 0x1, 0x000FFFFFFFFFFFFF, 0x7FEFFFFFFFFFFFFF, 0x0010000000000000,
            0x800FFFFFFFFFFFFF],
}
NEG_ZERO = {k: v[1] for k, v in EDGES.items()}
PLANT_AT = 16  # element offset of the planted block inside a partial tile

# =============================================================================================
# FedAvg case table
# =============================================================================================
# entry: "main" (fedagg_fedavg_<kind>, takes idx), "chain" (fedagg_fedavg_chain_<kind>, seed = 0:
# continues d_out), "push" (fedagg_fedavg_chain_push_<kind>: system-scope stores; din: "null" from
# +0.0, "sep" continues a separate d_in)
FaCase = namedtuple("FaCase", "id kind K nvec entry st_sc1 grid_cap pw din")


def _fedavg_cases():
    out = []

    def add(kind, shape, store, tag, K, nvec, entry="main", st=-1, cap=0, pw=False, din=None):
        out.append(FaCase(f"fa-{kind}-{shape}-{store}-{tag}", kind, K, nvec, entry, st, cap, pw, din))

    def family(kind, shape, vpt, threads, K, base, cap, stores, big=False):
        """The remainder / grid-cap / continuation cases of one tile for each store build.
        ``base``: a whole number of tiles at which dispatch picks this tile for K clients."""
        tile = vpt * threads
        rbig = (vpt - 1) * threads + 100
        capn = base + 37 if big or base > 4 * tile else 4 * tile + 37
        for store, st in stores:
            if store == "sys":
                add(kind, shape, store, f"K{K}-r0-null", K, base, "push", din="null")
                add(kind, shape, store, f"K{K}-r37-sep", K, base + 37, "push", din="sep")
                add(kind, shape, store, f"K{K}-rbig-sep", K, base + rbig, "push", din="sep")
                add(kind, shape, store, f"K{K}-cap{cap}-null", K, capn, "push", cap=cap, din="null")
                continue
            add(kind, shape, store, f"K{K}-r0", K, base, st=st)
            add(kind, shape, store, f"K{K}-r37-pw", K, base + 37, st=st, pw=True)
            add(kind, shape, store, f"K{K}-rbig", K, base + rbig, st=st)
            add(kind, shape, store, f"K{K}-cap{cap}", K, capn, st=st, cap=cap, pw=True)
            add(kind, shape, store, f"K{K}-r37-chain", K, base + 37, "chain", st=st)

    for kind in ("f32", "bf16"):
        big_threads = 512 if kind == "f32" else 256  # fp32: 16 x 512 threads; bf16: 16 x 256 over buffer loads
        many = [("nt", -1), ("sc1", 1), ("sys", -1)]  # K >= 32: automatic stores are nt
        few = [("sc1", -1), ("nt", 0), ("sys", -1)]  # K < 32: automatic stores are sc1
        family(kind, "2x8", 2, 256, 33, 2 * 512, 3, many)
        family(kind, "4x4", 4, 256, 33, SHORT, 100, many)  # r0: the first nvec of the 4 x 4 range
        family(kind, "8x4", 8, 256, 33, MID, 100, many)  # r0: the first nvec of the 8 x 4 range
        family(kind, "8x4", 8, 256, 5, 2 * 2048, 3, few)
        family(kind, "16x2", 16, big_threads, 33, BIG, 500, many, big=True)  # r0: the threshold itself
        # the last nvec below each threshold
        add(kind, "2x8", "nt", "K33-below-short", 33, SHORT - 1, pw=True)
        add(kind, "4x4", "nt", "K33-below-mid", 33, MID - 1, pw=True)
        add(kind, "8x4", "nt", "K33-below-big", 33, BIG - 1, pw=True)
        add(kind, "8x4", "sc1", "K33-below-big", 33, BIG - 1, st=1)
        # the client-count threshold at one M: 31 clients take the 8 x 4 tile with sc1 stores
        add(kind, "8x4", "sc1", "K31-at-short-M", 31, 2 * 512 + 37, pw=True)
        add(kind, "2x8", "nt", "K32-at-short-M", 32, 2 * 512 + 37, pw=True)
        add(kind, "8x4", "sc1", "K8-r37-pw", 8, 2 * 2048 + 37, pw=True)
        add(kind, "8x4", "nt", "K8-rbig", 8, 2 * 2048 + 7 * 256 + 100, st=0)
        add(kind, "8x4", "sys", "K8-r37-sep", 8, 2 * 2048 + 37, "push", din="sep")

    # fp16: 4 x 4 everywhere below the 16 x 2 threshold; no push entry
    family("f16", "4x4", 4, 256, 5, 2 * 1024, 3, [("sc1", -1), ("nt", 0)])
    family("f16", "4x4", 4, 256, 33, 2 * 1024, 3, [("nt", -1), ("sc1", 1)])
    family("f16", "16x2", 16, 256, 33, BIG, 500, [("nt", -1), ("sc1", 1)], big=True)
    add("f16", "4x4", "nt", "K33-below-big", 33, BIG - 1, pw=True)
    add("f16", "4x4", "sc1", "K33-below-big", 33, BIG - 1, st=1)
    add("f16", "4x4", "sc1", "K31-at-big-M", 31, BIG + 37, pw=True)
    add("f16", "16x2", "nt", "K32-at-big-M", 32, BIG + 37, pw=True)
    add("f16", "4x4", "sc1", "K8-r37-pw", 8, 2 * 1024 + 37, pw=True)
    # fp64: the pipelined 4 x 4 tile always
    family("f64", "4x4p", 4, 256, 5, 2 * 1024, 3, [("sc1", -1), ("nt", 0)])
    family("f64", "4x4p", 4, 256, 33, 2 * 1024, 3, [("nt", -1), ("sc1", 1)])
    add("f64", "4x4p", "sc1", "K8-r37-pw", 8, 2 * 1024 + 37, pw=True)
    add("f64", "4x4p", "sc1", "K31-r37", 31, 2 * 1024 + 37, pw=True)
    add("f64", "4x4p", "nt", "K32-r37", 32, 2 * 1024 + 37, pw=True)
    return out


FEDAVG_CASES = _fedavg_cases()


# =============================================================================================
# Tile-interleaved FedAvg case table (fedagg_fedavg_tiled_<kind>, fedagg_fedavg_chain_tiled_<kind>)
# =============================================================================================
# The three tiled kernels: (kind, tile T in 16-B vectors, vectors per thread, threads, store build,
# client counts).  The entry points take any K with any of their tiles; K <= 128 keeps a case one
# fedavg_kernel launch.  entry: "main" (engine.TiledFedAvgPlan, takes idx), "chain" (seed = 0:
# continues d_out).  fuse: the fuse_pairwise knob (0: separate gather / tree with the tiled map).
TILED_TILES = (("f32", 8192, 16, 512, "nt", (33, 5)),
               ("f32", 2048, 8, 256, "sc1", (5, 33)),
               ("bf16", 4096, 16, 256, "nt", (33, 5)))
TdCase = namedtuple("TdCase", "id kind K nvec entry grid_cap pw fuse tile")
# quiet NaNs in everything of the tiled buffer that is no client's element [0, M)
POISON = {"f32": 0x7FC5A5A5, "bf16": 0x7FC5}
# The fp32 poison is the output sentinel's pattern, and a NaN keeps its payload through x * w and
# acc + p: a pad element that reached the guard band would put the sentinel back.  The tiled cases
# guard their outputs with another quiet NaN.
TILED_GUARD = 0x7FE1B2B2


def _tiled_cases():
    out = []
    for kind, tile, vpt, threads, store, Ks in TILED_TILES:
        def add(K, tag, nvec, entry="main", cap=0, pw=False, fuse=1):
            out.append(TdCase(f"fa-{kind}-tiled{tile}-{store}-K{K}-{tag}", kind, K, nvec, entry, cap, pw, fuse, tile))

        for K in Ks:
            add(K, "r0", 2 * tile)
            add(K, "r37-pw", 2 * tile + 37, pw=True)
            add(K, "rbig", 2 * tile + (vpt - 1) * threads + 100)
            add(K, "cap3-pw", 4 * tile + 37, cap=3, pw=True)  # five tiles over three workgroups
            add(K, "r37-chain", 2 * tile + 37, "chain")
        add(Ks[0], "r37-unfused", 2 * tile + 37, pw=True, fuse=0)
    return out


def _tiled_small_cases():
    """The smallest buckets: everything scalar remainder (M < L), one vector, one tile and its
    neighbours.  nvec is not used: M is given."""
    out = []
    for kind, tile, vpt, threads, store, Ks in TILED_TILES:
        L = L_OF[kind]
        for K in (1, 5):
            for tag, M in (("M1", 1), ("Lm1", L - 1), ("L", L), ("Lp1", L + 1), ("TLm1", tile * L - 1),
                           ("TL", tile * L), ("TLp1", tile * L + 1)):
                out.append((f"fa-{kind}-tiled{tile}-{store}-K{K}-small-{tag}", kind, tile, K, M))
    return out


TILED_CASES = _tiled_cases()
TILED_SMALL_CASES = _tiled_small_cases()


def _tile_of(c) -> int:
    if isinstance(c, TdCase):
        return c.tile
    shape = c.id.split("-")[2]
    vpt = int(shape.split("x")[0])
    return vpt * (512 if (c.kind == "f32" and vpt == 16) else 256)


def _M(c) -> int:
    return c.nvec * L_OF[c.kind] + L_OF[c.kind] - 1


def _pw_idx(c: FaCase):
    """Four fused numel == 1 indices: element 0, inside a full tile, inside the partial tile (the
    last full tile when r = 0), M - 1 in the scalar remainder.  Neighbours are >= 2 apart."""
    L, tile, M = L_OF[c.kind], _tile_of(c), _M(c)
    n_full = c.nvec // tile
    in_full = (tile // 2 + 3) * L + 1
    in_part = (n_full * tile + 5) * L + 2 if c.nvec % tile else ((n_full - 1) * tile + tile // 2 + 9) * L + 2
    return [0, in_full, in_part, M - 1]


# =============================================================================================
# Scaffold case table
# =============================================================================================
# entry: "two" (fedagg_scaffold_<kind>: both buckets; sc_2l 0 = scaffold_kernel, -1 = automatic),
# "push" (fedagg_scaffold_chain_push_<kind>: one bucket, phase / finish / d_in), "bucket"
# (fedagg_scaffold_bucket: scaffold_rows_kernel).  off: every operand one element off 16-B
# alignment (the scalar walk).
ScCase = namedtuple("ScCase", "id kind K nvec entry sc_2l grid_cap pw off phase finish din")


def _scaffold_cases():
    out = []

    def add(name, tag, kind, K, nvec, entry, sc_2l=-1, cap=0, pw=False, off=0, phase=0, finish=1, din=None):
        out.append(ScCase(f"sc-{name}-{tag}", kind, K, nvec, entry, sc_2l, cap, pw, off, phase, finish, din))

    def rems(vpt):
        tile = vpt * 256
        return tile, [("r0", 2 * tile), ("r37", 2 * tile + 37), ("rbig", 2 * tile + (vpt - 1) * 256 + 100)]

    # scaffold_kernel: fp32 4 x 4 (K < 16), fp32 8 x 4 over buffer loads and fp64 8 x 2 (K >= 32), fp64 4 x 4
    for name, kind, vpt, Ks in (("two-f32-4x4", "f32", 4, (5,)), ("two-f32-8x4buf", "f32", 8, (33,)),
                                ("two-f64-4x4", "f64", 4, (5,)), ("two-f64-8x2", "f64", 8, (33,))):
        tile, rs = rems(vpt)
        for K in Ks:
            sc_2l = -1 if (kind == "f32" and K < 16) else 0
            for tag, nvec in rs:
                add(name, f"K{K}-{tag}", kind, K, nvec, "two", sc_2l, pw=(tag == "r37"))
            add(name, f"K{K}-cap3", kind, K, 4 * tile + 37, "two", sc_2l, cap=3, pw=True)
            if K >= 32:  # what these two kernels serve by default: the scalar walk of unaligned operands
                add(name, f"K{K}-unaligned", kind, K, 2 * tile + 37, "two", -1, off=1, pw=True)
    # scaffold_bucket_kernel PH 0 / 1 (one call launches both): from 16 clients (fp32), always (fp64)
    for name, kind, vpt in (("bucket2l-f32", "f32", 8), ("bucket2l-f64", "f64", 4)):
        tile, rs = rems(vpt)
        for K in (17, 65):  # 65: the 64-client chunk seam
            for tag, nvec in rs:
                add(name, f"K{K}-{tag}", kind, K, nvec, "two", -1, pw=(tag == "r37"))
        add(name, "K17-cap3", kind, 17, 4 * tile + 37, "two", -1, cap=3, pw=True)
    # scaffold_push_kernel: phase x separate-input builds for fp32 (8 x 4) and fp64 (pipelined 4 x 2)
    for kind, vpt in (("f32", 8), ("f64", 4)):
        tile, rs = rems(vpt)
        for phase in (0, 1):
            for din in ("null", "sep"):
                name = f"push-{kind}-ph{phase}-{din}"
                add(name, "K9-r0-finish", kind, 9, rs[0][1], "push", phase=phase, finish=1, din=din)
                add(name, "K9-r37-sums", kind, 9, rs[1][1], "push", phase=phase, finish=0, din=din)
                add(name, "K9-rbig-finish", kind, 9, rs[2][1], "push", phase=phase, finish=1, din=din)
                add(name, "K65-r37-finish", kind, 65, rs[1][1], "push", phase=phase, finish=1, din=din)
                add(name, "K9-cap3-sums", kind, 9, 4 * tile + 37, "push", cap=3, phase=phase, finish=0, din=din)
    # scaffold_rows_kernel for fp32 / fp64 rows (fedagg_scaffold_bucket); the 16-bit kinds are
    # pinned to the same NumPy form by test_scaffold16_kernel_gpu.py
    for kind, vpt in (("f32", 8), ("f64", 4)):
        tile, rs = rems(vpt)
        for phase in (0, 1):
            name = f"rows-{kind}"
            for tag, nvec in rs:
                add(name, f"ph{phase}-K5-{tag}", kind, 5, nvec, "bucket", pw=(tag == "r37"), phase=phase)
            add(name, f"ph{phase}-K65-r37", kind, 65, rs[1][1], "bucket", pw=True, phase=phase)
            add(name, f"ph{phase}-K5-cap3", kind, 5, 4 * tile + 37, "bucket", cap=3, phase=phase)
            add(name, f"ph{phase}-K5-unaligned", kind, 5, rs[1][1], "bucket", off=1, phase=phase)
    return out


SCAFFOLD_CASES = _scaffold_cases()
# the read-stream probes and the fp64 flat gather: no reduction, but shipped and launched nowhere else
MISC_CASES = ["misc-read-probe-stream", "misc-read-probe-tile-4", "misc-read-probe-tile-8", "misc-read-probe-tile-16",
              "misc-flat-gather-f64"]
CASE_IDS = ([c.id for c in FEDAVG_CASES] + [c.id for c in SCAFFOLD_CASES] + MISC_CASES
            + [c.id for c in TILED_CASES] + [c[0] for c in TILED_SMALL_CASES])
assert len(set(CASE_IDS)) == len(CASE_IDS)


# =============================================================================================
# helpers
# =============================================================================================
def _sync(torch):
    torch.cuda.synchronize()


def _torch_dtype(torch, kind):
    return {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}[kind]


def _int_dtype(torch, kind_or_bytes):
    n = kind_or_bytes if isinstance(kind_or_bytes, int) else {"f32": 4, "bf16": 2, "f16": 2, "f64": 8}[kind_or_bytes]
    return {2: torch.int16, 4: torch.int32, 8: torch.int64}[n]


def _signed(bits: int, nbytes: int) -> int:
    return bits - (1 << (8 * nbytes)) if bits >= 1 << (8 * nbytes - 1) else bits


def _plant_block(kind: str, K: int, n: int, rot: int) -> np.ndarray:
    """[K, n] stored bit patterns: rows 0-2 carry the edge values, rotated so that a column never
    holds the same edge twice (the other rows are zero and not used)."""
    e = EDGES[kind]
    blk = np.zeros((K, n), NP_STORE[kind])
    for j in range(n):
        for c in range(min(3, K)):
            blk[c, j] = e[(j + 3 * c + rot) % len(e)]
    return blk


def _plant(torch, rows, kind: str, pos: int, n: int, rot: int, all_neg_zero_last: bool):
    """Edge values for clients 0-2 at elements [pos, pos + n) of the shared rows; the last of them
    an all -0 column when asked."""
    if n <= 0:
        return
    nb = rows.element_size()
    iv = rows.view(_int_dtype(torch, nb))
    blk = _plant_block(kind, 3, n, rot).view({2: np.int16, 4: np.int32, 8: np.int64}[nb])
    iv[:3, pos: pos + n] = torch.from_numpy(blk).to(rows.device)
    if all_neg_zero_last:
        iv[:, pos + n - 1] = _signed(NEG_ZERO[kind], nb)


def _planted_positions(kind: str, nvec: int, tile: int):
    """(pos, n, all -0 last) of the planted blocks for one bucket length: first full tile, partial
    tile, scalar remainder."""
    L = L_OF[kind]
    n_e = len(EDGES[kind]) + 1
    spots = [(L * 3 + 1, n_e, True)]
    if nvec % tile:
        spots.append(((nvec // tile) * tile * L + PLANT_AT, min(n_e, (nvec % tile) * L - PLANT_AT), True))
    spots.append((nvec * L, L - 1, L - 1 >= 3 or nvec % 2 == 1))
    return spots


class _Rows:
    """The client rows of one kind, allocated once at the largest M any case of that kind uses
    (M is a launch argument, the row pitch stays) and never changed after planting."""

    def __init__(self, torch, kind: str, cases):
        self.kind = kind
        self.max_M = max(_M(c) for c in cases)
        self.pitch = (self.max_M + 64 + 63) // 64 * 64
        dt = _torch_dtype(torch, kind)
        self.x = torch.empty((K_MAX, self.pitch), dtype=dt, device=DEV)
        g = torch.Generator(device=DEV).manual_seed(20 + len(kind))
        for k in range(K_MAX):
            self.x[k].copy_(torch.randn(self.pitch, generator=g, device=DEV, dtype=torch.float32))
        self.planted = set()
        for nvec, tile in sorted({(c.nvec, _tile_of(c)) for c in cases}):
            for pos, n, zero in _planted_positions(kind, nvec, tile):
                _plant(torch, self.x, kind, pos, n, nvec % 7, zero)
                self.planted.update(range(pos, pos + n))
        rng = np.random.default_rng(len(kind))
        self.ns = [int(v) for v in rng.integers(100, 10000, K_MAX)]
        _sync(torch)
        self.reference_checked = None  # None: not yet; else the failure message ("" = fine)


@pytest.fixture(scope="module")
def fedavg_rows():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    held = {}

    def get(kind):
        if kind not in held:
            held[kind] = _Rows(torch, kind, [c for c in FEDAVG_CASES + TILED_CASES if c.kind == kind])
        return held[kind]

    yield get
    held.clear()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _restore_knobs():
    from substrafl_amd import _native

    try:
        yield
    finally:
        _native.tune(**RESET)


# ---------------------------------------------------------------------------------------------
# FedAvg references
# ---------------------------------------------------------------------------------------------
def _upcast_np(a_stored: np.ndarray, kind: str) -> np.ndarray:
    """Stored bits -> the NumPy array the reference computes on (bf16: its exact fp32 upcast)."""
    if kind == "bf16":
        return (a_stored.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return a_stored.view({"f32": np.float32, "f16": np.float16, "f64": np.float64}[kind])


def _host_rows(torch, x, kind, K, cols) -> np.ndarray:
    """[K, len(cols) or M] rows on the host as the reference's dtype; ``cols``: int (first M
    elements) or an index tensor."""
    iv = x.view(_int_dtype(torch, x.element_size()))
    sub = iv[:K, :cols] if isinstance(cols, int) else iv[:K][:, cols]
    return _upcast_np(np.ascontiguousarray(sub.cpu().numpy()).view(NP_STORE[kind]), kind)


def _np_sequential(xs: np.ndarray, w: np.ndarray, seed):
    """acc = seed or +0.0; acc = fl(acc + fl(x[k] * w[k])) in the dtype of ``xs`` (NumPy rounds
    every float16 operation once)."""
    with np.errstate(all="ignore"):
        acc = np.zeros(xs.shape[1], xs.dtype) if seed is None else seed.astype(xs.dtype).copy()
        for k in range(xs.shape[0]):
            acc = acc + xs[k] * w[k]
    assert acc.dtype == xs.dtype
    return acc


def _oracle_layers(xs: np.ndarray, ns, idx):
    """The oracle over [K, M] rows cut into layers, each index of ``idx`` a one-element layer."""
    M = xs.shape[1]
    cuts, pos = [], 0
    for i in sorted(idx):
        assert i == 0 or i - pos >= 2 or i == pos, "a layer between two numel == 1 indices needs >= 2 elements"
        if i > pos:
            cuts.append((pos, i))
        cuts.append((i, i + 1))
        pos = i + 1
    if M > pos:
        assert M - pos >= 2
        cuts.append((pos, M))
    pus = [[xs[k, a:b] for a, b in cuts] for k in range(xs.shape[0])]
    with np.errstate(all="ignore"):
        return np.concatenate([np.asarray(r).ravel() for r in fedavg_reference_structure(pus, ns)])


def _device_sequential(torch, x, kind, K, M, w, seed):
    """Torch eager ops on the device, client by client in list order, one rounded IEEE operation
    each; fp16: every step emulated in fp32 (exact product, innocuous double rounding of the sum)."""
    if kind == "f16":
        acc = torch.zeros(M, dtype=torch.float16, device=DEV) if seed is None else seed.clone()
        for k in range(K):
            wk = torch.tensor(float(w[k]), dtype=torch.float32, device=DEV)
            p = (x[k, :M].float() * wk).half()
            acc = (acc.float() + p.float()).half()
        return acc
    P = torch.float64 if kind == "f64" else torch.float32
    acc = torch.zeros(M, dtype=P, device=DEV) if seed is None else seed.clone()
    for k in range(K):
        wk = torch.tensor(float(w[k]), dtype=P, device=DEV)
        acc = acc + x[k, :M].to(P) * wk
    return acc


def _check_device_reference(torch, rows: _Rows):
    """The device reference against NumPy on a strided sample of the shared rows (all 33 clients)
    that contains every planted element: >= 2^20 elements for fp16, 2^16 otherwise.  Run once per
    kind, before the first use of the device reference; a failure here blames the reference."""
    from substrafl_amd.engine import fedavg_weights

    if rows.reference_checked is None:
        kind, M = rows.kind, rows.max_M
        want = (1 << 20) if kind == "f16" else (1 << 16)
        stride = max(1, M // want)
        stride -= 1 - stride % 2 if stride > 1 else 0  # odd: every lane and vector slot turns up
        cols = np.unique(np.concatenate([np.arange(0, M, stride), np.array(sorted(rows.planted))]))
        assert cols.size >= min(want, M)
        tc = torch.from_numpy(cols).to(DEV)
        w = fedavg_weights(rows.ns, kind)
        sample = rows.x[:, tc].contiguous()
        msgs = []
        odt = {"f16": torch.float16, "f64": torch.float64}.get(kind, torch.float32)
        for seeded in (False, True):
            seed_np = seed_t = None
            if seeded:
                seed_t = (sample[K_MAX - 1].to(odt) * 0.25).contiguous()
                seed_t[:8] = -0.0
                seed_np = seed_t.cpu().numpy()
            dev = _device_sequential(torch, sample, kind, K_MAX, cols.size, w, seed_t).cpu().numpy()
            ref = _np_sequential(_host_rows(torch, sample, kind, K_MAX, cols.size), w, seed_np)
            bad = np.flatnonzero(_bits(dev) != _bits(ref))
            if bad.size:
                msgs.append(f"seeded={seeded}: {bad.size} of {cols.size} sampled elements differ, first at element "
                            f"{cols[bad[:4]]}: device {dev[bad[:4]]} NumPy {ref[bad[:4]]}")
        rows.reference_checked = "; ".join(msgs)
    assert rows.reference_checked == "", (f"device reference disagrees with NumPy ({rows.kind}): "
                                          f"{rows.reference_checked}")


def _bits(a):
    a = np.asarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


SENTINEL = {2: 0x7E5A, 4: 0x7FC5A5A5, 8: 0x7FF8A5A5A5A5A5A5}  # quiet NaN patterns
GUARD = 64


def _sentinel_buffer(torch, n: int, dtype, pattern=None):
    nb = torch.empty(0, dtype=dtype).element_size()
    pattern = SENTINEL[nb] if pattern is None else pattern
    return torch.full((n + GUARD,), pattern, dtype=_int_dtype(torch, nb), device=DEV).view(dtype)


def _assert_guard(torch, buf, n: int, what: str, pattern=None):
    nb = buf.element_size()
    tail = buf.view(_int_dtype(torch, nb))[n:]
    hit = torch.nonzero(tail != (SENTINEL[nb] if pattern is None else pattern)).flatten()
    assert hit.numel() == 0, (f"{what}: elements at and beyond M were written, first at M + {int(hit[0])}: "
                              f"{buf[n + int(hit[0])].item()!r}")


def _assert_equal_bits(torch, got, ref, what: str):
    iv = _int_dtype(torch, got.element_size())
    assert got.dtype == ref.dtype, (got.dtype, ref.dtype)
    g, r = got.view(iv), ref.view(iv)
    if not torch.equal(g, r):
        bad = torch.nonzero(g != r).flatten()
        i = bad[:6].cpu().numpy()
        raise AssertionError(f"{what}: {bad.numel()} of {g.numel()} elements differ; first at {i}: got "
                             f"{got[bad[:6]].cpu().numpy()} reference {ref[bad[:6]].cpu().numpy()}")


# =============================================================================================
# FedAvg
# =============================================================================================
@pytest.mark.parametrize("case", FEDAVG_CASES, ids=[c.id for c in FEDAVG_CASES])
def test_fedavg_product_kernel(case, fedavg_rows):
    import torch

    from substrafl_amd import _native
    from substrafl_amd.engine import FedAvgPlan, fedavg_weights

    lib = _native.load()
    rows = fedavg_rows(case.kind)
    kind, K, M = case.kind, case.K, _M(case)
    x = rows.x[:K]
    ns = rows.ns[:K]
    w = fedavg_weights(ns, kind)
    odt = {"f16": torch.float16, "f64": torch.float64}.get(kind, torch.float32)
    idx = _pw_idx(case) if case.pw else []
    assert case.entry == "main" or not idx

    # the accumulator a chain / push call continues: a partial sum of other rows, -0 in front
    seed = None
    if case.entry == "chain" or case.din == "sep":
        seed = (rows.x[K_MAX - 1, :M].to(odt) * 0.25).contiguous()
        seed[:8] = -0.0
    out = _sentinel_buffer(torch, M, odt)
    d_in = None
    if case.entry == "chain":
        out[:M] = seed
    elif case.din == "sep":
        d_in = _sentinel_buffer(torch, M, odt)
        d_in[:M] = seed
    _sync(torch)

    _native.tune(st_sc1=case.st_sc1, grid_cap=case.grid_cap)
    try:
        if case.entry == "main":
            FedAvgPlan(kind, x, w, M, out, idx).launch()
        else:
            ptrs = _native.ptr_array([x.data_ptr() + k * rows.pitch * x.element_size() for k in range(K)])
            if kind == "f16":
                cw = (ctypes.c_uint16 * K)(*[int(v) for v in np.asarray(w, np.float16).view(np.uint16)])
            elif kind == "f64":
                cw = (ctypes.c_double * K)(*[float(v) for v in w])
            else:
                cw = (ctypes.c_float * K)(*[float(v) for v in w])
            if case.entry == "chain":
                rc = getattr(lib, f"fedagg_fedavg_chain_{kind}")(ptrs, cw, K, M, 0, out.data_ptr(), None)
            else:
                rc = getattr(lib, f"fedagg_fedavg_chain_push_{kind}")(ptrs, cw, K, M,
                                                                      d_in.data_ptr() if d_in is not None else None,
                                                                      out.data_ptr(), None)
            assert rc == 0, lib.fedagg_last_error()
        _sync(torch)
    finally:
        _native.tune(**RESET)

    if M < HOST_REF_MAX:
        xs = _host_rows(torch, x, kind, K, M)
        if seed is None:
            ref_np = _oracle_layers(xs, ns, idx)
        else:
            ref_np = _np_sequential(xs, w, seed.cpu().numpy())
        ref = torch.from_numpy(np.ascontiguousarray(ref_np)).to(DEV)
    else:
        _check_device_reference(torch, rows)
        ref = _device_sequential(torch, x, kind, K, M, w, seed)
        if idx:  # the numel == 1 elements: NumPy's pairwise order, from the oracle on the gathered columns
            cols = _host_rows(torch, x, kind, K, torch.tensor(idx, device=DEV))
            with np.errstate(all="ignore"):
                pw = fedavg_reference_structure([[cols[k, p: p + 1] for p in range(len(idx))] for k in range(K)], ns)
            ref[torch.tensor(idx, device=DEV)] = torch.from_numpy(np.concatenate(pw)).to(DEV)
    assert ref.dtype == odt and ref.numel() == M
    _assert_equal_bits(torch, out[:M], ref, case.id)
    _assert_guard(torch, out, M, case.id)
    if d_in is not None:  # the separate input is read, never written
        _assert_equal_bits(torch, d_in[:M], seed, case.id + " (d_in)")
        _assert_guard(torch, d_in, M, case.id + " (d_in)")
    # an all -0 column sums to +0.0 (the accumulator starts from +0.0)
    if seed is None:
        xi = x.view(_int_dtype(torch, x.element_size()))
        checked = 0
        for pos, n, zero in _planted_positions(kind, case.nvec, _tile_of(case)):
            col = pos + n - 1
            # (another bucket length's block may have been planted over this column since)
            neg0 = _signed(NEG_ZERO[kind], x.element_size())
            if zero and n > 0 and col not in idx and bool((xi[:, col] == neg0).all()):
                assert int(out.view(_int_dtype(torch, out.element_size()))[col]) == 0, (case.id, col)
                checked += 1
        assert checked, "no all -0 column left in this case's inputs"


# =============================================================================================
# FedAvg over tile-interleaved buckets
# =============================================================================================
def _tiled_buffer(torch, kind: str, xi, K: int, M: int, T: int):
    """The layout include/fedagg.h publishes, restated: tile t of client k at 16-B vector
    (t * K + k) * T of the buffer, every tile T vectors, the last one padded -- a [tiles, K, T * L]
    array whose [:, k, :] holds client k.  ``xi``: [>= K, >= M] stored bit patterns on the device.
    Only elements [0, M) of each client are copied in; the rest of the last tile, in every client,
    stays a quiet NaN, so one pad read that reaches an output turns it NaN."""
    L = L_OF[kind]
    TL = T * L
    tiles = -(-(-(-M // L)) // T)
    nb = xi.element_size()
    buf = torch.full((tiles * K * TL,), POISON[kind], dtype=_int_dtype(torch, nb), device=DEV)
    view = buf.view(tiles, K, TL)
    n_full = M // TL
    for k in range(K):
        if n_full:
            view[:n_full, k, :] = xi[k, : n_full * TL].view(n_full, TL)
        if M % TL:
            view[n_full, k, : M % TL] = xi[k, n_full * TL: M]
    assert int((buf == POISON[kind]).sum()) >= K * (tiles * TL - M)
    return buf


def _c_weights(w, K):
    return (ctypes.c_float * K)(*[float(v) for v in w])


@pytest.mark.parametrize("case", TILED_CASES, ids=[c.id for c in TILED_CASES])
def test_fedavg_tiled_product_kernel(case, fedavg_rows):
    import torch

    from substrafl_amd import _native
    from substrafl_amd.engine import TiledFedAvgPlan, fedavg_weights

    lib = _native.load()
    rows = fedavg_rows(case.kind)
    kind, K, M, T = case.kind, case.K, _M(case), case.tile
    x = rows.x[:K]
    ns = rows.ns[:K]
    w = fedavg_weights(ns, kind)
    idx = _pw_idx(case) if case.pw else []
    assert case.entry == "main" or not idx
    assert M < HOST_REF_MAX and K <= _native.FEDAGG_KCHUNK  # host references; one fedavg_kernel launch
    if idx:
        assert (idx[2] // L_OF[kind]) // T >= 1  # a numel == 1 index behind tile 0: its place depends on K
    buf = _tiled_buffer(torch, kind, x.view(_int_dtype(torch, x.element_size())), K, M, T)

    seed = None
    out = _sentinel_buffer(torch, M, torch.float32, TILED_GUARD)
    if case.entry == "chain":  # the accumulator the call continues: a partial sum of other rows, -0 in front
        seed = (rows.x[K_MAX - 1, :M].to(torch.float32) * 0.25).contiguous()
        seed[:8] = -0.0
        out[:M] = seed
        _assert_equal_bits(torch, out[:M], seed, case.id + " (seed)")
    ws = None
    if idx and not case.fuse:
        ws = torch.empty(max(16, lib.fedagg_pairwise_ws_bytes(K, len(idx), 8)), dtype=torch.uint8, device=DEV)
    _sync(torch)

    _native.tune(grid_cap=case.grid_cap, fuse_pairwise=case.fuse)
    try:
        if case.entry == "main":
            TiledFedAvgPlan(kind, buf, K, w, M, out, idx, ws, tv=T).launch()
        else:
            rc = getattr(lib, f"fedagg_fedavg_chain_tiled_{kind}")(buf.data_ptr(), _c_weights(w, K), K, M, T, 0,
                                                                   out.data_ptr(), None)
            assert rc == 0, lib.fedagg_last_error()
        _sync(torch)
    finally:
        _native.tune(**RESET)

    xs = _host_rows(torch, x, kind, K, M)
    if seed is None:
        ref_np = _oracle_layers(xs, ns, idx)
    else:
        ref_np = _np_sequential(xs, w, seed.cpu().numpy())
    ref = torch.from_numpy(np.ascontiguousarray(ref_np)).to(DEV)
    assert ref.dtype == torch.float32 and ref.numel() == M and not bool(torch.isnan(ref).any())
    _assert_equal_bits(torch, out[:M], ref, case.id)
    _assert_guard(torch, out, M, case.id, TILED_GUARD)
    if seed is None:  # an all -0 column sums to +0.0 (the accumulator starts from +0.0)
        xi = x.view(_int_dtype(torch, x.element_size()))
        neg0 = _signed(NEG_ZERO[kind], x.element_size())
        checked = 0
        for pos, n, zero in _planted_positions(kind, case.nvec, T):
            col = pos + n - 1
            if zero and n > 0 and col not in idx and bool((xi[:, col] == neg0).all()):
                assert int(out.view(torch.int32)[col]) == 0, (case.id, col)
                checked += 1
        assert checked, "no all -0 column left in this case's inputs"


@pytest.mark.parametrize("case", TILED_SMALL_CASES, ids=[c[0] for c in TILED_SMALL_CASES])
def test_fedavg_tiled_smallest_buckets(case):
    """M = 1, L - 1 (no vector at all: one workgroup, everything scalar remainder), L, L + 1 and
    one tile -1 / 0 / +1 elements, for 1 and 5 clients, against NumPy in client order; from three
    elements on, M - 1 is a numel == 1 index (the oracle)."""
    import torch

    from substrafl_amd import _native
    from substrafl_amd.engine import TiledFedAvgPlan, fedavg_weights

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    cid, kind, T, K, M = case
    rng = np.random.default_rng(sum(map(ord, cid)))
    stored = rng.standard_normal((K, M)).astype(np.float32).view(np.uint32)
    if kind == "bf16":
        stored = (stored >> np.uint32(16)).astype(np.uint16)
    n_e = min(M, len(EDGES[kind]))
    stored[: min(3, K), :n_e] = _plant_block(kind, 3, n_e, M % 7)[: min(3, K)]
    stored = np.ascontiguousarray(stored)
    ns = [int(v) for v in rng.integers(100, 10000, K)]
    w = fedavg_weights(ns, kind)
    idx = [M - 1] if M >= 3 else []
    xi = torch.from_numpy(stored.view({2: np.int16, 4: np.int32}[stored.itemsize])).to(DEV)
    buf = _tiled_buffer(torch, kind, xi, K, M, T)
    out = _sentinel_buffer(torch, M, torch.float32, TILED_GUARD)
    _sync(torch)
    TiledFedAvgPlan(kind, buf, K, w, M, out, idx, tv=T).launch()
    _sync(torch)

    xs = _upcast_np(stored, kind)
    ref_np = _np_sequential(xs, w, None)
    if idx:
        ref_np[M - 1] = _oracle_layers(xs, ns, idx)[M - 1]
    assert ref_np.dtype == np.float32 and not np.isnan(ref_np).any()
    _assert_equal_bits(torch, out[:M], torch.from_numpy(ref_np).to(DEV), cid)
    _assert_guard(torch, out, M, cid, TILED_GUARD)


# =============================================================================================
# Scaffold
# =============================================================================================
def _sc_inputs(case: ScCase, rng):
    """Host rows [K, M] of both buckets, c [M] and the weights; edge values planted as for FedAvg
    (first tile, partial tile, scalar remainder; three clients; c carries -0 and the edges too)."""
    kind, K = case.kind, case.K
    L, M = L_OF[kind], _M(case)
    ft = np.float32 if kind == "f32" else np.float64
    vpt = {"f32": 8, "f64": 4}[kind]
    if case.id.startswith("sc-two-f32-4x4") or case.id.startswith("sc-two-f64-8x2"):
        vpt = 4 if kind == "f32" else 8
    tile = vpt * 256
    d = rng.standard_normal((K, M)).astype(ft)
    cv = rng.standard_normal((K, M)).astype(ft)
    c = rng.standard_normal(M).astype(ft)
    for pos, n, zero in _planted_positions(kind, case.nvec, tile):
        for a, rot in ((d, 0), (cv, 2)):
            blk = _plant_block(kind, K, n, rot + case.nvec % 7)
            a.view(NP_STORE[kind])[: min(3, K), pos: pos + n] = blk[: min(3, K)]
            if zero and n > 0:
                a.view(NP_STORE[kind])[:, pos + n - 1] = NEG_ZERO[kind]
        if n > 0:
            c.view(NP_STORE[kind])[pos: pos + n] = _plant_block(kind, 1, n, 4)[0]
            c.view(NP_STORE[kind])[pos + n - 1] = NEG_ZERO[kind]
    n_s = rng.integers(1, 5000, K)
    w = (n_s / np.sum(n_s)).astype(np.float64)
    return d, cv, c, w, tile


def _sc_reference(rows, w, phase, c, lr, idx, seed, finish):
    """fp64 NumPy: acc = seed or +0.0; acc = acc + w[k] * x[k]; finish: lr * acc (phase 0) or
    acc + c (phase 1); numel == 1 indices: NumPy's pairwise order over K (K + 1, c last) terms."""
    with np.errstate(all="ignore"):
        x = rows.astype(np.float64)
        acc = np.zeros(x.shape[1], np.float64) if seed is None else seed.copy()
        for k in range(x.shape[0]):
            acc = acc + w[k] * x[k]
        if not finish:
            assert not len(idx)
            return acc
        c64 = c.astype(np.float64) if phase == 1 else None
        out = np.float64(lr) * acc if phase == 0 else acc + c64
        for e in idx:
            terms = [w[k] * x[k, e] for k in range(x.shape[0])] + ([c64[e]] if phase == 1 else [])
            s = np.float64(0.0) + numpy_pairwise_sum(np.array(terms, np.float64))
            out[e] = np.float64(lr) * s if phase == 0 else s
    return out


def _dev_rows(torch, a: np.ndarray, off: int):
    """Device copy of host rows [K, M], every row 16-B aligned plus ``off`` elements."""
    K, M = a.shape
    ld = (M + off + 15) // 16 * 16
    host = np.zeros((K, ld), a.dtype)
    host[:, off: off + M] = a
    t = torch.from_numpy(host).to(DEV)
    return t, [t.data_ptr() + (k * ld + off) * a.dtype.itemsize for k in range(K)]


def _sc_out(torch, M: int, off: int, seed=None):
    """fp64 output of M elements inside sentinels, ``off`` elements off alignment."""
    buf = torch.full((GUARD + off + M + GUARD,), SENTINEL[8], dtype=torch.int64, device=DEV).view(torch.float64)
    if seed is not None:
        buf[GUARD + off: GUARD + off + M] = torch.from_numpy(seed).to(DEV)
    return buf, buf.data_ptr() + (GUARD + off) * 8


def _sc_check(torch, buf, M, off, ref, what):
    got = buf.cpu().numpy()
    lo = GUARD + off
    g = got.view(np.uint64)
    assert np.all(g[:lo] == SENTINEL[8]) and np.all(g[lo + M:] == SENTINEL[8]), f"{what}: written outside [0, M)"
    assert not np.isnan(ref).any()
    bad = np.flatnonzero(g[lo: lo + M] != ref.view(np.uint64))
    assert bad.size == 0, (f"{what}: {bad.size} of {M} elements differ; first at {bad[:6]}: got "
                           f"{got[lo: lo + M][bad[:6]]} reference {ref[bad[:6]]}")


@pytest.mark.parametrize("case", SCAFFOLD_CASES, ids=[c.id for c in SCAFFOLD_CASES])
def test_scaffold_product_kernel(case):
    import torch

    from substrafl_amd import _native

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    lib = _native.load()
    kind, K, M, off = case.kind, case.K, _M(case), case.off
    L = L_OF[kind]
    rng = np.random.default_rng(sum(map(ord, case.id)))
    d, cv, c, w, tile = _sc_inputs(case, rng)
    lr = 0.7
    idx = []
    if case.pw:  # element 0, inside a full tile, inside the partial tile, M - 1 in the scalar remainder
        idx = [0, (tile // 2 + 3) * L + 1, ((case.nvec // tile) * tile + 5) * L + 1, M - 1]
    cidx = (ctypes.c_uint64 * max(1, len(idx)))(*idx)
    cw = (ctypes.c_double * K)(*[float(v) for v in w])
    ws = torch.empty(max(16, lib.fedagg_pairwise_ws_bytes(K, len(idx), 8)), dtype=torch.uint8, device=DEV)
    ch = np.zeros(M + off + 16, c.dtype)
    ch[off: off + M] = c
    tc = torch.from_numpy(ch).to(DEV)
    c_ptr = tc.data_ptr() + off * c.dtype.itemsize

    _native.tune(sc_2l=case.sc_2l, grid_cap=case.grid_cap)
    try:
        if case.entry == "two":
            td, dp = _dev_rows(torch, d, off)
            tcv, cp = _dev_rows(torch, cv, off)
            dout, dout_p = _sc_out(torch, M, off)
            cout, cout_p = _sc_out(torch, M, off)
            want_launches = 2 if case.id.startswith("sc-bucket2l") else 1
            assert lib.fedagg_scaffold_launches(K, d.dtype.itemsize, M, int(off == 0)) == want_launches, case.id
            rc = getattr(lib, f"fedagg_scaffold_{kind}")(_native.ptr_array(dp), _native.ptr_array(cp), c_ptr, cw, K, M,
                                                         cidx, len(idx), ws.data_ptr(), lr, dout_p, cout_p, None)
            assert rc == 0, lib.fedagg_last_error()
            _sync(torch)
            _sc_check(torch, dout, M, off, _sc_reference(d, w, 0, None, lr, idx, None, True), case.id + " (delta)")
            _sc_check(torch, cout, M, off, _sc_reference(cv, w, 1, c, lr, idx, None, True), case.id + " (c)")
        elif case.entry == "push":
            rows = d if case.phase == 0 else cv
            tr, rp = _dev_rows(torch, rows, 0)
            seed = None
            d_in = None
            if case.din == "sep":
                seed = rng.standard_normal(M)
                seed[:8] = -0.0
                d_in, d_in_p = _sc_out(torch, M, 0, seed)
            out, out_p = _sc_out(torch, M, 0)
            rc = getattr(lib, f"fedagg_scaffold_chain_push_{kind}")(
                _native.ptr_array(rp), cw, K, M, case.phase, c_ptr if case.phase == 1 else None, lr, case.finish,
                d_in_p if d_in is not None else None, out_p, None)
            assert rc == 0, lib.fedagg_last_error()
            _sync(torch)
            ref = _sc_reference(rows, w, case.phase, c, lr, [], seed, bool(case.finish))
            _sc_check(torch, out, M, 0, ref, case.id)
            if d_in is not None:
                _sc_check(torch, d_in, M, 0, seed, case.id + " (d_in)")
        else:
            rows = d if case.phase == 0 else cv
            tr, rp = _dev_rows(torch, rows, off)
            out, out_p = _sc_out(torch, M, off)
            code = {"f32": _native.FEDAGG_F32, "f64": _native.FEDAGG_F64}[kind]
            assert int(lib.fedagg_scaffold_bucket_tile(code)) == tile * L
            rc = lib.fedagg_scaffold_bucket(_native.ptr_array(rp), code, cw, K, M, case.phase,
                                            c_ptr if case.phase == 1 else None, code, lr, cidx, len(idx),
                                            ws.data_ptr(), out_p, None)
            assert rc == 0, lib.fedagg_last_error()
            _sync(torch)
            _sc_check(torch, out, M, off, _sc_reference(rows, w, case.phase, c, lr, idx, None, True), case.id)
    finally:
        _native.tune(**RESET)


# =============================================================================================
# read-stream probes, fp64 flat gather
# =============================================================================================
@pytest.mark.parametrize("case", MISC_CASES)
def test_misc_product_kernel(case):
    import torch

    from substrafl_amd import _native

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    lib = _native.load()
    if case == "misc-read-probe-stream":
        # sink[b] = the sum over wave 0 of workgroup b of the elements its lanes read in the grid-stride
        # walk; small integers, so every order of the fp32 adds gives the same sum
        grid, nvec = 3, 5 * 256 + 77
        rng = np.random.default_rng(5)
        x = rng.integers(-8, 9, nvec * 4 + 3).astype(np.float32)
        tx = torch.from_numpy(x).to(DEV)
        sink = _sentinel_buffer(torch, grid, torch.float32)
        rc = lib.fedagg_read_probe_f32(tx.data_ptr(), x.size, sink.data_ptr(), grid, None)
        assert rc == 0, lib.fedagg_last_error()
        _sync(torch)
        v = np.arange(nvec)
        lane = v % (grid * 256)
        ref = np.array([x[: nvec * 4].reshape(nvec, 4)[(lane >= b * 256) & (lane < b * 256 + 64)].sum(dtype=np.float64)
                        for b in range(grid)]).astype(np.float32)
        _assert_equal_bits(torch, sink[:grid], torch.from_numpy(ref).to(DEV), case)
        _assert_guard(torch, sink, grid, case)
    elif case.startswith("misc-read-probe-tile"):
        # the sink is written only by a thread whose XOR fold of its vectors is the marker: zeros
        # with one marker word in a full tile, in the partial tile (a thread on the full-tile path, one
        # on the per-vector path), and nowhere
        vpt = int(case.rsplit("-", 1)[1])
        tile = vpt * 256
        nvec = 2 * tile + (vpt - 1) * 256 + 100
        marker = 0x9E3779B9
        for word in ((tile + 300) * 4 + 1, (2 * tile + 256 + 7) * 4 + 2, (2 * tile + 256 + 150) * 4 + 3, None):
            x = np.zeros(nvec * 4, np.uint32)
            if word is not None:
                x[word] = marker
            tx = torch.from_numpy(x.view(np.int32)).to(DEV)
            sink = _sentinel_buffer(torch, 0, torch.float32)
            rc = lib.fedagg_read_probe_tile_f32(tx.data_ptr(), x.size, sink.data_ptr(), vpt, None)
            assert rc == 0, lib.fedagg_last_error()
            _sync(torch)
            got = sink.view(torch.int32).cpu().numpy().view(np.uint32)
            assert got[0] == (marker if word is not None else SENTINEL[4]), (case, word, hex(int(got[0])))
            assert np.all(got[1:] == SENTINEL[4]), case
    else:
        numel = [0, 1, 3, 8191, 8193, 2, 0, 16385]
        rng = np.random.default_rng(6)
        src = [rng.standard_normal(n) for n in numel]
        for a in src:
            a.view(np.uint64)[: min(a.size, 7)] = EDGES["f64"][: min(a.size, 7)]
        dev = [torch.from_numpy(a).to(DEV) for a in src]
        n = sum(numel)
        flat = _sentinel_buffer(torch, n, torch.float64)
        rc = lib.fedagg_flat_gather(_native.ptr_array([t.data_ptr() for t in dev]), _native.FEDAGG_F64,
                                    (ctypes.c_uint64 * len(numel))(*numel), len(numel), flat.data_ptr(), None)
        assert rc == 0, lib.fedagg_last_error()
        _sync(torch)
        _assert_equal_bits(torch, flat[:n], torch.from_numpy(np.concatenate(src)).to(DEV), case)
        _assert_guard(torch, flat, n, case)
