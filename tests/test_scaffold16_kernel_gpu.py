"""``fedagg_scaffold_bucket``: one Scaffold bucket per call over rows of any float kind, bit for
bit against NumPy.

Reference: fp64 NumPy on the exact upcasts of the rows and of ``c`` -- ``acc = +0.0; acc = acc +
w_k * x_k`` in client order, then ``lr * acc`` (phase 0) or ``acc + c`` (phase 1) -- with
``oracle.numpy_pairwise_sum`` over the K (phase 0) or K + 1 (phase 1, ``c`` last) fp64 terms of
the ``numel == 1`` elements.  Where the reference is NaN only NaN-ness is compared.

Sizes come from the dispatched tile (``fedagg_scaffold_bucket_tile``), never from a constant.
The argument checks return before any HIP call and carry no ``gpu`` mark."""

import ctypes

import numpy as np
import pytest
import torch  # before libfedagg: one HIP runtime in the process

from oracle import numpy_pairwise_sum
from substrafl_amd import _native

gpu = pytest.mark.gpu

CODE = {"f16": _native.FEDAGG_F16, "bf16": _native.FEDAGG_BF16, "f32": _native.FEDAGG_F32, "f64": _native.FEDAGG_F64}
STORE = {"f16": np.uint16, "bf16": np.uint16, "f32": np.float32, "f64": np.float64}
GUARD = 16  # fp64 elements before and after d_out
SENTINEL = 0x7FF8A5A5A5A5A5A5


def widen(a: np.ndarray, kind: str) -> np.ndarray:
    """The exact fp64 values of stored elements of ``kind``."""
    if kind == "f16":
        return a.view(np.float16).astype(np.float64)
    if kind == "bf16":
        return (a.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)
    return a.astype(np.float64)


def random_stored(rng, kind: str, shape) -> np.ndarray:
    """Random bit patterns of the 16-bit kinds (every class of value), normal draws otherwise."""
    if kind in ("f16", "bf16"):
        return rng.integers(0, 1 << 16, size=shape, dtype=np.uint16)
    return rng.standard_normal(shape).astype(STORE[kind])


def weights(rng, K: int) -> np.ndarray:
    n = rng.integers(1, 5000, K)
    return (n / np.sum(n)).astype(np.float64)  # not representable in fp32


def reference(rows, kind, w, phase, c, c_kind, lr, idx):
    with np.errstate(all="ignore"):
        x = widen(rows, kind)
        acc = np.zeros(x.shape[1], np.float64)
        for k in range(x.shape[0]):
            acc = acc + w[k] * x[k]
        c64 = widen(c, c_kind) if phase == 1 else None
        out = np.float64(lr) * acc if phase == 0 else acc + c64
        for e in idx:
            terms = [w[k] * x[k, e] for k in range(x.shape[0])] + ([c64[e]] if phase == 1 else [])
            s = np.float64(0.0) + numpy_pairwise_sum(np.array(terms, np.float64))
            out[e] = np.float64(lr) * s if phase == 0 else s
    return out


def assert_same(got, ref, what=""):
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), f"NaN positions differ {what}"
    bad = np.flatnonzero((got.view(np.uint64) != ref.view(np.uint64)) & ~nan)
    assert bad.size == 0, f"{bad.size} elements differ {what}: first {bad[:4]} got {got[bad[:4]]} ref {ref[bad[:4]]}"


def launch(rows, kind, w, phase, c, c_kind, lr, idx=(), offset=0, ws=True):
    """Run the entry on device copies of ``rows`` [K, M] (and ``c`` [M]); ``offset`` = 1 moves every
    row, ``c`` and the output off 16-B alignment by one element.  Checks the guard bands."""
    lib = _native.load()
    K, M = rows.shape
    ld = (M + 1 + 15) // 16 * 16
    host = np.zeros((K, ld), rows.dtype)
    host[:, offset : offset + M] = rows
    d_rows = torch.from_numpy(host.view(np.uint8).reshape(K, -1)).cuda()
    isz = rows.dtype.itemsize
    ptrs = _native.ptr_array([d_rows.data_ptr() + (k * ld + offset) * isz for k in range(K)])
    d_c, c_ptr = None, None
    if c is not None:
        ch = np.zeros(M + 16, c.dtype)
        ch[offset : offset + M] = c
        d_c = torch.from_numpy(ch.view(np.uint8)).cuda()
        c_ptr = d_c.data_ptr() + offset * c.dtype.itemsize
    out = torch.from_numpy(np.full(M + 2 * GUARD + 1, SENTINEL, np.uint64).view(np.int64)).cuda()
    idx = np.asarray(idx, np.uint64)
    d_ws = torch.empty(max(16, lib.fedagg_pairwise_ws_bytes(K, int(idx.size), 8)), dtype=torch.uint8, device="cuda")
    rc = lib.fedagg_scaffold_bucket(ptrs, CODE[kind], (ctypes.c_double * K)(*w), K, M, phase, c_ptr,
                                    CODE[c_kind] if c is not None else 0, float(lr),
                                    (ctypes.c_uint64 * max(1, idx.size))(*[int(i) for i in idx]), int(idx.size),
                                    d_ws.data_ptr() if ws else None, out.data_ptr() + (GUARD + offset) * 8, None)
    assert rc == 0, lib.fedagg_last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint64)
    lo, hi = GUARD + offset, GUARD + offset + M
    assert np.all(got[:lo] == SENTINEL) and np.all(got[hi:] == SENTINEL), "guard band written"
    return got[lo:hi].view(np.float64).copy()


def tile_of(kind: str) -> int:
    t = int(_native.load().fedagg_scaffold_bucket_tile(CODE[kind]))
    assert t > 0 and t % (16 // np.dtype(STORE[kind]).itemsize) == 0
    return t


def patch_indices(M: int, L: int, P: int):
    """P distinct numel == 1 indices: the first vector, the last full vector, the scalar tail."""
    nfull = M // L * L
    want = ([0, L - 1, nfull - L, nfull - 1] + list(range(nfull, M)) + list(range(L, nfull - L, max(1, M // 23)))
            + list(range(min(M, 32))))
    out = []
    for i in want:
        if 0 <= i < M and i not in out:
            out.append(i)
    assert len(out) >= P
    return sorted(out[:P])


@gpu
@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_sizes_alignment_and_grid_stride(kind):
    """Every size around the tile, with and without the grid cap, aligned (vector walk) and one
    element off (scalar walk): both equal the reference, hence each other, byte for byte."""
    lib, rng, tile = _native.load(), np.random.default_rng(16), tile_of(kind)
    sizes = [1, 7, 8, 9, tile - 1, tile, tile + 1, 2 * tile + 9]
    K, c_kinds = 5, ["f16", "bf16", "f32", "f64"]
    w = weights(rng, K)
    try:
        for cap in (0, 3):
            assert lib.fedagg_tune(b"grid_cap", cap) == 0
            for n, M in enumerate(sizes):
                rows = random_stored(rng, kind, (K, M))
                c_kind = c_kinds[n % 4]
                c = random_stored(rng, c_kind, M)
                idx = patch_indices(M, 8, min(3, M))
                for phase in (0, 1):
                    ref = reference(rows, kind, w, phase, c, c_kind, 0.7, idx)
                    vec = launch(rows, kind, w, phase, c if phase else None, c_kind, 0.7, idx)
                    sca = launch(rows, kind, w, phase, c if phase else None, c_kind, 0.7, idx, offset=1)
                    assert_same(vec, ref, f"(vector, M={M}, cap={cap}, phase={phase})")
                    assert_same(sca, ref, f"(scalar, M={M}, cap={cap}, phase={phase})")
                    assert np.array_equal(np.isnan(vec), np.isnan(sca))
                    assert np.array_equal(vec.view(np.uint64)[~np.isnan(vec)], sca.view(np.uint64)[~np.isnan(sca)])
    finally:
        lib.fedagg_tune(b"grid_cap", 0)


@gpu
def test_empty_bucket_touches_nothing():
    for kind in ("f16", "bf16", "f32", "f64"):
        rows = np.zeros((2, 0), STORE[kind])
        assert launch(rows, kind, [0.5, 0.5], 1, np.zeros(0, STORE[kind]), kind, 1.0).size == 0


@gpu
@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_client_counts(kind):
    """The client-group remainder and the 64-client chunk seam, in the full tile, the partial
    tile and the scalar tail."""
    rng, tile = np.random.default_rng(17), tile_of(kind)
    M = tile + 8 * 70 + 3
    for K in (1, 2, 3, 5, 63, 64, 65, 130):
        w = weights(rng, K)
        rows = random_stored(rng, kind, (K, M))
        c = random_stored(rng, "f64", M)
        idx = [5, M - 2]
        for phase in (0, 1):
            ref = reference(rows, kind, w, phase, c, "f64", 0.7, idx)
            assert_same(launch(rows, kind, w, phase, c if phase else None, "f64", 0.7, idx), ref, f"(K={K}, {phase})")
    # finite values only: the accumulated sums themselves are compared (random patterns mostly overflow)
    for K in (5, 65):
        w = weights(rng, K)
        rows = rng.standard_normal((K, M)).astype(np.float32)
        rows = rows.astype(np.float16).view(np.uint16) if kind == "f16" else (rows.view(np.uint32) >> 16).astype(np.uint16)
        c = rng.standard_normal(M).astype(np.float32)
        for phase in (0, 1):
            ref = reference(rows, kind, w, phase, c, "f32", 0.7, [])
            assert not np.isnan(ref).any()
            assert_same(launch(rows, kind, w, phase, c if phase else None, "f32", 0.7), ref, f"(finite, K={K})")


@gpu
@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_c_kinds_and_lr(kind):
    rng, tile = np.random.default_rng(18), tile_of(kind)
    M, K = tile + 9, 3
    w = weights(rng, K)
    rows = rng.standard_normal((K, M)).astype(np.float32)
    rows = rows.astype(np.float16).view(np.uint16) if kind == "f16" else (rows.view(np.uint32) >> 16).astype(np.uint16)
    for c_kind in ("f16", "bf16", "f32", "f64"):
        c = random_stored(rng, c_kind, M)
        for lr in (0, 0.7, 1, 2):
            for phase in (0, 1):
                ref = reference(rows, kind, w, phase, c, c_kind, lr, [M - 1])
                got = launch(rows, kind, w, phase, c if phase else None, c_kind, lr, [M - 1])
                assert_same(got, ref, f"(c {c_kind}, lr {lr}, phase {phase})")


def edge_bits(kind: str) -> np.ndarray:
    if kind == "f16":  # +-0, smallest / largest subnormal, smallest normal, max finite, +-inf, NaN, 1, -1.5
        return np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x0400, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00,
                         0x3C00, 0xBE00], np.uint16)
    return np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x007F, 0x0080, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x7FC0,
                     0x3F80, 0xBFC0], np.uint16)


@gpu
@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_edge_values(kind):
    """+-0, subnormals, max finite, +-inf and NaN in every client position; an all -0 column
    sums to +0 (NumPy seeds the reduction with +0.0), with a -0 c as well."""
    e = edge_bits(kind)
    n, K = e.size, 3
    cols = np.array([[e[i], e[j], e[(i + j) % n]] for i in range(n) for j in range(n)], np.uint16).T  # [K, n*n]
    zeros = np.full((K, 40), 0x8000, np.uint16)  # all -0: vector and tail positions
    rows = np.ascontiguousarray(np.concatenate([zeros, cols], axis=1))
    M = rows.shape[1]
    w = np.array([0.3, 0.3, 0.4])
    for c_kind in (kind, "f64"):
        c = np.resize(e, M).copy() if c_kind == kind else widen(np.resize(e, M), kind)
        if c_kind == kind:
            c[:40] = 0x8000
        else:
            c[:40] = -0.0
        for lr in (1, 0.7):
            for phase in (0, 1):
                ref = reference(rows, kind, w, phase, c, c_kind, lr, [])
                for offset in (0, 1):
                    got = launch(rows, kind, w, phase, c if phase else None, c_kind, lr, offset=offset)
                    assert_same(got, ref, f"(c {c_kind}, lr {lr}, phase {phase}, offset {offset})")
                    assert np.all(got[:40].view(np.uint64) == 0), "an all -0 column must give +0"
    # subnormal inputs survive the widening (nothing flushed)
    sub = np.full((1, 16), e[2], np.uint16)
    got = launch(sub, kind, [1.0], 0, None, kind, 1)
    assert np.all(got == widen(sub[0], kind)) and np.all(got > 0)


@gpu
@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("K", [3, 9, 130])
def test_numel_one_patch(kind, K):
    """Fused (P <= 16 and K <= 64) and separate patches, NumPy's pairwise order over K / K + 1 terms."""
    rng, tile = np.random.default_rng(19 + K), tile_of(kind)
    M = tile + 8 * 3 + 5
    w = weights(rng, K)
    rows = rng.standard_normal((K, M)).astype(np.float32)
    rows = rows.astype(np.float16).view(np.uint16) if kind == "f16" else (rows.view(np.uint32) >> 16).astype(np.uint16)
    c = rng.standard_normal(M)
    for P in (0, 1, 16, 17):
        idx = patch_indices(M, 8, P)
        for phase in (0, 1):
            ref = reference(rows, kind, w, phase, c, "f64", 0.7, idx)
            for offset in (0, 1):
                got = launch(rows, kind, w, phase, c if phase else None, "f64", 0.7, idx, offset=offset)
                assert_same(got, ref, f"(P={P}, phase={phase}, offset={offset})")


@gpu
@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_f32_f64_rows_match_the_two_bucket_entry(kind):
    """Both phases are byte-identical to the two outputs of fedagg_scaffold_f32 / _f64."""
    lib, rng, tile = _native.load(), np.random.default_rng(20), tile_of(kind)
    tdt = torch.float32 if kind == "f32" else torch.float64
    for M in (9, tile + 1):
        for K in (3, 65):
            for P in (0, 2):
                idx = [1, M - 1][:P]
                w = weights(rng, K)
                d = rng.standard_normal((K, M)).astype(STORE[kind])
                cv = rng.standard_normal((K, M)).astype(STORE[kind])
                c = rng.standard_normal(M).astype(STORE[kind])
                td, tcv, tc = (torch.from_numpy(a).cuda() for a in (d, cv, c))
                dout, cout = torch.zeros(M, dtype=torch.float64, device="cuda"), torch.zeros(M, dtype=torch.float64,
                                                                                               device="cuda")
                ws = torch.empty(lib.fedagg_pairwise_ws_bytes(K, P, 8), dtype=torch.uint8, device="cuda")
                rows = lambda t: _native.ptr_array([t.data_ptr() + k * M * t.element_size() for k in range(K)])  # noqa: E731
                fn = getattr(lib, f"fedagg_scaffold_{kind}")
                rc = fn(rows(td), rows(tcv), tc.data_ptr(), (ctypes.c_double * K)(*w), K, M,
                        (ctypes.c_uint64 * max(1, P))(*idx), P, ws.data_ptr(), 0.7, dout.data_ptr(), cout.data_ptr(), None)
                assert rc == 0, lib.fedagg_last_error()
                torch.cuda.synchronize()
                assert tdt == td.dtype
                got_d = launch(d, kind, w, 0, None, kind, 0.7, idx)
                got_c = launch(cv, kind, w, 1, c, kind, 0.7, idx)
                assert np.array_equal(got_d.view(np.uint64), dout.cpu().numpy().view(np.uint64)), (M, K, P)
                assert np.array_equal(got_c.view(np.uint64), cout.cpu().numpy().view(np.uint64)), (M, K, P)


def test_argument_errors():
    """Every FEDAGG_EINVAL case: returned before any HIP call (fake, never dereferenced pointers)."""
    lib = _native.load()
    F16, F32, F64 = CODE["f16"], CODE["f32"], CODE["f64"]
    rows = _native.ptr_array([256, 512])
    null_row = _native.ptr_array([256, 0])
    w = (ctypes.c_double * 2)(0.5, 0.5)
    idx = (ctypes.c_uint64 * 17)(*range(17))

    def call(rows=rows, kind=F16, w=w, K=2, M=64, phase=0, c=1024, c_kind=F16, idx=None, P=0, ws=None, out=2048):
        return lib.fedagg_scaffold_bucket(rows, kind, w, K, M, phase, c, c_kind, 1.0, idx, P, ws, out, None)

    def refused(needle, **kw):
        assert call(**kw) == -1
        assert needle in lib.fedagg_last_error(), lib.fedagg_last_error()

    refused(b"K must be > 0", K=0)
    refused(b"K must be > 0", K=-3)
    refused(b"NULL", rows=None)
    refused(b"NULL", w=None)
    refused(b"NULL", out=None)
    refused(b"client pointer 1 is NULL", rows=null_row)
    refused(b"phase", phase=2)
    refused(b"phase", phase=-1)
    refused(b"NULL d_c", phase=1, c=None)
    refused(b"unknown row kind", kind=7)
    refused(b"unknown c kind", phase=1, c_kind=7)
    refused(b"must equal", kind=F32, phase=1, c_kind=F64)
    refused(b"must equal", kind=F64, phase=1, c_kind=F16)
    refused(b"out of range", idx=(ctypes.c_uint64 * 1)(64), P=1)
    refused(b"index list", idx=None, P=1)
    refused(b"index list", idx=idx, P=-1)
    refused(b"workspace needed", idx=idx, P=17)  # more than the fused patch takes
    big = _native.ptr_array([256] * 65)
    refused(b"workspace needed", rows=big, w=(ctypes.c_double * 65)(*[1 / 65] * 65), K=65, idx=idx, P=1)
    assert call(M=0) == 0  # nothing to do, nothing touched
    assert call(M=0, phase=1, c=1024, c_kind=F64) == 0
    assert lib.fedagg_scaffold_bucket_tile(7) == 0
