"""Scaffold on the multi-GPU route, all on one GPU with repeated device indices.

* ``fedagg_multi_scaffold_bucket`` (csrc/multi.hip) against ONE whole-range
  ``fedagg_scaffold_bucket`` launch on the same rows, both phases: the same bits wherever the
  reference is not NaN and NaN exactly where it is (the rule of ``golden_dtypes_cases.same``: a
  NaN's sign and payload are not compared).  The entry's sessions are private to it, so instead of
  their buffers the host outputs are poisoned (0xA5 bytes, a finite double) before each call, and
  consecutive cases differ in every input.
* the check of the clients' ``c`` on the pack workers, range by range, for each kind;
* the reference's recorded vectors (``tests/golden/golden_dtypes.npz``) through
  ``NativeMultiScaffold`` and ``MultiDeviceEngine.scaffold_per_bucket``;
* 16-bit buckets past ``max_bucket_bytes`` stream through ``AggregationEngine``;
* ``strategies.Scaffold`` over two devices on bf16 shared states.
"""

import ctypes

import numpy as np
import pytest

import golden_dtypes_cases as G
from substrafl_amd import _native, wire

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]

SMALL = 64  # bytes: below one row of any case, so sub-ranges are the 512-element minimum
CODE = {"f16": _native.FEDAGG_F16, "bf16": _native.FEDAGG_BF16, "f32": _native.FEDAGG_F32, "f64": _native.FEDAGG_F64}
UINT = {"f16": np.uint16, "bf16": np.uint16, "f32": np.uint32, "f64": np.uint64}
# bit patterns per kind: subnormals, +-0, +-inf, NaN
SPECIAL = {"f16": [0x0001, 0x83FF, 0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00],
           "bf16": [0x0001, 0x807F, 0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0],
           "f32": [0x00000001, 0x807FFFFF, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000],
           "f64": [0x1, 0x800FFFFFFFFFFFFF, 0x0, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,
                   0x7FF8000000000000]}
SIGN = {"f16": 0x8000, "bf16": 0x8000, "f32": 0x80000000, "f64": 0x8000000000000000}
QNAN = {k: v[6] for k, v in SPECIAL.items()}
ONE = {"f16": 0x3C00, "bf16": 0x3F80, "f32": 0x3F800000, "f64": 0x3FF0000000000000}
TWO = {"f16": 0x4000, "bf16": 0x4000, "f32": 0x40000000, "f64": 0x4000000000000000}
POISON = 0xA5


def values(kind, shape, rng, specials=True):
    """Bit patterns of normal values of ``kind`` with every special value planted three times."""
    x = rng.standard_normal(shape) * 3.0
    if kind == "f16":
        bits = x.astype(np.float16).view(np.uint16)
    elif kind == "bf16":
        bits = (x.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    else:
        bits = x.astype(np.float32 if kind == "f32" else np.float64).view(UINT[kind])
    bits = np.ascontiguousarray(bits)
    if specials:
        flat = bits.reshape(-1)
        pos = rng.choice(flat.size, size=min(flat.size, 3 * len(SPECIAL[kind])), replace=False)
        for j, p in enumerate(pos):
            flat[p] = SPECIAL[kind][j % len(SPECIAL[kind])]
    return bits


def same_bits(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype == np.float64 and got.shape == ref.shape, what
    nan = np.isnan(ref)
    assert 0 < (~nan).sum() and nan.mean() < 0.5, (what, "the reference is mostly NaN")
    assert np.array_equal(np.isnan(got), nan), (what, "NaN placement")
    bad = (got.view(np.uint64) != ref.view(np.uint64)) & ~nan
    assert not bad.any(), (what, f"{int(bad.sum())} of {ref.size} differ, first at {int(np.argmax(bad))}")


@pytest.fixture(scope="module")
def lib():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _native.load()


@pytest.fixture(scope="module")
def native(lib):
    """The C entry's engines over [0, 0] and [0, 0, 0], sub-ranges of the 512-element minimum."""
    from substrafl_amd.multi_device import NativeMultiScaffold

    objs = {2: NativeMultiScaffold([0, 0], max_shard_bytes=SMALL), 3: NativeMultiScaffold([0, 0, 0], max_shard_bytes=SMALL)}
    yield objs
    for o in objs.values():
        o.close()


class WholeRange:
    """One ``fedagg_scaffold_bucket`` launch over the whole range on a session of its own."""

    def __init__(self):
        from substrafl_amd import runtime

        self.s = runtime.Session(0)

    def __call__(self, rows, kind, phase, w, lr, idx, c=None, c_kind=None):
        from substrafl_amd.engine import ScaffoldBucketPlan
        from substrafl_amd.multi_device import _ld

        s, (K, M), isz = self.s, rows.shape, rows.itemsize
        ld = _ld(M, isz)
        d = s.buffer(0, K * ld * isz)
        s.stage(d, ld * isz, [[rows[k]] for k in range(K)])
        d_c = None
        if phase == 1:
            d_c = s.buffer(5, _ld(M, c.itemsize) * c.itemsize)
            s.stage(d_c, _ld(M, c.itemsize) * c.itemsize, [[c]])
        d_out = s.buffer(1, _ld(M, 8) * 8)
        s.memset(d_out, 0xFF, _ld(M, 8) * 8)
        ws = s.buffer(2, s.lib.fedagg_pairwise_ws_bytes(K, max(1, len(idx)), 8))
        ScaffoldBucketPlan(kind, [d + k * ld * isz for k in range(K)], phase, d_c, c_kind, w, M, lr, d_out,
                           np.asarray(idx, np.uint64), ws).launch(s.stream)
        return s.fetch(d_out, np.empty(M, np.float64))


@pytest.fixture(scope="module")
def whole(lib):
    w = WholeRange()
    yield w
    w.s.close()


def multi_call(nat, phase, rows, kind, w, lr, idx, c=None, c_kind=None, mismatches=True):
    """``fedagg_multi_scaffold_bucket`` on ``rows`` [K, M] cut into uneven host segments (one of one
    element); ``c`` [Kc, M].  Returns ``(out, mismatches or None)``."""
    from substrafl_amd import runtime

    K, M = rows.shape
    edges = sorted({0, int(M * 0.31), min(M, int(M * 0.31) + 1), int(M * 0.9), M})
    cut = lambda a: [[a[k, lo:hi] for lo, hi in zip(edges, edges[1:])] for k in range(a.shape[0])]  # noqa: E731
    nseg, ptrs, sizes, keep = runtime._segments(cut(rows))
    Kc, c_nseg, c_ptrs, c_sizes, c_keep = 0, 0, None, None, None
    if phase == 1:
        Kc = c.shape[0]
        c_nseg, c_ptrs, c_sizes, c_keep = runtime._segments([[row] for row in c])  # c: one segment per copy
    out = np.empty(M, np.float64)
    out.view(np.uint8).fill(POISON)
    idx = np.asarray(idx, np.uint64)
    mism = ctypes.c_uint64(123456789)
    before = ctypes.c_int(-1)
    nat.lib.fedagg_device_get(ctypes.byref(before))
    rc = nat.lib.fedagg_multi_scaffold_bucket(
        nat._h, phase, K, nseg, ptrs, sizes, CODE[kind], w.ctypes.data, float(lr), Kc, c_nseg, c_ptrs, c_sizes,
        CODE[c_kind] if c_kind else 0, idx.ctypes.data if idx.size else None, int(idx.size), out.ctypes.data,
        ctypes.byref(mism) if mismatches else None)
    _native.check(rc, "fedagg_multi_scaffold_bucket")
    after = ctypes.c_int(-2)
    nat.lib.fedagg_device_get(ctypes.byref(after))
    assert after.value == before.value, "the caller's current device changed"
    del keep, c_keep
    return out, (int(mism.value) if mismatches else None)


def weights(K, rng):
    from substrafl_amd.engine import scaffold_weights

    return scaffold_weights([int(v) for v in rng.integers(1, 5000, K)])


M3 = 3109  # [0,0,0]: shards [0,1536) [1536,3072) [3072,3109): three sub-ranges on the full ones, 37 ragged elements
EDGES = (0, 511, 512, 1535, 1536, M3 - 1)
CASES = [  # id, devices, row kind, c kind, M, K, numel == 1 indices
    ("f16-3dev", 3, "f16", "bf16", M3, 3, EDGES),
    ("bf16-3dev", 3, "bf16", "f32", M3, 3, EDGES),
    ("f32-3dev", 3, "f32", "f32", M3, 3, EDGES),
    ("f64-3dev", 3, "f64", "f64", M3, 3, EDGES),
    ("f16-K65-separate-pairwise", 2, "f16", "f64", M3, 65, (0, 2047, 2048, M3 - 1)),  # K > 64 with P >= 1: not fusable
    ("bf16-K130", 2, "bf16", "f16", M3, 130, (1536,)),  # three argument chunks continuing the accumulator
    ("f32-K65", 2, "f32", "f32", M3, 65, ()),  # a second chunk
    ("f64-K130", 3, "f64", "f64", M3, 130, (5, 3071, 3072)),
    ("f16-17-indices-in-one-sub-range", 3, "f16", "f16", M3, 3, tuple(range(520, 537))),  # past FEDAGG_FUSED_PAIRWISE
    ("bf16-c-bf16", 2, "bf16", "bf16", M3, 3, EDGES),
    ("f16-c-f32-K1", 2, "f16", "f32", M3, 1, EDGES),
    ("bf16-c-f64-512", 3, "bf16", "f64", 512, 3, (0, 511)),  # a single sub-range
    ("f32-512-K1", 2, "f32", "f32", 512, 1, (0, 511)),
    ("f64-500", 3, "f64", "f64", 500, 3, (0, 499)),  # only shard 0 has work
    ("f16-500-K65", 2, "f16", "f16", 500, 65, (499,)),
]


@pytest.mark.parametrize("devices,kind,c_kind,M,K,idx", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_entry_equals_one_whole_range_launch(native, whole, devices, kind, c_kind, M, K, idx):
    rng = np.random.default_rng(1000 * K + M + devices + len(kind))
    nat, w, lr = native[devices], weights(K, rng), 0.7
    for phase in (0, 1):
        rows = values(kind, (K, M), rng)
        c = values(c_kind, (1, M), rng) if phase == 1 else None
        ref = whole(rows, kind, phase, w, lr, idx, c[0] if phase == 1 else None, c_kind)
        got, mism = multi_call(nat, phase, rows, kind, w, lr, idx, c, c_kind if phase == 1 else None)
        assert not (got.view(np.uint8) == POISON).all(axis=None), "nothing was written"
        same_bits(got, ref, (kind, c_kind, M, K, "phase", phase))
        assert mism == (0 if phase == 1 else 123456789)  # Kc == 1: no check; phase 0 leaves it alone
        info = nat.shard_info()
        assert [i["device"] for i in info] == [0] * devices
        busy, most = sum(1 for i in info if i["hi"] > i["lo"]), max(i["ranges"] for i in info)
        assert info[0]["lo"] == 0 and max(i["hi"] for i in info) == M
        if M == M3:
            assert busy >= 2 and most > 1, info
            assert (busy, most) == ((3, 3) if devices == 3 else (2, 4)), info
        else:
            assert busy == 1 and most == 1 and sum(i["ranges"] for i in info) == 1, info


def test_m_zero_and_a_refused_call_leave_the_engine_usable(native, whole):
    nat = native[2]
    rng = np.random.default_rng(5)
    w = weights(2, rng)
    out, _ = multi_call(nat, 0, np.zeros((2, 0), np.uint16), "f16", w, 0.5, ())
    assert out.size == 0
    rows = values("f32", (2, 700), rng)
    with pytest.raises(_native.NativeLibraryError, match="out of range"):
        multi_call(nat, 0, rows, "f32", w, 0.5, (700,))
    ref = whole(rows, "f32", 0, w, 0.5, (3,))
    same_bits(multi_call(nat, 0, rows, "f32", w, 0.5, (3,))[0], ref, "after a refused call")


# ------------------------------------------------------------------------------------- the check of c
@pytest.mark.parametrize("c_kind", ["f16", "bf16", "f32", "f64"])
def test_c_copies_are_compared_range_by_range(native, whole, c_kind):
    rng = np.random.default_rng(77 + len(c_kind))
    K, M, nat = 4, M3, native[3]
    w, rows = weights(K, rng), values("f16", (K, M), rng)
    c0 = values(c_kind, (M,), rng, specials=False)
    in_shard1_second = 1536 + 512 + 5  # shard 1 is [1536, 3072); its second sub-range [2048, 2560)
    c0[in_shard1_second] = c0[M - 1] = ONE[c_kind]
    c0[10], c0[2000], c0[3100] = 0, QNAN[c_kind], SIGN[c_kind]
    ref = whole(rows, "f16", 1, w, 0.7, EDGES, c0, c_kind)

    c = np.stack([c0] * K)
    got, mism = multi_call(nat, 1, rows, "f16", w, 0.7, EDGES, c, c_kind)
    assert mism == 0
    same_bits(got, ref, (c_kind, "equal copies"))

    c[2, in_shard1_second] = TWO[c_kind]
    c[K - 1, M - 1] = TWO[c_kind]
    got, mism = multi_call(nat, 1, rows, "f16", w, 0.7, EDGES, c, c_kind)
    assert mism == 2
    same_bits(got, ref, (c_kind, "the outputs are copy 0's whatever the count"))

    c = np.stack([c0] * K)  # copies that differ by the sign of zero and by NaN payload and sign only
    c[1, 10], c[3, 3100] = SIGN[c_kind], 0
    c[2, 2000] = QNAN[c_kind] | SIGN[c_kind] | 1
    assert not np.array_equal(c[1], c0) and not np.array_equal(c[2], c0)
    got, mism = multi_call(nat, 1, rows, "f16", w, 0.7, EDGES, c, c_kind)
    assert mism == 0
    same_bits(got, ref, (c_kind, "+-0 and NaN payloads"))

    # Kc == 1: one copy staged, nothing compared, and no counter needed
    got, mism = multi_call(nat, 1, rows, "f16", w, 0.7, EDGES, c[:1], c_kind, mismatches=False)
    assert mism is None
    same_bits(got, ref, (c_kind, "Kc == 1"))


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_session_stage_check_counts_16_bit_kinds(whole, kind):
    """Session.stage_check on fp16 / bf16 copies: planted differences counted, +-0 and NaN payloads
    equal, the 0x7E00 / 0x7E01 pair equal as fp16 (two NaNs) and different as bf16 (two finite
    values); the same through a byte range; copy 0's bytes are what is staged."""
    s, dt = whole.s, (np.dtype(np.float16) if kind == "f16" else wire.BF16)
    rng = np.random.default_rng(3)
    base = values(kind, (2000,), rng, specials=False)
    base[20], base[30], base[50] = 0, QNAN[kind], 0x7E00
    copies = [base.copy() for _ in range(3)]
    copies[1][20], copies[2][30], copies[1][50] = SIGN[kind], QNAN[kind] | SIGN[kind] | 3, 0x7E01
    copies[1][10] ^= 0x0010  # segment 0
    copies[2][705] ^= 0x0010  # segment 1
    copies[2][1999] ^= 0x0010  # the last element
    rows = [[x[:700].view(dt), x[700:].view(dt)] for x in copies]
    d = s.buffer(7, 4096)
    assert s.stage_check(d, rows, dt) == 3 + (kind == "bf16")
    assert s.check(rows, dt) == 3 + (kind == "bf16")
    staged = s.fetch(d, np.empty(2000, np.uint16))
    assert np.array_equal(staged, base)
    assert s.stage_check(d, rows, dt, byte_range=(2 * 600, 2 * 1000)) == 1
    assert np.array_equal(s.fetch(d, np.empty(400, np.uint16)), base[600:1000])
    assert s.stage_check(d, rows, dt, byte_range=(2 * 40, 2 * 60)) == (kind == "bf16")
    assert s.stage_check(d, rows[:1], dt) == 0


# ------------------------------------------------------------------------------------- the reference's vectors
def _shards_busy(ranges) -> bool:
    return sum(1 for x in ranges if x) >= 2 and max(len(x) for x in ranges) > 1


def _poison(sessions):
    for s in sessions:
        for slot in (1, 6):
            s.memset(s.buffer(slot, 1 << 18), 0xFF, 1 << 18)
        s.sync()


def test_golden_vectors_through_both_routes(native):
    """Every recorded Scaffold case through NativeMultiScaffold (all of them have uniform buckets)
    and through MultiDeviceEngine.scaffold_per_bucket: the reference's vectors bit for bit, and
    how many cases took each route."""
    from substrafl_amd.multi_device import MultiDeviceEngine

    nat = native[3]
    md = MultiDeviceEngine([0, 0, 0], max_shard_bytes=SMALL)
    n, red = {}, []

    def count(route):
        n[route] = n.get(route, 0) + 1

    def same(got, ref, what):
        try:
            G.same(got, ref, what)
        except AssertionError as e:
            red.append(str(e)[:300])

    for case, ns, pu, cv, cs, lr, out in G.scaffold_cases():
        key, sixteen = case["key"], "f16" in case["triple"][:2]
        identity = all(row is cs[0] for row in cs)
        # the C entry
        mism, new_c, avg = nat.scaffold(pu, cv, cs, ns, lr)
        assert (mism > 0) == (out is None), key
        if out is not None:
            same(avg, out[0], (key, "native", "avg"))
            same(new_c, out[1], (key, "native", "new c"))
        if case["kind"] == "edge":
            info = nat.shard_info()
            assert sum(1 for i in info if i["hi"] > i["lo"]) >= 2 and max(i["ranges"] for i in info) > 1, info
            count("NativeMultiScaffold (busy shards)")
        count("NativeMultiScaffold" if out is not None else "NativeMultiScaffold (mismatch counted)")
        # the Python engine
        plain = None
        if not sixteen:
            md.last_timing = {}
            md.scaffold(pu, cv, cs, ns, lr)
            plain = md.last_timing
        _poison(md.sessions())
        md.last_timing = {}
        mism, new_c, avg = md.scaffold_per_bucket(pu, cv, cs, ns, lr)
        assert (mism > 0) == (out is None), key
        if out is not None:
            same(avg, out[0], (key, "multi-device per bucket", "avg"))
            same(new_c, out[1], (key, "multi-device per bucket", "new c"))
        lt = md.last_timing
        if sixteen:
            assert list(lt["bucket_kinds"]) == case["triple"], key
            assert lt["c_check"] == ("identity" if identity else "host"), key
            assert any(lt["ranges"]) and any(lt["ranges_cv"]), key
            if case["kind"] == "edge":
                assert _shards_busy(lt["ranges"]) and _shards_busy(lt["ranges_cv"]), lt
                count("scaffold_per_bucket (16-bit, busy shards)")
            count("scaffold_per_bucket (16-bit, range-sharded)")
        else:
            assert set(lt) == set(plain) == {"total_s", "ranges"} and lt["ranges"] == plain["ranges"], key
            count("scaffold_per_bucket (f32 / f64: MultiDeviceEngine.scaffold)")
    assert not red, f"{len(red)} red:\n" + "\n".join(red)
    # 16-bit: the three tables, the (f16, f64, f64) edge, two fp16 non-finite, fp16 c equal by value and mismatching
    assert n == {"NativeMultiScaffold": 45, "NativeMultiScaffold (mismatch counted)": 2,
                 "NativeMultiScaffold (busy shards)": 2,
                 "scaffold_per_bucket (16-bit, range-sharded)": 3 * 7 + 1 + 2 + 2,
                 "scaffold_per_bucket (16-bit, busy shards)": 1,
                 "scaffold_per_bucket (f32 / f64: MultiDeviceEngine.scaffold)": 2 * 7 + 1 + 4 + 2}, n


def test_native_refuses_what_the_entry_does_not_take(native):
    nat = native[2]
    f16 = [[np.ones((3, 2), np.float16), np.ones(1, np.float16)]] * 2
    f32 = [[np.ones((3, 2), np.float32), np.ones(1, np.float32)]] * 2
    f64 = [[np.ones((3, 2), np.float64), np.ones(1, np.float64)]] * 2
    mixed = [[np.ones((3, 2), np.float16), np.ones(1, np.float32)]] * 2
    ints = [[np.ones((3, 2), np.int32), np.ones(1, np.int32)]] * 2
    for pu, cv, cs in ((mixed, f16, f16), (f16, ints, f16), (f16, f32, f64), (f16, f64, f16), (f32, f32, f16)):
        with pytest.raises(NotImplementedError):
            nat.scaffold(pu, cv, cs, [1, 2], 0.5)
    mism, new_c, avg = nat.scaffold(f32, f16, f64, [1, 3], 0.5)  # any c kind next to a 16-bit bucket
    assert mism == 0 and all(np.array_equal(a, np.full(a.shape, 2.0)) for a in new_c)
    assert all(np.array_equal(a, np.full(a.shape, 0.5)) for a in avg)


# ------------------------------------------------------------------------------------- out of core, end to end
SHAPES = [(40, 30), (1,), (7,), (1300,)]  # M = 2508: two busy shards over (0, 0)


def _model(kind, K, rng, c_per_client):
    dt = np.dtype(np.float16) if kind == "f16" else wire.BF16
    mk = lambda: [values(kind, s, rng, specials=False).view(dt) for s in SHAPES]  # noqa: E731
    pus, cvs, c = [mk() for _ in range(K)], [mk() for _ in range(K)], mk()
    cs = [[a.copy() for a in c] for _ in range(K)] if c_per_client else [c] * K
    return pus, cvs, cs, [int(v) for v in rng.integers(1, 5000, K)]


@pytest.mark.parametrize("kind,c_per_client", [("f16", True), ("bf16", False)], ids=["f16-host-check", "bf16-identity"])
def test_sixteen_bit_buckets_past_the_budget_stream(lib, kind, c_per_client):
    from substrafl_amd.engine import AggregationEngine

    pus, cvs, cs, ns = _model(kind, 3, np.random.default_rng(11), c_per_client)
    eng = AggregationEngine(device=0)
    mism, new_c, avg = eng.scaffold_per_bucket(pus, cvs, cs, ns, 0.7)
    assert mism == 0 and "out_of_core" not in eng.last_timing and eng.last_timing["bucket_kinds"] == (kind,) * 3
    first = ([a.copy() for a in avg], [a.copy() for a in new_c])
    small = AggregationEngine(device=0, max_bucket_bytes=SMALL)
    _poison([small.session()])
    mism, new_c, avg = small.scaffold_per_bucket(pus, cvs, cs, ns, 0.7)
    ooc = small.last_timing["out_of_core"]
    assert mism == 0 and ooc["bucket_kinds"] == (kind,) * 3
    assert ooc["c_check"] == ("host" if c_per_client else "identity")
    assert len(ooc["ranges"][0]) == len(ooc["ranges_cv"][0]) == 5  # 2508 elements, 512 at a time
    G.same(avg, first[0], (kind, "out of core", "avg"))
    G.same(new_c, first[1], (kind, "out of core", "new c"))
    if c_per_client:
        cs[2][3].view(np.uint16)[1299] ^= 0x0100
        assert small.scaffold_per_bucket(pus, cvs, cs, ns, 0.7)[0] == 1
        assert eng.scaffold_per_bucket(pus, cvs, cs, ns, 0.7)[0] == 1


def test_strategy_over_two_devices_on_bf16_states(lib, dummy_algo_class):
    """strategies.Scaffold with devices (0, 0) on bf16 shared states: what the one-device strategy
    returns.  Without MultiDeviceEngine.scaffold_per_bucket this raised NotImplementedError."""
    from substrafl_amd.engine import engine_for
    from substrafl_amd.schemas import ScaffoldSharedState
    from substrafl_amd.strategies import Scaffold

    pus, cvs, cs, ns = _model("bf16", 4, np.random.default_rng(23), False)
    states = [ScaffoldSharedState(parameters_update=pus[k], control_variate_update=cvs[k], n_samples=ns[k],
                                  server_control_variate=cs[k]) for k in range(4)]
    one = Scaffold(algo=dummy_algo_class(), aggregation_lr=0.7, device=0).avg_shared_states(states, _skip=True)
    one = ([np.array(a) for a in one.avg_parameters_update], [np.array(a) for a in one.server_control_variate])
    two = Scaffold(algo=dummy_algo_class(), aggregation_lr=0.7, device=(0, 0)).avg_shared_states(states, _skip=True)
    lt = engine_for((0, 0)).last_timing
    assert lt["bucket_kinds"] == ("bf16", "bf16", "bf16") and lt["c_check"] in ("identity", "host")
    assert sum(1 for x in lt["ranges"] if x) == sum(1 for x in lt["ranges_cv"] if x) == 2
    G.same(two.avg_parameters_update, one[0], "avg")
    G.same(two.server_control_variate, one[1], "new c")
    assert all(np.isfinite(a).all() for a in one[0] + one[1])
