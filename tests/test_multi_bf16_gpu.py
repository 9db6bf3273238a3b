"""bf16 FedAvg on the multi-GPU route, all on one GPU with repeated device indices.

* ``fedagg_multi_fedavg_bf16`` (csrc/multi.hip) against ONE whole-range ``fedagg_fedavg_bf16`` launch
  on the same rows and against the oracle on their fp32 upcasts: the same bits wherever the
  reference is not NaN and NaN exactly where it is (the rule of
  ``test_multi_scaffold_gpu.same_bits``).  The entry's sessions are private to it, so instead of
  their buffers the host outputs are poisoned (0xA5 bytes) before each call;
* repeated calls on one object, and the default budget;
* the reference's recorded vectors (``tests/golden/golden_dtypes.npz``) through
  ``NativeMultiFedAvg.fedavg_bf16``, ``MultiDeviceEngine.fedavg_routed`` and, past
  ``max_bucket_bytes``, ``AggregationEngine.fedavg_routed``;
* ``fedavg_routed`` on other inputs is ``fedavg``;
* ``strategies.FedAvg`` over two devices on bf16 shared states; the plain-C demo.
"""

import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import golden_dtypes_cases as G
from oracle import fedavg_reference_structure
from substrafl_amd import _native, wire

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]

ROOT = Path(__file__).resolve().parents[1]
SMALL = 64  # bytes: below one row of any case, so sub-ranges are the 512-element minimum
ALIGN = 512
SPECIAL = [0x0001, 0x807F, 0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0]  # subnormals, +-0, +-inf, NaN
POISON = 0xA5


def values(shape, rng):
    """bf16 bit patterns of normal values x 3 (truncated), and from 512 elements a row every
    special value planted three times over the whole array (at most 21 columns touched)."""
    bits = np.ascontiguousarray((rng.standard_normal(shape) * 3.0).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    if shape[-1] >= ALIGN:
        flat = bits.reshape(-1)
        for j, p in enumerate(rng.choice(flat.size, size=3 * len(SPECIAL), replace=False)):
            flat[p] = SPECIAL[j % len(SPECIAL)]
    return bits


def upcast(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def same_bits(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype == np.float32 and got.shape == ref.shape, what
    nan = np.isnan(ref)
    assert 0 < (~nan).sum() and nan.mean() < 0.5, (what, "the reference is mostly NaN")
    assert np.array_equal(np.isnan(got), nan), (what, "NaN placement")
    bad = (got.view(np.uint32) != ref.view(np.uint32)) & ~nan
    assert not bad.any(), (what, f"{int(bad.sum())} of {ref.size} differ, first at {int(np.argmax(bad))}")


def oracle(rows, ns, idx):
    """fed_avg.py:217-222 on the fp32 upcasts, the row cut into layers so that exactly the
    elements of ``idx`` are numel == 1 layers (NumPy reduces those in pairwise order)."""
    K, M = rows.shape
    edges = sorted({0, M} | {int(i) for i in idx} | {int(i) + 1 for i in idx})
    pieces = list(zip(edges, edges[1:]))
    assert all((hi - lo == 1) == (lo in set(idx)) for lo, hi in pieces) or M == 1, "a one-element piece is no index"
    x = upcast(rows)
    out = fedavg_reference_structure([[x[k, lo:hi] for lo, hi in pieces] for k in range(K)], ns)
    return np.concatenate([np.asarray(o, np.float32).reshape(-1) for o in out])


@pytest.fixture(scope="module")
def lib():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _native.load()


@pytest.fixture(scope="module")
def native(lib):
    """The C entry's engines over [0, 0] and [0, 0, 0], sub-ranges of the 512-element minimum."""
    from substrafl_amd.multi_device import NativeMultiFedAvg

    objs = {2: NativeMultiFedAvg([0, 0], max_shard_bytes=SMALL), 3: NativeMultiFedAvg([0, 0, 0], max_shard_bytes=SMALL)}
    yield objs
    for o in objs.values():
        o.close()


class WholeRange:
    """One ``fedagg_fedavg_bf16`` launch over the whole range on a session of its own."""

    def __init__(self):
        from substrafl_amd import runtime

        self.s = runtime.Session(0)

    def __call__(self, rows, w, idx):
        from substrafl_amd.engine import FedAvgPlan
        from substrafl_amd.multi_device import _ld

        s, (K, M) = self.s, rows.shape
        ld = _ld(M, 2)
        d = s.buffer(0, K * ld * 2)
        s.stage(d, ld * 2, [[rows[k]] for k in range(K)])
        d_out = s.buffer(1, _ld(M, 4) * 4)
        s.memset(d_out, 0xFF, _ld(M, 4) * 4)
        ws = s.buffer(2, s.lib.fedagg_pairwise_ws_bytes(K, max(1, len(idx)), 8))
        FedAvgPlan("bf16", [d + k * ld * 2 for k in range(K)], w, M, d_out, np.asarray(idx, np.uint64), ws).launch(s.stream)
        return s.fetch(d_out, np.empty(M, np.float32))


@pytest.fixture(scope="module")
def whole(lib):
    w = WholeRange()
    yield w
    w.s.close()


def multi_call(nat, rows, w, idx):
    """``fedagg_multi_fedavg_bf16`` on ``rows`` [K, M] as two host segments cut at element 7 (one
    segment up to 7 elements) into a poisoned output; the caller's device stays."""
    from substrafl_amd import runtime

    K, M = rows.shape
    segs = [[rows[k, :7], rows[k, 7:]] if M > 7 else [rows[k]] for k in range(K)]
    nseg, ptrs, sizes, keep = runtime._segments(segs)
    out = np.empty(M, np.float32)
    out.view(np.uint8).fill(POISON)
    idx = np.asarray(idx, np.uint64)
    before, after = ctypes.c_int(-1), ctypes.c_int(-2)
    nat.lib.fedagg_device_get(ctypes.byref(before))
    rc = nat.lib.fedagg_multi_fedavg_bf16(nat._h, K, nseg, ptrs, sizes, w.ctypes.data,
                                          idx.ctypes.data if idx.size else None, int(idx.size), out.ctypes.data)
    _native.check(rc, "fedagg_multi_fedavg_bf16")
    nat.lib.fedagg_device_get(ctypes.byref(after))
    assert after.value == before.value, "the caller's current device changed"
    del keep
    if M:
        assert not (out.view(np.uint32) == 0xA5A5A5A5).any(), "an element was not written"
    return out


def samples(K, rng):
    return [int(v) for v in rng.integers(1, 5001, K)]


def check_plan(nat, M, minimum_step=True):
    """The shards tile [0, M) contiguously at 512-element multiples; with the smallest budget every
    sub-range is 512 elements, with the default one every busy shard streams one."""
    info = nat.shard_info()
    assert [i["device"] for i in info] == [0] * len(info)
    at = 0
    for i in info:
        assert i["lo"] == min(at, M) and i["lo"] <= i["hi"] <= M, info
        assert i["lo"] % ALIGN == 0 or i["lo"] == M, info
        n = i["hi"] - i["lo"]
        assert i["ranges"] == (-(-n // ALIGN) if minimum_step else int(n > 0)), info
        at = i["hi"]
    assert at == M, info
    return info


M4 = 3 * 512 + 37
M17 = 4096 + 5
CASES = [  # id, K, M, numel == 1 indices
    ("K1-M1", 1, 1, ()),
    ("M511", 3, 511, ()),
    ("M512", 3, 512, ()),
    ("M513", 3, 513, ()),
    ("indices-on-sub-range-edges", 5, M4, (0, 511, 512, M4 - 1)),
    ("K33-many-client-kernel", 33, 2 * 512 + 8, (5,)),
    # K > FEDAGG_KCHUNK: a continued accumulator, and the separate gather / tree with the workspace
    ("K129-two-chunks", 129, 1024 + 3, (0, 1024)),
    # P > FEDAGG_FUSED_PAIRWISE, spread over the shards of both engines (and two in one sub-range)
    ("17-indices", 3, M17, tuple(range(3, M17, 256))[:15] + (M17 - 4, M17 - 1)),
]


@pytest.mark.parametrize("K,M,idx", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_entry_equals_one_whole_range_launch(native, whole, K, M, idx):
    from substrafl_amd.engine import fedavg_weights

    assert K <= _native.FEDAGG_KCHUNK or K == 129
    assert len(idx) <= _native.FEDAGG_FUSED_PAIRWISE or len(idx) == 17
    rng = np.random.default_rng(1000 * K + M)
    rows, ns = values((K, M), rng), samples(K, rng)
    w = fedavg_weights(ns, "bf16")
    assert w.dtype == np.float32
    ref = oracle(rows, ns, idx)
    one = whole(rows, w, idx)
    same_bits(one, ref, (K, M, "one whole-range launch against the oracle"))
    for devices in (2, 3):
        got = multi_call(native[devices], rows, w, idx)
        same_bits(got, one, (K, M, devices, "against one whole-range launch"))
        same_bits(got, ref, (K, M, devices, "against the oracle"))
        info = check_plan(native[devices], M)
        if M > 2 * ALIGN:
            assert sum(1 for i in info if i["hi"] > i["lo"]) >= 2, info  # (check_plan pins the sub-ranges)


def test_repeated_calls_and_the_default_budget(native, whole):
    from substrafl_amd.engine import fedavg_weights

    nat, rng = native[2], np.random.default_rng(42)
    first = None
    for K, M, idx in ((5, M4, (0, 511, 512, M4 - 1)), (3, 700, (699,)), (5, M4, (0, 511, 512, M4 - 1))):
        rows, ns = values((K, M), rng), samples(K, rng)  # new values every time
        w = fedavg_weights(ns, "bf16")
        got = multi_call(nat, rows, w, idx)  # a smaller call after a larger one: the buffers are reused
        same_bits(got, whole(rows, w, idx), (K, M, "repeated"))
        check_plan(nat, M)
        if first is not None:
            assert got.shape != first.shape or not np.array_equal(got.view(np.uint32), first.view(np.uint32))
        first = got
    # M == 0: nothing to do, nothing touched
    assert multi_call(nat, np.zeros((2, 0), np.uint16), fedavg_weights([1, 2], "bf16"), ()).size == 0
    with pytest.raises(_native.NativeLibraryError, match="out of range"):
        multi_call(nat, rows, w, (M,))
    # the default budget: the per-device share of the free HBM, one sub-range per busy shard
    _native.check(nat.lib.fedagg_multi_set(nat._h, b"max_shard_bytes", 0), "multi_set")
    try:
        got = multi_call(nat, rows, w, idx)
        same_bits(got, first, "default budget")
        info = check_plan(nat, M, minimum_step=False)
        assert [i["ranges"] for i in info] == [1, 1], info
    finally:
        _native.check(nat.lib.fedagg_multi_set(nat._h, b"max_shard_bytes", SMALL), "multi_set")


# ------------------------------------------------------------------------------------- the reference's vectors
def _poison(sessions):
    for s in sessions:
        s.memset(s.buffer(1, 1 << 18), 0xFF, 1 << 18)
        s.sync()


def bf16_cases():
    for case, ns, clients, out in G.fedavg_cases(kinds=("bf16",)):
        rows = [[wire.float32_to_bf16(a) for a in c] for c in clients]
        for row, c in zip(rows, clients):
            for b, a in zip(row, c):
                assert b.dtype == wire.BF16 and np.array_equal(G.bits(wire.bf16_to_float32(b)), G.bits(a))
        yield case, [int(n) for n in ns], rows, out


def test_golden_vectors_through_every_route(native):
    from substrafl_amd.engine import AggregationEngine
    from substrafl_amd.multi_device import MultiDeviceEngine

    md = MultiDeviceEngine([0, 0, 0], max_shard_bytes=SMALL)
    small = AggregationEngine(device=0, max_bucket_bytes=SMALL)
    n = 0
    for case, ns, rows, out in bf16_cases():
        key = case["key"]
        got = native[3].fedavg_bf16(rows, ns)
        assert all(np.asarray(a).dtype == np.float32 for a in got)
        G.same(got, out, (key, "NativeMultiFedAvg.fedavg_bf16"))
        for tiled in (False, True):
            md.tiled, md.last_timing = tiled, {}
            _poison(md.sessions())
            G.same(md.fedavg_routed(rows, ns), out, (key, "MultiDeviceEngine.fedavg_routed", tiled))
            lt = md.last_timing
            assert set(lt) == {"shards", "total_s", "ranges"} and len(lt["shards"]) == len(lt["ranges"]) == 3
            for tm, rg in zip(lt["shards"], lt["ranges"]):
                if rg:
                    assert tm["layout"] == ("tiles" if tiled else "rows") and tm["ranges"] == len(rg)
                    assert all(hi - lo <= ALIGN for lo, hi in rg)
        G.same(md.fedavg_routed([wire.pack(x) for x in rows], ns, wire=True), out, (key, "packed rows, wire layers"))
        _poison([small.session()])
        small.last_timing = {}
        G.same(small.fedavg_routed(rows, ns), out, (key, "AggregationEngine.fedavg_routed past the budget"))
        assert small.last_timing["staging"] == "out-of-core"
        assert set(small.last_timing["out_of_core"]) == {"shards", "total_s", "ranges"}
        n += 1
    assert n == 2


# ------------------------------------------------------------------------------------- other inputs
def _model(dtypes, K, rng):
    shapes = [(40, 30), (1,), (7,), (1300,)]  # M = 2508
    return [[(rng.standard_normal(s) * 3).astype(dt) for s, dt in zip(shapes, dtypes)] for _ in range(K)]


@pytest.mark.parametrize("dtypes", [(np.float32,) * 4, (np.float16,) * 4, (np.float32, np.float64, np.float16, np.float32)],
                         ids=["f32", "f16", "mixed"])
def test_other_inputs_go_where_fedavg_sends_them(lib, dtypes):
    from substrafl_amd.engine import AggregationEngine
    from substrafl_amd.multi_device import MultiDeviceEngine

    rng = np.random.default_rng(9)
    pus, ns = _model(dtypes, 3, rng), samples(3, rng)
    for eng in (MultiDeviceEngine([0, 0], max_shard_bytes=SMALL), AggregationEngine(device=0),
                AggregationEngine(device=0, max_bucket_bytes=SMALL)):
        want = [np.array(a) for a in eng.fedavg(pus, ns)]
        timing = set(eng.last_timing)
        eng.last_timing = {}
        G.same(eng.fedavg_routed(pus, ns), want, (type(eng).__name__, "fedavg_routed is fedavg"))
        assert set(eng.last_timing) == timing


def test_a_bf16_layer_next_to_others_is_refused_as_before(lib):
    """Not uniformly wire.BF16: ``fedavg_routed`` is ``fedavg``, its refusals included."""
    from substrafl_amd.multi_device import MultiDeviceEngine

    rng = np.random.default_rng(10)
    pus = [[wire.float32_to_bf16(a[0]), a[1]] for a in _model((np.float32, np.float32), 3, rng)]
    md = MultiDeviceEngine([0, 0], max_shard_bytes=SMALL)
    for call in (md.fedavg, md.fedavg_routed):
        with pytest.raises(NotImplementedError):
            call(pus, [1, 2, 3])
    bf = [[a[0]] for a in pus]
    with pytest.raises(NotImplementedError):
        md.fedavg(bf, [1, 2, 3])  # the pinned refusal stands; the route is the new name
    assert md.fedavg_routed(bf, [1, 2, 3])[0].dtype == np.float32


# ------------------------------------------------------------------------------------- strategy level
def test_strategy_over_two_devices_on_bf16_states(lib, dummy_algo_class):
    """strategies.FedAvg with devices (0, 0) on bf16 shared states: what the one-device strategy
    returns, bit for bit.  Without ``fedavg_routed`` this raised NotImplementedError."""
    from substrafl_amd.engine import engine_for
    from substrafl_amd.schemas import FedAvgSharedState
    from substrafl_amd.strategies import FedAvg

    rng = np.random.default_rng(23)
    K = 4
    pus = [[values(s, rng).view(wire.BF16) for s in [(40, 30), (1,), (7,), (1300,)]] for _ in range(K)]
    states = [FedAvgSharedState(n_samples=n, parameters_update=p) for n, p in zip(samples(K, rng), pus)]
    before, after = ctypes.c_int(-1), ctypes.c_int(-2)
    lib.fedagg_device_get(ctypes.byref(before))
    one = FedAvg(algo=dummy_algo_class(), device=0).avg_shared_states(shared_states=states, _skip=True)
    one = [np.array(a) for a in one.avg_parameters_update]
    two = FedAvg(algo=dummy_algo_class(), device=(0, 0)).avg_shared_states(shared_states=states, _skip=True)
    lib.fedagg_device_get(ctypes.byref(after))
    assert after.value == before.value, "the caller's current device changed"
    lt = engine_for((0, 0)).last_timing
    assert sum(1 for x in lt["ranges"] if x) == 2 and [tm["ranges"] for tm in lt["shards"]] == [1, 1], lt
    assert all(a.dtype == np.float32 for a in one)
    G.same(two.avg_parameters_update, one, "FedAvg over (0, 0) against device 0")
    flat = np.concatenate([a.reshape(-1) for a in one])
    assert 0 < np.isfinite(flat).sum() and np.isnan(flat).mean() < 0.5


# ------------------------------------------------------------------------------------- the C demo
def test_the_c_demo_runs_bit_exact(lib, tmp_path):
    gcc = shutil.which("gcc")
    assert gcc is not None, "the demo needs gcc"
    exe, libdir = tmp_path / "fedavg_multi_bf16_demo", _native.LIB_PATH.parent
    subprocess.run([gcc, "-O2", "-ffp-contract=off", "-Wall", "-Werror", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "c" / "fedavg_multi_bf16_demo.c"), f"-L{libdir}", "-lfedagg",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), "0", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mismatches=0 again=0 used=2" in r.stdout, r.stdout
