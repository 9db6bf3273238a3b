"""FedAvg over the MXFP8 wire on the GPU (``libfedagg_mx.so``, include/fedagg_mx.h): the kernel, the
quantiser, the engine route and the client option, every comparison bit for bit (NaN by position)
against references that share no code with the kernels: ``wire.mxfp8_to_float32`` /
``wire.float32_to_mxfp8`` (NumPy) and the oracle's reference-structured FedAvg on the decoded
inputs, plus the golden vectors the reference itself produced."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch  # before the native libraries: one HIP runtime in the process

from mxfp8_cases import golden_cases, hand_blocks
from oracle import fedavg_reference_structure
from substrafl_amd import _native, _native_mx, wire
from substrafl_amd.engine import fedavg_weights
from substrafl_amd.wire import E4M3, E8M0

pytestmark = pytest.mark.gpu

GUARD = 64  # bytes / floats of sentinel before and after every output
SENT8, SENT32 = 0xA5, 0x7FA5A5A5  # the fp32 sentinel is a NaN no sum produces


@pytest.fixture(scope="module")
def mx():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _native.load()
    lib = _native_mx.load()
    yield lib
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


TILE, KGROUP = 4096, 4  # checked against fedagg_mx_blocking by test_blocking_is_what_the_cases_assume


def test_blocking_is_what_the_cases_assume(mx):
    assert _native_mx.blocking() == (TILE, KGROUP)


# ================================================================================ helpers
class Rows:
    """K byte rows, each 16-B aligned (pitch a multiple of 16), in one device buffer; ``off`` shifts
    every row by that many bytes (scale rows need no alignment)."""

    def __init__(self, a: np.ndarray, off: int = 0):
        K, n = a.shape
        self.pitch = -(-(n + off) // 16) * 16
        host = np.zeros((K, self.pitch), np.uint8)
        host[:, off: off + n] = a
        self.t = torch.from_numpy(host).cuda()
        self.ptrs = [self.t.data_ptr() + k * self.pitch + off for k in range(K)]


class Out:
    """M floats between two guard bands of the sentinel; ``off`` floats past 16-B alignment."""

    def __init__(self, M: int, off: int = 0):
        self.M, self.off = M, off
        self.t = torch.full((GUARD + off + M + GUARD,), SENT32, dtype=torch.int32, device="cuda")
        self.ptr = self.t.data_ptr() + 4 * (GUARD + off)

    def get(self) -> np.ndarray:
        g = self.t.cpu().numpy().view(np.uint32)
        lo = GUARD + self.off
        assert np.all(g[:lo] == SENT32) and np.all(g[lo + self.M:] == SENT32), "a guard band was written"
        return g[lo: lo + self.M].copy()


def _fedavg(lib, codes: Rows, scales: Rows, w, M, idx, out: Out, stream=None):
    K = len(codes.ptrs)
    h_w = (ctypes.c_float * K)(*[float(v) for v in w])
    h_idx = (ctypes.c_uint64 * max(1, len(idx)))(*[int(i) for i in idx])
    rc = lib.fedagg_mx_fedavg_e4m3(_native.ptr_array(codes.ptrs), _native.ptr_array(scales.ptrs), h_w, K, M, h_idx,
                                   len(idx), out.ptr, stream)
    assert rc == 0, lib.fedagg_mx_last_error()
    return h_w, h_idx


def _decode_rows(codes: np.ndarray, scales: np.ndarray) -> np.ndarray:
    return np.stack([wire.mxfp8_to_float32(c.view(E4M3), s.view(E8M0)) for c, s in zip(codes, scales)])


def _oracle(x: np.ndarray, ns, idx) -> np.ndarray:
    """The oracle (fed_avg.py:217-222 as the reference calls NumPy) over decoded rows [K, M] cut
    into layers: each index of ``idx`` a one-element layer (NumPy's pairwise order), every stretch
    between them a layer reduced along the client axis; a one-element stretch that is no numel == 1
    layer is doubled so that NumPy reduces it sequentially like its neighbours."""
    K, M = x.shape
    cuts, pos = [], 0
    for i in sorted(idx):
        if i > pos:
            cuts.append((pos, i, False))
        cuts.append((i, i + 1, True))
        pos = i + 1
    if M > pos:
        cuts.append((pos, M, False))
    pus = [[np.repeat(x[k, a:b], 2) if (b - a == 1 and not one) else x[k, a:b] for a, b, one in cuts] for k in range(K)]
    with np.errstate(all="ignore"):
        res = fedavg_reference_structure(pus, ns)
    return np.concatenate([np.asarray(r).reshape(-1)[: b - a] for r, (a, b, _) in zip(res, cuts)]).astype(np.float32)


def _same(got_bits: np.ndarray, ref: np.ndarray, what: str):
    ref = np.ascontiguousarray(ref, np.float32)
    want = ref.view(np.uint32)
    nan = np.isnan(ref)
    got_nan = (got_bits & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    assert np.array_equal(got_nan, nan), f"{what}: NaN positions differ"
    bad = np.flatnonzero((got_bits != want) & ~nan)
    assert bad.size == 0, (f"{what}: {bad.size} of {want.size} elements differ; first at {bad[:6]}: got "
                           f"{[hex(int(v)) for v in got_bits[bad[:6]]]} reference {[hex(int(v)) for v in want[bad[:6]]]}")


def _samples(K: int):
    return [int(v) for v in np.random.default_rng(1000 + K).integers(100, 10000, K)]


def _cancelling(rng, K: int, M: int):
    """Random codes over the whole table (two NaN codes planted among them) under scales of a moderate
    band; every odd client is the negation of the client before it, and their sample counts differ
    by one, so most of every sum cancels."""
    codes = rng.integers(0, 256, (K, M)).astype(np.uint8)
    codes[(codes & 0x7F) == 0x7F] ^= 0x01  # NaN codes only where planted: with many clients every sum would be NaN
    codes[0, 5 % M] = 0x7F
    codes[K // 2, M // 2] = 0xFF
    scales = rng.integers(117, 138, (K, -(-M // 32))).astype(np.uint8)
    codes[1::2] = codes[: 2 * (K // 2): 2] ^ 0x80
    scales[1::2] = scales[: 2 * (K // 2): 2]
    ns = [5000 + (k % 2) for k in range(K)]
    return codes, scales, ns


# ================================================================================ decode, exhaustively
def test_exhaustive_decode(mx):
    """K = 1, weight 1: all 256 codes under each of the 256 scale bytes, 8 blocks per scale: the
    vector walk's decoder against wire.mxfp8_to_float32 through the oracle, fp32-subnormal results,
    overflow to inf and s == 255 included.  The same rows shifted off the vector path (an output
    that is not 16-B aligned) check the plain C++ decoder."""
    M = 65536
    scales = np.repeat(np.arange(256, dtype=np.uint8), 8)[None, :]  # 2048 blocks
    codes = np.tile(np.arange(256, dtype=np.uint8), 256)[None, :]   # block b holds codes 32 (b % 8) .. + 32
    assert scales.shape[1] * 32 == M == codes.shape[1]
    ref = _oracle(_decode_rows(codes, scales), [3], [])
    dec = wire.mxfp8_to_float32(codes[0].view(E4M3), scales[0].view(E8M0))
    keep = ~np.isnan(dec) & (dec != 0)  # weight 3 / 3 = 1: the oracle returns the decoded values (+0.0 + -0.0 is +0.0)
    assert np.array_equal(ref.view(np.uint32)[keep], dec.view(np.uint32)[keep])
    sub = (np.abs(dec) > 0) & (np.abs(dec) < np.finfo(np.float32).tiny)
    assert sub.sum() > 500 and np.isinf(dec).sum() > 500 and np.isnan(dec).sum() == 256 * 2 + 256 - 2
    c, s = Rows(codes), Rows(scales)
    for off in (0, 1):
        out = Out(M, off)
        _fedavg(mx, c, s, [1.0], M, [], out)
        torch.cuda.synchronize()
        _same(out.get(), ref, f"exhaustive decode, output offset {off}")


# ================================================================================ geometry
M_SIZES = [1, 15, 16, 17, 31, 32, 33, 1023, TILE - 1, TILE, TILE + 1, 2 * TILE + 17]
K_SIZES = sorted({1, 2, 3, KGROUP - 1, KGROUP + 1, 8, 9, 33, 64, 65, 257})


@pytest.mark.parametrize("K", K_SIZES)
def test_geometry(mx, K):
    """Every size at which the kernel changes path: the scalar tail alone, whole vectors, partial
    and whole workgroup steps, several steps; client groups, their remainder, two and three chunks
    of 128 clients.  One draw per K at the largest M, the smaller sizes are its prefixes."""
    rng = np.random.default_rng(40 + K)
    Mmax = max(M_SIZES)
    codes, scales, ns = _cancelling(rng, K, Mmax)
    w = fedavg_weights(ns, "f32")
    for M in M_SIZES:
        nb = -(-M // 32)
        cm, sm = np.ascontiguousarray(codes[:, :M]), np.ascontiguousarray(scales[:, :nb])
        ref = _oracle(_decode_rows(cm, sm), ns, [])
        out = Out(M)
        _fedavg(mx, Rows(cm), Rows(sm, off=M % 7), w, M, [], out)  # scale rows at any alignment
        torch.cuda.synchronize()
        _same(out.get(), ref, f"K={K} M={M}")


def test_unaligned_output_takes_the_scalar_walk(mx):
    rng = np.random.default_rng(7)
    K, M = 5, TILE + 33
    codes, scales, ns = _cancelling(rng, K, M)
    ref = _oracle(_decode_rows(codes, scales), ns, [])
    for off in (1, 2, 3):
        out = Out(M, off)
        _fedavg(mx, Rows(codes), Rows(scales), fedavg_weights(ns, "f32"), M, [], out)
        torch.cuda.synchronize()
        _same(out.get(), ref, f"output offset {off}")


# ================================================================================ numel == 1 layers
@pytest.mark.parametrize("K", [7, 8, 9, 129, 200, 255, 256])
def test_numel_one_layers(mx, K):
    """numel == 1 layers at flat positions 0, 31, 32 and last take NumPy's pairwise tree over the K
    products: below 8 terms, the 8-accumulator leaf, two leaves (129, 200, 256) and a right half
    that splits again (255)."""
    rng = np.random.default_rng(90 + K)
    for M in (70, TILE + 35):
        idx = [0, 31, 32, M - 1]
        codes, scales, ns = _cancelling(rng, K, M)
        ns = _samples(K)
        ref = _oracle(_decode_rows(codes, scales), ns, idx)
        seq = _oracle(_decode_rows(codes, scales), ns, [])
        out = Out(M)
        _fedavg(mx, Rows(codes), Rows(scales), fedavg_weights(ns, "f32"), M, idx, out)
        torch.cuda.synchronize()
        _same(out.get(), ref, f"K={K} M={M} numel-1")
        if K >= 9:  # the patch matters: the sequential order gives other bits somewhere
            assert not np.array_equal(ref.view(np.uint32)[idx], seq.view(np.uint32)[idx])


def test_many_numel_one_layers(mx):
    """More indices than one launch of the pairwise kernel takes (64)."""
    rng = np.random.default_rng(3)
    K, M = 130, 600
    idx = list(range(0, 3 * 70, 3))
    codes, scales, _ = _cancelling(rng, K, M)
    ns = _samples(K)
    out = Out(M)
    _fedavg(mx, Rows(codes), Rows(scales), fedavg_weights(ns, "f32"), M, idx, out)
    torch.cuda.synchronize()
    _same(out.get(), _oracle(_decode_rows(codes, scales), ns, idx), "70 numel-1 layers")


# ================================================================================ golden
GOLDEN = golden_cases()


@pytest.mark.parametrize("case", GOLDEN, ids=[c[0] for c in GOLDEN])
def test_golden_through_the_entry_point(mx, case):
    key, _kind, updates, ns, want = case
    codes = np.stack([np.concatenate([a["e4m3fn"].reshape(-1) for a in u[:-1]]) for u in updates])
    scales = np.stack([u[-1]["e8m0"] for u in updates])
    cuts = np.cumsum([0] + [w.size for w in want])
    idx = [int(a) for a, w in zip(cuts, want) if w.size == 1]
    out = Out(codes.shape[1])
    _fedavg(mx, Rows(codes), Rows(scales), fedavg_weights(ns, "f32"), codes.shape[1], idx, out)
    torch.cuda.synchronize()
    _same(out.get(), np.concatenate([w.reshape(-1) for w in want]), key)


@pytest.mark.parametrize("case", GOLDEN, ids=[c[0] for c in GOLDEN])
def test_golden_through_the_strategy(mx, case):
    from substrafl_amd.engine import engine_for
    from substrafl_amd.schemas import FedAvgSharedState
    from substrafl_amd.strategies import FedAvg

    class _Algo:
        strategies = ["Federated Averaging"]

    key, _kind, updates, ns, want = case
    states = [FedAvgSharedState(n_samples=n, parameters_update=u) for n, u in zip(ns, updates)]
    got = FedAvg(algo=_Algo(), device=0).avg_shared_states(shared_states=states, _skip=True).avg_parameters_update
    assert engine_for(0).last_timing["staging"] == "mxfp8-host-rows"
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert isinstance(g, wire.BucketArray) and g.dtype == np.float32 and g.shape == w.shape
        assert np.array_equal(np.asarray(g).view(np.uint32), w.view(np.uint32)), key
    assert wire.flat_of(list(got)) is not None  # L layers of one bucket


# ================================================================================ quantiser
def _quantize(lib, x: np.ndarray, kind: str, off: int = 0, stream=None):
    """``x``: fp32 values, or bf16 bit patterns (uint16); ``off``: elements past 16-B alignment."""
    M = x.size
    nb = -(-M // 32)
    isz = x.dtype.itemsize
    src = torch.zeros(M + off + 8, dtype=torch.int32 if isz == 4 else torch.int16, device="cuda")
    src[off: off + M] = torch.from_numpy(x.view(np.int32 if isz == 4 else np.int16)).cuda()
    dst = torch.full((GUARD + M + 3 + nb + GUARD,), SENT8, dtype=torch.uint8, device="cuda")
    d_codes = dst.data_ptr() + GUARD
    d_scales = d_codes + M + 3  # neither output needs an alignment
    rc = lib.fedagg_mx_quantize(src.data_ptr() + off * isz, _native.FEDAGG_F32 if kind == "f32" else _native.FEDAGG_BF16,
                                M, d_codes, d_scales, stream)
    assert rc == 0, lib.fedagg_mx_last_error()

    def read():
        g = dst.cpu().numpy()
        assert np.all(g[:GUARD] == SENT8) and np.all(g[GUARD + M: GUARD + M + 3] == SENT8)
        assert np.all(g[GUARD + M + 3 + nb:] == SENT8), "the quantiser wrote past its outputs"
        return g[GUARD: GUARD + M].copy(), g[GUARD + M + 3: GUARD + M + 3 + nb].copy()

    return read, (src, dst)


def _bf16_bits(x: np.ndarray) -> np.ndarray:
    return wire.float32_to_bf16(x)["bfloat16"]


def _check_quantize(lib, x32: np.ndarray, what: str, offs=(0,)):
    for kind in ("f32", "bf16"):
        stored = x32 if kind == "f32" else _bf16_bits(x32)
        values = x32 if kind == "f32" else wire.bf16_to_float32(stored.view(wire.BF16))
        want_c, want_s = wire.float32_to_mxfp8(values)
        for off in offs:
            read, keep = _quantize(lib, stored, kind, off)
            torch.cuda.synchronize()
            got_c, got_s = read()
            assert np.array_equal(got_s, want_s["e8m0"]), f"{what} {kind} offset {off}: scales differ"
            bad = np.flatnonzero(got_c != want_c["e4m3fn"])
            assert bad.size == 0, (f"{what} {kind} offset {off}: {bad.size} codes differ, first at {bad[:5]}: "
                                   f"{got_c[bad[:5]]} vs {want_c['e4m3fn'][bad[:5]]} for {values[bad[:5]]}")


@pytest.mark.parametrize("name", sorted(hand_blocks()))
def test_quantize_hand_made_blocks(mx, name):
    x, want_scale, want = hand_blocks()[name]
    _check_quantize(mx, x, name)
    read, keep = _quantize(mx, x, "f32")  # and against the values worked out by hand
    torch.cuda.synchronize()
    codes, scales = read()
    assert list(scales) == want_scale and all(codes[p] == c for p, c in want.items())


def test_quantize_random(mx):
    rng = np.random.default_rng(21)
    for M in (1, 31, 33, TILE + 1):
        x = (rng.standard_normal(M) * np.exp(rng.uniform(-60, 60, M))).astype(np.float32)
        if M > 40:
            x[5], x[40] = 0.0, -0.0
        _check_quantize(mx, x, f"random M={M}", offs=(0, 1))  # 1: a buffer at an odd element offset
    # every scale byte the rule can produce, ties and the 464 bump among thousands of blocks
    M = 32 * 3000 + 5
    x = (rng.standard_normal(M) * np.exp2(rng.integers(-149, 128, M // 32 + 1).repeat(32)[:M])).astype(np.float32)
    x[np.isinf(x)] = np.float32(3e38)
    _check_quantize(mx, x, "every exponent")


def test_quantize_then_average_is_the_oracle_on_the_decoded_values(mx):
    """The two entry points together, device-resident: what a client produces is what the
    aggregator decodes."""
    rng = np.random.default_rng(5)
    K, M = 3, 2 * TILE + 17
    xs = (rng.standard_normal((K, M)) * 0.05).astype(np.float32)
    enc = [wire.float32_to_mxfp8(x) for x in xs]
    codes, scales = np.stack([c["e4m3fn"] for c, _ in enc]), np.stack([s["e8m0"] for _, s in enc])
    for k in range(K):
        read, keep = _quantize(mx, xs[k], "f32")
        torch.cuda.synchronize()
        c, s = read()
        assert np.array_equal(c, codes[k]) and np.array_equal(s, scales[k])
    ns = _samples(K)
    out = Out(M)
    _fedavg(mx, Rows(codes), Rows(scales), fedavg_weights(ns, "f32"), M, [], out)
    torch.cuda.synchronize()
    _same(out.get(), _oracle(_decode_rows(codes, scales), ns, []), "quantised updates")


# ================================================================================ stream contract
def test_stream_contract(mx):
    """Both entry points on a non-blocking side stream (only that stream is synchronised), then
    captured once into a graph -- nothing may run while capturing, the host arrays are trashed
    afterwards -- and replayed over new data in the same buffers: the same bits."""
    rng = np.random.default_rng(13)
    K, M, idx = 130, TILE + 37, [0, 100, TILE + 36]
    nb = -(-M // 32)
    ns = _samples(K)
    w = fedavg_weights(ns, "f32")
    data = {}
    for ds in "AB":
        x = (rng.standard_normal(M) * np.exp(rng.uniform(-8, 8, M))).astype(np.float32)
        codes, scales, _ = _cancelling(rng, K, M)
        data[ds] = (x, codes, scales, _oracle(_decode_rows(codes, scales), ns, idx), wire.float32_to_mxfp8(x))
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    assert sp != 0
    c, s, out = Rows(data["A"][1]), Rows(data["A"][2]), Out(M)
    src = torch.zeros(M, dtype=torch.float32, device="cuda")
    q = torch.full((M + nb,), SENT8, dtype=torch.uint8, device="cuda")

    def put(ds):
        x, codes, scales, _, _ = data[ds]
        host_c, host_s = np.zeros((K, c.pitch), np.uint8), np.zeros((K, s.pitch), np.uint8)
        host_c[:, :M], host_s[:, :nb] = codes, scales
        c.t.copy_(torch.from_numpy(host_c), non_blocking=False)
        s.t.copy_(torch.from_numpy(host_s), non_blocking=False)
        src.copy_(torch.from_numpy(x))
        out.t.fill_(SENT32)
        q.fill_(SENT8)

    def call():
        keep = _fedavg(mx, c, s, w, M, idx, out, sp)
        assert mx.fedagg_mx_quantize(src.data_ptr(), _native.FEDAGG_F32, M, q.data_ptr(), q.data_ptr() + M, sp) == 0
        return keep

    def check(ds, stage):
        _, _, _, ref, (qc, qs) = data[ds]
        _same(out.get(), ref, f"fedavg, {stage}")
        g = q.cpu().numpy()
        assert np.array_equal(g[:M], qc["e4m3fn"]) and np.array_equal(g[M:], qs["e8m0"]), f"quantize, {stage}"

    with torch.cuda.stream(stream):
        put("A")
        call()
    stream.synchronize()
    check("A", "eager on the side stream")

    with torch.cuda.stream(stream):
        put("A")
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        h_w, h_idx = call()
    torch.cuda.synchronize()
    assert np.all(out.get() == SENT32) and bool((q == SENT8).all()), "a kernel ran during the capture"
    for i in range(K):
        h_w[i] = float("nan")
    for i in range(len(idx)):
        h_idx[i] = 1 << 63
    del h_w, h_idx
    for ds in ("B", "A"):
        with torch.cuda.stream(stream):
            put(ds)
            graph.replay()
        torch.cuda.synchronize()
        check(ds, f"replay over data set {ds}")
    del graph


# ================================================================================ engine refusals on the device
def test_engine_refusals_name_their_route(mx):
    from substrafl_amd.engine import AggregationEngine, engine_for
    from substrafl_amd.schemas import ScaffoldSharedState
    from substrafl_amd.strategies import Scaffold

    class _Algo:
        strategies = ["Federated Averaging", "Scaffold"]

    _key, _kind, updates, ns, want = GOLDEN[1]
    with pytest.raises(NotImplementedError, match="out-of-core route has no MXFP8 path"):
        AggregationEngine(device=0, max_bucket_bytes=64).fedavg_routed(updates, ns)
    with pytest.raises(NotImplementedError, match="MultiDeviceEngine.fedavg_routed.*no MXFP8 path"):
        engine_for([0, 0]).fedavg_routed(updates, ns)
    with pytest.raises(NotImplementedError, match="client-sharded FedAvg: no MXFP8 path"):
        from substrafl_amd.sharding import client_sharded_fedavg, LoopbackGroup

        client_sharded_fedavg(updates, ns, transport=LoopbackGroup(1).transport(0))
    c = [np.zeros(a.shape, np.float32) for a in updates[0]]
    states = [ScaffoldSharedState(parameters_update=u, control_variate_update=u, n_samples=n, server_control_variate=c)
              for u, n in zip(updates, ns)]
    with pytest.raises(NotImplementedError, match="MXFP8"):
        Scaffold(algo=_Algo(), aggregation_lr=1.0, device=0).avg_shared_states(shared_states=states, _skip=True)


# ================================================================================ end to end
def test_federation_end_to_end(mx):
    """Two ``accelerate_algo(TorchFedAvgAlgo, wire="mxfp8")`` clients -- an fp32 MLP and a bf16 copy
    of it -- under ``accelerate(FedAvg)`` for two rounds: the shared states are E4M3 layers plus one
    E8M0 array in one bucket, equal to the host encoder on the client's delta; the average is the
    oracle on the decoded states; each client's weights after applying it are torch's ``w += avg``
    with the promotion of the existing paths."""
    import standin_substrafl.strategies as ss
    from standin_substrafl.algorithms.pytorch import TorchFedAvgAlgo
    from standin_substrafl.index_generator import NpIndexGenerator

    from substrafl_amd.integration import accelerate, accelerate_algo

    def data(n, seed):
        r = np.random.default_rng(seed)
        x = r.standard_normal((n, 6)).astype(np.float32)
        return x, (x @ r.standard_normal((6, 1))).astype(np.float32)

    def algo(dtype, client):
        torch.manual_seed(7)
        model = torch.nn.Sequential(torch.nn.Linear(6, 24), torch.nn.BatchNorm1d(24), torch.nn.ReLU(),
                                    torch.nn.Linear(24, 1)).to(dtype)

        class XY(torch.utils.data.Dataset):
            def __init__(self, data_from_opener, is_inference=False):
                self.x, self.y = data_from_opener

            def __getitem__(self, i):
                return torch.from_numpy(self.x[i]).to(dtype), torch.from_numpy(self.y[i]).to(dtype)

            def __len__(self):
                return len(self.x)

        class MyAlgo(TorchFedAvgAlgo):
            def __init__(self):
                super().__init__(model=model, criterion=torch.nn.MSELoss(),
                                 optimizer=torch.optim.SGD(model.parameters(), lr=0.02),
                                 index_generator=NpIndexGenerator(batch_size=32, num_updates=3, seed=11 + client),
                                 dataset=XY, with_batch_norm_parameters=True, disable_gpu=False)

        return accelerate_algo(MyAlgo, wire="mxfp8")()

    def weights(a):
        from substrafl_amd.algorithms.weight_manager import model_parameters

        return [p.data.detach().clone() for p in model_parameters(a.model, True)()]

    cudnn = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False  # the native BatchNorm kernels: deterministic training
    try:
        algos = [algo(torch.float32, 0), algo(torch.bfloat16, 1)]
        datasets = [data(120, 1), data(77, 2)]
        strategy = accelerate(ss.FedAvg)(algo=algos[0])
        avg = None
        for rnd in range(2):
            before = [weights(a) for a in algos]
            states = [a.train(data_from_opener=d, shared_state=avg, _skip=True) for a, d in zip(algos, datasets)]
            if avg is not None:  # the average of the round before went onto the model first
                for a, w0 in zip(algos, before):
                    # train() set the model back to its pre-train weights: those are w0 += avg
                    for p, w, u in zip(weights(a), w0, avg.avg_parameters_update):
                        w += 1.0 * torch.from_numpy(np.asarray(u)).to(w.device)
                        assert torch.equal(p.view(torch.int16 if p.dtype == torch.bfloat16 else torch.int32),
                                           w.view(torch.int16 if w.dtype == torch.bfloat16 else torch.int32)), rnd
            M = sum(int(np.prod(t.shape)) for t in before[0])
            for st in states:
                pu = list(st.parameters_update)
                assert wire.is_mxfp8(pu) and wire.mxfp8_check(pu) == M
                assert [a.shape for a in pu[:-1]] == [tuple(t.shape) for t in before[0]]
                assert all(isinstance(a, wire.BucketArray) for a in pu) and len({id(a._bucket) for a in pu}) == 1
                assert pu[0]._bucket.flat.nbytes == M + -(-M // 32)  # 1.03 bytes per parameter, one buffer
                # canonical: what the host encoder gives for the decoded values
                dec = wire.mxfp8_to_float32(pu[:-1], pu[-1])
                assert np.isfinite(np.concatenate([d.reshape(-1) for d in dec])).all()
                c2, s2 = wire.float32_to_mxfp8(dec)
                assert np.array_equal(s2, pu[-1]) and all(np.array_equal(a, b) for a, b in zip(c2, pu[:-1]))
            avg = strategy.avg_shared_states(shared_states=states, _skip=True)
            decoded = [wire.mxfp8_to_float32(list(st.parameters_update)[:-1], st.parameters_update[-1]) for st in states]
            ref = fedavg_reference_structure(decoded, [st.n_samples for st in states])
            assert len(avg.avg_parameters_update) == len(ref)
            for g, r in zip(avg.avg_parameters_update, ref):
                assert g.dtype == np.float32 and g.shape == r.shape
                assert np.array_equal(np.asarray(g).view(np.uint32), r.view(np.uint32)), rnd
            assert any(np.any(np.asarray(g) != 0) for g in avg.avg_parameters_update)  # a real training run
    finally:
        torch.backends.cudnn.enabled = cudnn


def test_fp16_model_is_refused(mx):
    from substrafl_amd.algorithms import weight_manager as wm

    for dt in (torch.float16, torch.float64):
        with pytest.raises(NotImplementedError, match="wire='mxfp8'"):
            wm.export_mxfp8([torch.zeros(40, dtype=dt, device="cuda")])
    out = wm.export_mxfp8([torch.full((5, 8), 0.75, device="cuda"), torch.zeros(1, device="cuda")])
    assert wire.is_mxfp8(out) and out[0].shape == (5, 8) and out[-1].shape == (2,)
    assert np.all(wire.mxfp8_to_float32(out[:-1], out[-1])[0] == np.float32(0.75))


# ================================================================================ the C demo
def test_the_c_demo_runs_bit_exact(mx, tmp_path):
    import shutil
    import subprocess

    from test_mx_abi import demo_command

    assert shutil.which("gcc") is not None, "the demo needs gcc"
    exe = tmp_path / "fedavg_mx_demo"
    subprocess.run(demo_command(exe), check=True)
    r = subprocess.run([str(exe), "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mismatches=0 refused=-1" in r.stdout, r.stdout
