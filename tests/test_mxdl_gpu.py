"""The MXFP8 downlink on the GPU (``libfedagg_mxdl.so``, include/fedagg_mxdl.h), bit for bit against
references that share no code with the kernels: ``wire.mxfp8_to_float32`` / ``wire.mxfp4_to_float32``,
the oracle's reference-structured FedAvg on the decoded rows, then ``wire.float32_to_mxfp8``."""

from __future__ import annotations

import numpy as np
import pytest
import torch  # before the native libraries: one HIP runtime in the process

from oracle import fedavg_reference_structure
from substrafl_amd import _native, _native_mxdl, wire
from substrafl_amd.engine import AggregationEngine, fedavg_weights
from substrafl_amd.wire import E2M1X2, E4M3, E8M0
from test_mxfp8_gpu import Rows, _oracle

pytestmark = pytest.mark.gpu

GUARD, SENT = 64, 0xA5
TILE, VEC, KGROUP = 4096, 16, 4  # asserted against fedagg_mxdl_blocking by the fixture
KINDS = {"e4m3": _native_mxdl.E4M3, "e2m1": _native_mxdl.E2M1}


@pytest.fixture(scope="module")
def dl():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _native.load()
    assert _native_mxdl.blocking() == (TILE, VEC, KGROUP)
    yield _native_mxdl
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


class Guarded:
    """``n`` elements of ``dtype`` between two guard bands; ``off`` elements past 16-B alignment."""

    def __init__(self, n: int, off: int = 0, dtype=torch.uint8, fill=None):
        body = torch.full((n,), SENT, dtype=dtype) if fill is None else fill
        host = torch.cat([torch.full((GUARD + off,), SENT, dtype=dtype), body, torch.full((GUARD,), SENT, dtype=dtype)])
        e = host.element_size()
        self.lo, self.hi, self.host = (GUARD + off) * e, (GUARD + off + n) * e, host.view(torch.uint8).numpy().copy()
        self.t = host.cuda()
        self.ptr = self.t.data_ptr() + self.lo

    def get(self) -> np.ndarray:
        g = self.t.cpu().view(torch.uint8).numpy()
        assert np.array_equal(g[: self.lo], self.host[: self.lo]) and np.array_equal(g[self.hi:], self.host[self.hi:]), \
            "a guard band was written"
        return g[self.lo: self.hi].copy()


def _encode(kind: str, x: np.ndarray):
    """Client rows x [K, M] through the wire's encoder: (code bytes [K, .], scale bytes [K, nb])."""
    if kind == "e4m3":
        enc = [wire.float32_to_mxfp8(r) for r in x]
        return np.stack([c["e4m3fn"] for c, _ in enc]), np.stack([s["e8m0"] for _, s in enc])
    enc = [wire.float32_to_mxfp4(r) for r in x]
    return np.stack([c["e2m1x2"] for c, _, _ in enc]), np.stack([s["e8m0"] for _, s, _ in enc])


def _decode(kind: str, codes: np.ndarray, scales: np.ndarray, M: int) -> np.ndarray:
    if kind == "e4m3":
        return np.stack([wire.mxfp8_to_float32(c[:M].view(E4M3), s.view(E8M0)) for c, s in zip(codes, scales)])
    return np.stack([wire.mxfp4_to_float32(c[: -(-M // 2)].copy().view(E2M1X2), s.view(E8M0), M)
                     for c, s in zip(codes, scales)])


def _reference(kind, codes, scales, M, ns, idx=()):
    """(code bytes, scale bytes, the fp32 average) the contract asks for."""
    nb = -(-M // 32)
    avg = _oracle(_decode(kind, codes, scales[:, :nb], M), ns, list(idx))
    c, s = wire.float32_to_mxfp8(avg)
    return c["e4m3fn"], s["e8m0"], avg


def _run(dl, kind, codes, scales, M, ns, idx=(), c_off=0, s_off=0):
    nb = -(-M // 32)
    nc = M if kind == "e4m3" else -(-M // 2)
    rc, rs = Rows(np.ascontiguousarray(codes[:, :nc])), Rows(np.ascontiguousarray(scales[:, :nb]), off=M % 7)
    oc, os_ = Guarded(M, c_off), Guarded(nb, s_off)
    dl.fedavg(KINDS[kind], rc.ptrs, rs.ptrs, fedavg_weights(ns, "f32"), M, list(idx), oc.ptr, os_.ptr, 0)
    torch.cuda.synchronize()
    return oc.get(), os_.get()


def _check(got, want, what):
    for name, g, w in zip(("codes", "scales"), got, want):
        assert np.array_equal(g, w), f"{what}: {name} differ at {np.flatnonzero(g != w)[:6]}"


def _client_rows(rng, K: int, M: int) -> np.ndarray:
    """fp32 client rows over a wide range of block magnitudes; every odd client negates the one
    before it and their sample counts differ by one, so most of every sum cancels."""
    x = rng.standard_normal((K, M)).astype(np.float32) * np.exp2(rng.integers(-12, 12, (K, -(-M // 8)))).repeat(8, 1)[:, :M]
    x[1::2] = -x[: 2 * (K // 2): 2]
    return x.astype(np.float32)


M_SIZES = [1, 15, 16, 17, 31, 32, 33, 64 * VEC - 1, TILE, TILE + VEC + 5, 2 * TILE + 33]


@pytest.mark.parametrize("K", [1, 3, 4, 9, 128])
@pytest.mark.parametrize("kind", ["e4m3", "e2m1"])
def test_fused_kernel_against_numpy(dl, kind, K):
    """Every size at which the kernel changes path, at both output alignments.  One draw per case at
    the largest M; the smaller sizes are its prefixes (for e2m1 an odd M leaves the next element's
    code in the last byte's high nibble, which must not be read)."""
    rng = np.random.default_rng(100 * K + len(kind))
    codes, scales = _encode(kind, _client_rows(rng, K, max(M_SIZES)))
    ns = [5000 + (k % 2) for k in range(K)]
    for M in M_SIZES:
        want = _reference(kind, codes, scales, M, ns)[:2]
        for c_off, s_off in ((0, 0), (0, 3), (1, 0), (1, 3)):
            _check(_run(dl, kind, codes, scales, M, ns, (), c_off, s_off), want, f"{kind} K={K} M={M} +{c_off},{s_off}")


# name -> (the 4 clients' values at one position of the block, raw edit, the block's expected scale byte)
HAND = {
    "amax_464": ([1536.0, 256.0, 64.0, 0.0], None, 127),            # 0.25 * 1856: the tie that still rounds to 448
    "amax_464_next": ([1536.0, 256.0, 64.0, 2.0 ** -13], None, 128),  # one ulp above: the bump
    "clamp_low": ([2.0 ** -120] * 4, None, 0),                       # e = -128 clamps to -127
    "largest_scale": ([1.5 * 2.0 ** 127] * 4, None, 246),            # the largest e a finite fp32 reaches
    "negative_zeros": ([-0.0] * 4, None, 127),
    "nan_block": ([1.0] * 4, "nan", 255),                            # one client's scale byte 255
    "overflow_to_inf": ([1.0] * 4, "inf", 255),                      # finite codes under scale 254 decode to inf
}


@pytest.mark.parametrize("name", sorted(HAND))
@pytest.mark.parametrize("kind", ["e4m3", "e2m1"])
def test_hand_made_averages(dl, kind, name):
    """K = 4 clients of equal weight 0.25, so every sum below is exact: the block sits once in the
    first lane pair and once in the last, partial block (its position in the pair's second lane,
    which owns 4 of its 16 elements)."""
    vals, edit, want_s = HAND[name]
    K, M, ns = 4, 64 + 20, [7, 7, 7, 7]
    x = np.zeros((K, M), np.float32)
    x[:, 32:64] = _client_rows(np.random.default_rng(5), K, 32)
    spots = (3, 64 + 17)
    for p in spots:
        x[:, p] = vals
    if name == "negative_zeros":
        x[:, :32], x[:, 64:] = -0.0, -0.0
    codes, scales = _encode(kind, x)
    assert np.array_equal(_decode(kind, codes, scales, M)[:, spots].view(np.uint32), x[:, spots].view(np.uint32))  # exact
    for p in spots:
        if edit == "nan":
            scales[1, p // 32] = 255
        if edit == "inf":
            scales[0, p // 32] = 254
            if kind == "e4m3":
                codes[0, p] = 0x7E
            else:
                codes[0, p // 2] = 0x7 << (4 * (p % 2))
    want_c, want_s_row, avg = _reference(kind, codes, scales, M, ns)
    assert [int(want_s_row[p // 32]) for p in spots] == [want_s, want_s], (name, want_s_row)
    if name == "amax_464":
        assert avg[3] == 464.0 and want_c[3] == 0x7E
    if name == "overflow_to_inf":
        assert np.isinf(avg[3]) and np.isfinite(_decode(kind, codes, scales, M)[1:]).all()
    _check(_run(dl, kind, codes, scales, M, ns), (want_c, want_s_row), f"{kind} {name}")


def test_identity(dl):
    """K = 1 with weight 1.0 over rows the encoder produced: encode(decode(.)) is the identity, so the
    bytes come back (a negative zero as +0: the sum starts from +0.0)."""
    M = TILE + 33
    codes, scales = _encode("e4m3", _client_rows(np.random.default_rng(8), 1, M))
    _check(_run(dl, "e4m3", codes, scales, M, [3]), (np.where(codes[0] == 0x80, 0, codes[0]), scales[0]), "identity")


def _pow2_samples(K: int):
    """Sample counts whose weights are exact: 1 / 2^m for all clients but the last."""
    return [1] * (K - 1) + [(1 << (K - 1).bit_length()) - (K - 1)]


def _plant(x: np.ndarray, ns, idx):
    """At every listed element the weighted terms become X, 0, h, h, -X, 0, .. with X = 2^24 h: in
    client order X + h ties back to X twice and the sum is 0; NumPy's tree (at 8 terms and above)
    adds h + h first and gives 2 h, the largest average of its block -- so codes AND scale differ."""
    w = np.float32(ns[0]) / np.float32(sum(ns))
    for n, i in enumerate(idx):
        h = 2.0 ** (15 + n)
        x[:, i] = 0.0
        x[[0, 2, 3, 4], i] = np.array([2.0 ** 24 * h, h, h, -(2.0 ** 24) * h], np.float32) / w


def _orders_differ(kind, codes, scales, M, ns, idx):
    """The contract's bytes, after asserting that the sequential order would give other bytes at
    every listed element and in every scale byte of their blocks."""
    want_c, want_s, _ = _reference(kind, codes, scales, M, ns, idx)
    seq_c, seq_s, _ = _reference(kind, codes, scales, M, ns)
    assert (want_c[idx] != seq_c[idx]).all() and (want_s[np.asarray(idx) // 32] != seq_s[np.asarray(idx) // 32]).all()
    return want_c, want_s


@pytest.mark.parametrize("K", [9, 128])
@pytest.mark.parametrize("kind", ["e4m3", "e2m1"])
def test_numel_one_indices(dl, kind, K):
    """numel == 1 layers at flat position 0, two in one block, and as the last element of a partial
    block take NumPy's pairwise tree before their block is scaled."""
    M, idx, ns = 100, [0, 40, 45, 99], _pow2_samples(K)
    x = _client_rows(np.random.default_rng(90 + K), K, M)
    _plant(x, ns, idx)
    codes, scales = _encode(kind, x)
    want = _orders_differ(kind, codes, scales, M, ns, idx)
    _check(_run(dl, kind, codes, scales, M, ns, idx, 1, 0), want, f"{kind} K={K} numel-1")


@pytest.mark.parametrize("kind, K", [("e4m3", 129), ("e4m3", 9), ("e2m1", 9)])
def test_two_step_equals_fused(dl, monkeypatch, kind, K):
    shapes = [(5, 8), (1,), (33,), (1,), (TILE + 7,)]
    M, ns, idx = sum(int(np.prod(s)) for s in shapes), _pow2_samples(K), [40, 74]
    x = _client_rows(np.random.default_rng(K), K, M)
    _plant(x, ns, idx)
    cuts = np.cumsum([int(np.prod(s)) for s in shapes])[:-1]
    ups = []
    for row in x:
        layers = [a.reshape(s) for a, s in zip(np.split(row, cuts), shapes)]
        enc = wire.float32_to_mxfp8(layers) if kind == "e4m3" else wire.float32_to_mxfp4(layers)
        ups.append([*enc[0], enc[1]] if kind == "e4m3" else list(enc))
    want = _orders_differ(kind, *_encode(kind, x), M, ns, idx)
    eng = AggregationEngine(device=0)
    routes = set()
    for kmax in (dl.KMAX, 4):
        monkeypatch.setattr(dl, "KMAX", kmax)
        out = eng.fedavg_routed(ups, ns, downlink="mxfp8")
        routes.add(eng.last_timing["downlink"])
        assert eng.last_timing["staging"] == ("mxfp8-host-rows" if kind == "e4m3" else "mxfp4-host-rows")
        assert wire.is_mxfp8(out) and [a.shape for a in out[:-1]] == shapes
        assert all(isinstance(a, wire.BucketArray) for a in out) and len({id(a._bucket) for a in out}) == 1
        got_c = np.concatenate([np.asarray(a)["e4m3fn"].reshape(-1) for a in out[:-1]])
        _check((got_c, np.asarray(out[-1])["e8m0"]), want, f"{kind} K={K} kmax={kmax}")
    assert routes == ({"mxfp8-two-step"} if K > 128 else {"mxfp8-fused", "mxfp8-two-step"})


@pytest.mark.parametrize("m", [1.0, 0.3])
@pytest.mark.parametrize("flat", [False, True])
def test_increment_fp32(dl, m, flat):
    """Tensors of 5, 1, 33, T + 7 and 16 elements: blocks span tensors.  Separately allocated, tensor
    k starts (3 k + c) % 4 elements past 16-B alignment, so over c = 0, 1 the lanes inside the two
    long tensors begin 0, 1, 2 and 3 elements before an aligned address; ``flat``: the same as views
    of one bucket."""
    numels = [5, 1, 33, TILE + 7, 16]
    M, c = sum(numels), int(m < 1)
    rng = np.random.default_rng(int(10 * m) + flat)
    codes, s = wire.float32_to_mxfp8((rng.standard_normal(M) * np.exp2(rng.integers(-6, 6, M))).astype(np.float32))
    w0 = rng.standard_normal(M).astype(np.float32)
    want = w0 + np.float32(m) * wire.mxfp8_to_float32(codes, s)
    cuts = np.cumsum([0] + numels)
    if flat:
        outs = [Guarded(M, 0, torch.float32, torch.from_numpy(w0))]
        ptrs = [outs[0].ptr + 4 * int(a) for a in cuts[:-1]]
    else:
        outs = [Guarded(n, (3 * k + c) % 4, torch.float32, torch.from_numpy(w0[a:a + n]))
                for k, (a, n) in enumerate(zip(cuts, numels))]
        ptrs = [o.ptr for o in outs]
    dev = torch.from_numpy(np.concatenate([codes["e4m3fn"], s["e8m0"]])).cuda()
    dl.increment(ptrs, numels, dev.data_ptr(), dev.data_ptr() + M, M, m, 0)
    torch.cuda.synchronize()
    assert np.array_equal(np.concatenate([o.get() for o in outs]).view(np.uint32), want.view(np.uint32))


def test_decode_exhaustive(dl):
    """All 256 codes under all 256 scale bytes, at both alignments of the output."""
    codes = np.tile(np.arange(256, dtype=np.uint8), 256)
    scales = np.repeat(np.arange(256, dtype=np.uint8), 8)
    M = codes.size
    want = wire.mxfp8_to_float32(codes.view(E4M3), scales.view(E8M0))
    dev = torch.from_numpy(np.concatenate([codes, scales])).cuda()
    for off in (0, 1):
        out = Guarded(M, off, torch.float32, torch.zeros(M))
        dl.decode(dev.data_ptr(), dev.data_ptr() + M, M, out.ptr, 0)
        torch.cuda.synchronize()
        got, ok = out.get().view(np.float32), ~np.isnan(want)
        assert np.array_equal(np.isnan(got), ~ok) and np.array_equal(got.view(np.uint32)[ok], want.view(np.uint32)[ok])


def test_increment_parameters_bf16_model(dl):
    """A bf16 model handed the MXFP8 update equals the same model handed the host-decoded fp32 layers."""
    from substrafl_amd.algorithms import weight_manager as wm

    torch.manual_seed(3)
    models = [torch.nn.Sequential(torch.nn.Linear(33, 40), torch.nn.Linear(40, 1)).to(torch.bfloat16).cuda() for _ in range(2)]
    models[1].load_state_dict(models[0].state_dict())
    shapes = [tuple(p.shape) for p in models[0].parameters()]
    rng = np.random.default_rng(4)
    c, s = wire.float32_to_mxfp8([rng.standard_normal(sh).astype(np.float32) for sh in shapes])
    wm.increment_parameters(models[0], list(c) + [s], with_batch_norm_parameters=False, updates_multiplier=0.3)
    wm.increment_parameters(models[1], wire.mxfp8_to_float32(list(c), s), with_batch_norm_parameters=False,
                            updates_multiplier=0.3)
    for p, q in zip(models[0].parameters(), models[1].parameters()):
        assert torch.equal(p.view(torch.int16), q.view(torch.int16))


@pytest.mark.parametrize("dtype, uplink, ef", [(torch.float32, "mxfp8", False), (torch.bfloat16, "mxfp8", False),
                                               (torch.float32, "mxfp4", True)])
def test_federation_end_to_end(dl, monkeypatch, dtype, uplink, ef):
    """3 clients, 2 rounds, twice from the same seed: ``FedAvg(downlink="mxfp8")`` against the same
    federation without it whose clients are handed the host-decoded host-encoded fp32 average
    through the existing path.  The final weights are the same bits."""
    from standin_substrafl.algorithms.pytorch import TorchFedAvgAlgo
    from standin_substrafl.index_generator import NpIndexGenerator

    from substrafl_amd.algorithms.weight_manager import model_parameters
    from substrafl_amd.integration import accelerate_algo
    from substrafl_amd.schemas import FedAvgAveragedState
    from substrafl_amd.strategies import FedAvg

    class XY(torch.utils.data.Dataset):
        def __init__(self, data_from_opener, is_inference=False):
            self.x, self.y = data_from_opener

        def __getitem__(self, i):
            return torch.from_numpy(self.x[i]).to(dtype), torch.from_numpy(self.y[i]).to(dtype)

        __len__ = lambda self: len(self.x)  # noqa: E731

    def algo(client):
        torch.manual_seed(7)
        model = torch.nn.Sequential(torch.nn.Linear(6, 24), torch.nn.BatchNorm1d(24), torch.nn.ReLU(),
                                    torch.nn.Linear(24, 1)).to(dtype)

        class MyAlgo(TorchFedAvgAlgo):
            def __init__(self):
                super().__init__(model=model, criterion=torch.nn.MSELoss(),
                                 optimizer=torch.optim.SGD(model.parameters(), lr=0.02),
                                 index_generator=NpIndexGenerator(batch_size=32, num_updates=3, seed=11 + client),
                                 dataset=XY, with_batch_norm_parameters=True, disable_gpu=False)

        return accelerate_algo(MyAlgo, wire=uplink, error_feedback=ef)()

    def federation(downlink):
        rng = np.random.default_rng(1)
        xs = [rng.standard_normal((n, 6)).astype(np.float32) for n in (120, 77, 50)]
        data = [(x, (x @ rng.standard_normal((6, 1))).astype(np.float32)) for x in xs]
        algos = [algo(k) for k in range(3)]
        strategy = FedAvg(algo=type("A", (), {"strategies": ["Federated Averaging"]})(), device=0, downlink=downlink)
        avg = None
        for _ in range(2):
            states = [a.train(data_from_opener=d, shared_state=avg, _skip=True) for a, d in zip(algos, data)]
            avg = strategy.avg_shared_states(shared_states=states, _skip=True)
            if downlink is None:
                c, s = wire.float32_to_mxfp8([np.asarray(a) for a in avg.avg_parameters_update])
                avg = FedAvgAveragedState(avg_parameters_update=wire.mxfp8_to_float32(list(c), s))
            else:
                assert wire.is_mxfp8(list(avg.avg_parameters_update))
        # one more train applies the last average; the weights before its local steps are what counts
        for a, d in zip(algos, data):
            a.train(data_from_opener=d, shared_state=avg, _skip=True)
        return [[p.data.detach().cpu().view(torch.int16 if dtype == torch.bfloat16 else torch.int32).numpy()
                 for p in model_parameters(a.model, True)()] for a in algos]

    monkeypatch.setattr(torch.backends.cudnn, "enabled", False)  # the native BatchNorm kernels: deterministic training
    for g, w in zip(federation("mxfp8"), federation(None)):
        assert all(np.array_equal(a, b) for a, b in zip(g, w))
