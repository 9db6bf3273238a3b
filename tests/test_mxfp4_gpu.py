"""libfedagg_mx4.so on the GPU, bit for bit (NaN by position) against wire.py and a plain NumPy
FedAvg on the decoded inputs: both decoders over every byte under every scale, the FedAvg kernel
at every size at which it changes path (taken from fedagg_mx4_blocking), numel == 1 layers, the
quantiser with and without error feedback, and one round end to end."""

from __future__ import annotations

import ctypes
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch  # before the native libraries: one HIP runtime in the process

from oracle import fedavg_reference_structure
from substrafl_amd import _native, _native_mx4, wire
from substrafl_amd.engine import fedavg_weights

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
TILE, GROUP = _native_mx4.blocking()  # the sizes at which the kernel changes path (no HIP call)


def dev(a: np.ndarray, pad: int = 0) -> torch.Tensor:
    """``a``'s bytes in a fresh device buffer (torch allocations are 256-B aligned), ``pad`` spare bytes behind."""
    t = torch.zeros(a.nbytes + pad, dtype=torch.uint8, device="cuda")
    t[: a.nbytes] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8))
    return t


def fedavg(codes, scales, w, M, idx=(), off=0):
    """The library over the [K, ceil(M/2)] codes and [K, ceil(M/32)] scales; the result's bits.
    ``off``: the byte offset of d_out from a 16-B boundary."""
    K = codes.shape[0]
    dc = [dev(codes[k]) for k in range(K)]
    ds = [dev(scales[k]) for k in range(K)]
    out = torch.full((M + 8,), float("nan"), dtype=torch.float32, device="cuda")
    _native_mx4.fedavg_e2m1([t.data_ptr() for t in dc], [t.data_ptr() for t in ds], w, M, list(idx),
                            out.data_ptr() + off, int(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert (got[off // 4 + M:] == 0x7FC00000).all() and (got[: off // 4] == 0x7FC00000).all()  # nothing past the row
    return got[off // 4: off // 4 + M]


def same(got_bits, ref, what=""):
    ref = np.ascontiguousarray(ref, np.float32)
    nan = np.isnan(ref)
    assert np.array_equal((got_bits & 0x7FFFFFFF) > 0x7F800000, nan), f"{what}: NaN positions differ"
    bad = np.flatnonzero((got_bits != ref.view(np.uint32)) & ~nan)
    assert bad.size == 0, (what, bad.size, bad[:8], [hex(v) for v in got_bits[bad[:8]]],
                           [hex(v) for v in ref.view(np.uint32)[bad[:8]]])


def reference(x, w, idx=()):
    """fp32 FedAvg in list order from +0.0 over the decoded rows x [K, M]; NumPy's own np.sum of
    the products at the numel == 1 indices."""
    with np.errstate(all="ignore"):
        acc = np.zeros(x.shape[1], np.float32)
        for k in range(x.shape[0]):
            acc = acc + x[k] * np.float32(w[k])
        for i in idx:
            acc[i] = np.float32(0.0) + np.sum(x[:, i] * np.asarray(w, np.float32))
    return acc


@pytest.mark.parametrize("off", [0, 4], ids=["vector-walk", "plain-walk"])
def test_exhaustive_decode(off):
    """Every byte value under every scale byte, K = 1, w = 1: M = 256 * 16 * 32."""
    byte = np.tile(np.repeat(np.arange(256, dtype=np.uint8), 16), 256)  # block b: 16 copies of byte b % 256
    scales = np.repeat(np.arange(256, dtype=np.uint8), 256)             # block b: scale b // 256
    M = byte.size * 2
    x = wire.mxfp4_to_float32(byte.view(wire.E2M1X2), scales.view(wire.E8M0), M)
    same(fedavg(byte[None], scales[None], [1.0], M, off=off), reference(x[None], [1.0]), f"offset {off}")


def random_rows(rng, K, M):
    codes = rng.integers(0, 256, (K, -(-M // 2)), dtype=np.uint8)
    scales = rng.integers(117, 131, (K, -(-M // 32)), dtype=np.uint8)
    scales[rng.random(scales.shape) < 0.02] = rng.choice(np.array([0, 1, 253, 254, 255], np.uint8))  # the rare-scale path
    x = np.stack([wire.mxfp4_to_float32(codes[k].view(wire.E2M1X2), scales[k].view(wire.E8M0), M) for k in range(K)])
    ns = rng.integers(100, 10000, K)
    return codes, scales, x, fedavg_weights([int(n) for n in ns], "f32")


@pytest.mark.parametrize("K", [1, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP + 1, 129])
@pytest.mark.parametrize("M", [1, 31, 33, TILE - 1, TILE + 1, 2 * TILE + 47])
def test_fedavg(K, M):
    codes, scales, x, w = random_rows(np.random.default_rng(K * 100003 + M), K, M)
    same(fedavg(codes, scales, w, M), reference(x, w), f"K={K} M={M}")


@pytest.mark.parametrize("K", [3, 129, 256])
def test_numel_one_layers(K):
    M = TILE + 47
    codes, scales, x, w = random_rows(np.random.default_rng(K), K, M)
    idx = [0, M // 2, M - 1]
    same(fedavg(codes, scales, w, M, idx), reference(x, w, idx), f"K={K}")


def edge_input(M, seed):
    """Normal data of mixed magnitudes with the edge blocks of the CPU test laid over its start."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(M) * np.exp(rng.uniform(-6, 6, M))).astype(np.float32)
    ties = np.array([6, .25, .75, 1.25, 1.75, 2.5, 3.5, 5, -.25, -.75, -1.25, -1.75, -2.5, -3.5, -5, 5.5, -6], np.float32)
    edges = [ties, np.nextafter(ties, np.float32(9)), np.nextafter(ties, np.float32(-9)), ties * np.float32(2.0 ** -60),
             np.array([np.nextafter(np.float32(7), np.float32(0))]), np.array([7.0]), np.array([1.0, np.inf]),
             np.array([np.nan, 2.0]), np.array([0.0, -0.0, 0.0]), np.array([2.0 ** -149, -2.0 ** -149, 2.0 ** -140]),
             np.array([3.4e38, -1e38, 1.0]), np.array([2.0 ** -126, 2.0 ** -127])]
    for b, e in enumerate(edges):
        if 32 * b + 32 <= M:
            x[32 * b: 32 * b + 32] = 0
            x[32 * b: 32 * b + e.size] = e
    return x


@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off-by-one"])
@pytest.mark.parametrize("M", [1, 7, 8, 31, 32, 33, 8 * TILE + 5])
def test_quantize(kind, off, M):
    """Codes and scales against wire.float32_to_mxfp4; with a residual also res', over two calls."""
    x = edge_input(M, M + off)
    if kind == "bf16":
        x = wire.bf16_to_float32(wire.float32_to_bf16(x))
        src, k, esz = dev(wire.float32_to_bf16(np.concatenate([np.zeros(off, np.float32), x]))), _native.FEDAGG_BF16, 2
    else:
        src, k, esz = dev(np.concatenate([np.zeros(off, np.float32), x])), _native.FEDAGG_F32, 4
    nc, nb = -(-M // 2), -(-M // 32)
    stream = int(torch.cuda.current_stream().cuda_stream)
    for ef in (False, True):
        res = np.zeros(M, np.float32)
        d_res = torch.zeros(M + off + 4, dtype=torch.float32, device="cuda")
        for call in range(2 if ef else 1):
            d_out = torch.full((nc + nb + 8,), 0xEE, dtype=torch.uint8, device="cuda")
            _native_mx4.quantize(src.data_ptr() + off * esz, k, M, d_res.data_ptr() + 4 * off if ef else None,
                                 d_out.data_ptr(), d_out.data_ptr() + nc, stream)
            torch.cuda.synchronize()
            got = d_out.cpu().numpy()
            if ef:
                c_ref, s_ref, res = wire.mxfp4_error_feedback(x, res)
                same(d_res.cpu().numpy()[off: off + M].view(np.uint32), res, f"res' call {call}")
                assert not d_res[off + M:].any() and not d_res[:off].any()
            else:
                c_ref, s_ref, _ = wire.float32_to_mxfp4(x)
            assert np.array_equal(got[:nc], c_ref["e2m1x2"]), (ef, call, np.flatnonzero(got[:nc] != c_ref["e2m1x2"])[:8])
            assert np.array_equal(got[nc: nc + nb], s_ref["e8m0"]), (ef, call)
            assert (got[nc + nb:] == 0xEE).all()  # nothing past the scale row


def test_one_round_end_to_end():
    """Two ``accelerate_algo(TorchFedAvgAlgo, wire="mxfp4", error_feedback=True)`` clients export, the
    strategy aggregates: the oracle on the decoded exports.  The library is loaded here, and a plain
    fp32 federation in a fresh process never loads it."""
    import standin_substrafl.strategies as ss
    from standin_substrafl.algorithms.pytorch import TorchFedAvgAlgo
    from standin_substrafl.index_generator import NpIndexGenerator

    from substrafl_amd.integration import accelerate, accelerate_algo

    def algo(dtype, client):
        torch.manual_seed(7)
        model = torch.nn.Sequential(torch.nn.Linear(6, 24), torch.nn.ReLU(), torch.nn.Linear(24, 1)).to(dtype)

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
                                 dataset=XY, disable_gpu=False)

        return accelerate_algo(MyAlgo, wire="mxfp4", error_feedback=True)()

    rng = np.random.default_rng(3)
    datasets = [(rng.standard_normal((n, 6)).astype(np.float32), rng.standard_normal((n, 1)).astype(np.float32))
                for n in (120, 77)]
    algos = [algo(torch.float32, 0), algo(torch.bfloat16, 1)]
    states = [a.train(data_from_opener=d, shared_state=None, _skip=True) for a, d in zip(algos, datasets)]
    M = 6 * 24 + 24 + 24 + 1
    for st, a in zip(states, algos):
        pu = list(st.parameters_update)
        assert wire.is_mxfp4(pu) and wire.mxfp4_check(pu) == M and len({id(p._bucket) for p in pu}) == 1
        assert wire.mxfp4_layer_shapes(pu[2]) == [(24, 6), (24,), (1, 24), (1,)]
        assert a._fedagg_mx_residual.dtype == torch.float32 and bool(a._fedagg_mx_residual.any())
    avg = accelerate(ss.FedAvg)(algo=algos[0]).avg_shared_states(shared_states=states, _skip=True)
    decoded = [wire.mxfp4_to_float32(*st.parameters_update) for st in states]
    ref = fedavg_reference_structure(decoded, [st.n_samples for st in states])
    assert len(avg.avg_parameters_update) == len(ref) == 4
    for g, r in zip(avg.avg_parameters_update, ref):
        assert g.dtype == np.float32 and g.shape == r.shape
        assert np.array_equal(np.asarray(g).view(np.uint32), r.view(np.uint32))
    assert any(np.any(np.asarray(g) != 0) for g in avg.avg_parameters_update) and _native_mx4.loaded()

    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import numpy as np, torch\n"
            "from substrafl_amd import _native_mx4\n"
            "from substrafl_amd.schemas import FedAvgSharedState\n"
            "from substrafl_amd.strategies import FedAvg\n"
            "class A: strategies = ['Federated Averaging']\n"
            "s = [FedAvgSharedState(n_samples=n, parameters_update=[np.ones((3, 2), np.float32)]) for n in (1, 2)]\n"
            "out = FedAvg(algo=A(), device=0).avg_shared_states(shared_states=s, _skip=True)\n"
            "assert np.asarray(out.avg_parameters_update[0]).shape == (3, 2)\n"
            "assert not _native_mx4.loaded() and 'libfedagg_mx4' not in open('/proc/self/maps').read()\n"
            % (str(ROOT), str(ROOT / "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
