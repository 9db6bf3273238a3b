"""``wire.BF16``: the host dtype of bfloat16 layers (a 2-byte structured dtype holding the bit
pattern).  It pickles with plain NumPy and through the flat wire format, NumPy refuses arithmetic on
it, and the conversion helpers agree with ``torch.bfloat16``.  CPU only."""

import pickle

import numpy as np
import pytest
import torch

from substrafl_amd import wire
from substrafl_amd.remote.mapped_pickle import BIG, load_mapped
from substrafl_amd.schemas import FedAvgSharedState

PROTOCOLS = [2, 4, 5]


def _bits(n, seed=0):
    return np.random.default_rng(seed).integers(0, 1 << 16, n, dtype=np.uint16).view(wire.BF16)


def _u16(a):
    return np.asarray(a).view(np.ndarray).view(np.uint16)


def test_dtype_is_two_bytes_and_tagged():
    assert wire.BF16.itemsize == 2 and wire.BF16.names == ("bfloat16",)
    assert wire.is_bf16(_bits(3)) and wire.is_bf16(wire.BF16) and not wire.is_bf16(np.zeros(3, np.uint16))
    assert wire.BF16 != np.dtype(np.uint16) and wire.BF16 != np.dtype(np.float16)


@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_plain_array_round_trips(protocol):
    a = _bits(1000).reshape(10, 100)
    b = pickle.loads(pickle.dumps(a, protocol=protocol))
    assert type(b) is np.ndarray and b.dtype == wire.BF16 and b.dtype.itemsize == 2 and b.shape == a.shape
    assert np.array_equal(_u16(a), _u16(b))


@pytest.mark.parametrize("protocol", PROTOCOLS)
@pytest.mark.parametrize("maker", ["bucket_views", "pack"])
def test_bucket_layers_round_trip(protocol, maker):
    shapes = [(3, 5), (1,), (), (257,), (4099,)]
    flat = _bits(sum(int(np.prod(s)) for s in shapes), 1)
    if maker == "bucket_views":
        layers = wire.bucket_views(flat, shapes)
    else:
        offs = np.cumsum([0] + [int(np.prod(s)) for s in shapes])
        layers = wire.pack([flat[o : o + int(np.prod(s))].reshape(s) for o, s in zip(offs, shapes)])
    assert all(a.dtype == wire.BF16 and a.shape == s for a, s in zip(layers, shapes))
    spanning = wire.flat_of(layers)
    assert spanning is not None and spanning.dtype == wire.BF16 and np.array_equal(_u16(spanning), _u16(flat))
    blob = pickle.dumps(layers, protocol=protocol)
    assert blob.count(b"_bucket_from_buffer") == 1 and b"_reconstruct" not in blob  # one buffer, no per-layer arrays
    if protocol >= 4:  # (protocol 2 writes bytes through a latin-1 text encoding, up to twice the size)
        assert len(blob) < flat.nbytes + 2000
    back = pickle.loads(blob)
    assert all(isinstance(a, wire.BucketArray) and a.dtype == wire.BF16 and a.dtype.itemsize == 2 and a.shape == s
               for a, s in zip(back, shapes))
    f = wire.flat_of(back)
    assert f is not None and f.dtype == wire.BF16 and np.array_equal(_u16(f), _u16(flat))
    # existing dtypes pickle to what they did: the record still carries dtype.str
    f32 = wire.bucket_views(np.arange(6, dtype=np.float32), [(2, 3)])[0]
    assert f32.__reduce_ex__(protocol)[1][3] == "<f4"


@pytest.mark.parametrize("protocol", PROTOCOLS)
@pytest.mark.parametrize("form", ["plain", "bucket"])
def test_mapped_loader(tmp_path, protocol, form):
    n_big = BIG // 2 + 1001  # > 1 MiB of payload: handed out as a view of the mapping
    flat = _bits(n_big + 15, 2)
    shapes = [(n_big,), (3, 5)]
    if form == "plain":
        layers = [flat[:n_big].copy(), flat[n_big:].reshape(3, 5).copy()]
    else:
        layers = wire.bucket_views(flat, shapes)
    st = FedAvgSharedState(n_samples=5, parameters_update=layers)
    p = tmp_path / "state"
    p.write_bytes(pickle.dumps(st, protocol=protocol))
    ref = pickle.loads(p.read_bytes())
    got = load_mapped(p)
    assert type(got) is type(ref) and got.n_samples == 5
    for g, r, s in zip(got.parameters_update, ref.parameters_update, shapes):
        assert type(g) is type(r) and g.dtype == wire.BF16 and g.shape == s
        assert np.array_equal(_u16(g), _u16(r))
    assert (wire.flat_of(list(got.parameters_update)) is not None) == (form == "bucket")


def test_arithmetic_raises():
    a = _bits(8)
    for op in (lambda: a * 0.5, lambda: a + a, lambda: np.sum([a, a], axis=0), lambda: np.result_type(wire.BF16, 1.0)):
        with pytest.raises(TypeError):  # UFuncTypeError and DTypePromotionError are TypeErrors
            op()
    layer = wire.bucket_views(a, [(8,)])[0]
    with pytest.raises(TypeError):
        layer * 0.5


def _torch_bf16_bits(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def _check_against_torch(x):
    got = wire.float32_to_bf16(x)
    assert got.dtype == wire.BF16 and got.shape == x.shape
    ref = _torch_bf16_bits(x)
    nan = np.isnan(x)
    assert np.array_equal(_u16(got)[~nan], ref[~nan])
    up = wire.bf16_to_float32(got)
    assert up.dtype == np.float32 and up.shape == x.shape
    assert np.isnan(up[nan]).all()  # NaN stays NaN
    ref_up = torch.from_numpy(ref.view(np.int16)).view(torch.bfloat16).float().numpy()
    assert np.array_equal(up.view(np.uint32)[~nan], ref_up.view(np.uint32)[~nan])  # the upcast is exact


def test_conversion_edge_table():
    bits = np.array([
        0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x3F818001,  # ties at the bf16 boundary: to even
        0xBF808000, 0xBF818000,
        0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,  # max finite fp32 -> inf; the last bf16 tie; just below
        0x00000001, 0x007FFFFF, 0x00008000, 0x00018000, 0x80000001, 0x807FFFFF,  # fp32 subnormals
        0x00000000, 0x80000000, 0x7F800000, 0xFF800000,  # +-0, +-inf
        0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0x7F80FFFF,  # NaNs (quiet, signalling, low payload)
    ], dtype=np.uint32)
    x = bits.view(np.float32)
    _check_against_torch(x)
    got = _u16(wire.float32_to_bf16(x))
    assert got[0] == 0x3F80 and got[1] == 0x3F82  # 1.00390625 ties down to even, 1.01171875 up to even
    assert got[7] == 0x7F80 and got[8] == 0xFF80  # overflow to +-inf
    assert np.isnan(wire.bf16_to_float32(wire.float32_to_bf16(x[21:]))).all()
    assert wire.float32_to_bf16(np.float32(1.5)).shape == ()  # 0-d in, 0-d out


def test_conversion_random_bit_patterns():
    bits = np.random.default_rng(3).integers(0, 1 << 32, 100_000, dtype=np.uint64).astype(np.uint32)
    _check_against_torch(bits.view(np.float32))


def test_non_accelerated_average_fails_loudly():
    """What a peer without this package's aggregator does (fed_avg.py:217-222) raises on
    ``wire.BF16`` layers instead of averaging bit patterns."""
    layers = [wire.float32_to_bf16(np.ones((2, 3), np.float32)) for _ in range(2)]
    with pytest.raises(TypeError):
        np.sum([a * 0.5 for a in layers], axis=0)
