"""The MXFP8 wire format on the host (``substrafl_amd/wire.py``): OCP ``e4m3fn`` codes with one
``e8m0`` scale byte per block of 32 elements.  Decode and the element rounding are held to torch's
CPU ``float8_e4m3fn``; the scale rule to hand-made blocks worked out from the rule's text; the two
dtypes pickle as one buffer and refuse NumPy arithmetic.  No GPU."""

import pickle

import numpy as np
import pytest
import torch

from mxfp8_cases import all_values, hand_blocks
from substrafl_amd import wire
from substrafl_amd.wire import E4M3, E8M0


def _codes(b) -> np.ndarray:
    return np.asarray(b, np.uint8).view(E4M3)


def _scales(b) -> np.ndarray:
    return np.asarray(b, np.uint8).view(E8M0)


def test_decode_of_all_codes_is_torchs():
    c = np.arange(256, dtype=np.uint8)
    got = wire.mxfp8_to_float32(_codes(c), _scales([127] * 8))
    ref = torch.from_numpy(c.copy()).view(torch.float8_e4m3fn).to(torch.float32).numpy()
    assert got.dtype == np.float32 and got.shape == (256,)
    nan = np.isnan(ref)
    assert list(np.flatnonzero(nan)) == [0x7F, 0xFF] and np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], ref.view(np.uint32)[~nan])  # signed zeros included
    assert not np.isinf(got).any()  # e4m3fn has no infinity


def test_decode_scales_exactly_down_to_subnormals_and_up_to_inf():
    c = np.arange(256, dtype=np.uint8)
    base = wire.mxfp8_to_float32(_codes(c), _scales([127] * 8)).astype(np.float64)
    for s in (0, 1, 7, 126, 128, 245, 254):
        got = wire.mxfp8_to_float32(_codes(c), _scales([s] * 8))
        with np.errstate(over="ignore", invalid="ignore"):
            ref = (base * 2.0 ** (s - 127)).astype(np.float32)  # exact in fp64, one rounding (overflow) to fp32
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got), nan), s
        assert np.array_equal(got.view(np.uint32)[~nan], ref.view(np.uint32)[~nan]), s
        finite = np.isfinite(ref)
        assert np.array_equal(got[finite].astype(np.float64), (base * 2.0 ** (s - 127))[finite]), s  # nothing flushed
    assert wire.mxfp8_to_float32(_codes([0x01]), _scales([0]))[0] == np.float32(2.0 ** -136)
    assert np.isposinf(wire.mxfp8_to_float32(_codes([0x7E]), _scales([254]))[0])  # 448 * 2^127
    assert np.isnan(wire.mxfp8_to_float32(_codes([0x00, 0x38, 0x80]), _scales([255]))).all()  # s == 255: NaN block


def test_element_rounding_is_torchs_cast_ties_included():
    vals = all_values()  # the 127 non-negative finite e4m3fn values, ascending
    mids = (vals[:-1] + vals[1:]) / 2  # every midpoint between adjacent codes: exact in fp32
    rng = np.random.default_rng(5)
    y = np.concatenate([
        vals, mids, np.nextafter(mids.astype(np.float32), np.float32(0)), np.nextafter(mids.astype(np.float32), np.float32(1e9)),
        [464.0, np.nextafter(np.float32(464), np.float32(0)), 448.0, 2.0 ** -10, 2.0 ** -11, 1e-30, 1e-45],
        rng.uniform(0, 464, 150000), rng.uniform(0, 2.0 ** -5, 50000), np.exp(rng.uniform(-20, 6.13, 100000)),
    ]).astype(np.float32)
    y = y[np.abs(y) <= 464]
    y = np.concatenate([y, -y])
    assert y.size > 3e5
    got = wire._e4m3_round(y)
    ref = torch.from_numpy(y).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(got, ref)
    assert (got & 0x7F).max() == 0x7E  # 464 is the tie that still rounds to 448: nothing becomes NaN


@pytest.mark.parametrize("name", sorted(hand_blocks()))
def test_scale_rule_on_hand_made_blocks(name):
    x, want_scale, want = hand_blocks()[name]
    codes, scales = wire.float32_to_mxfp8(x)
    assert codes.dtype == E4M3 and scales.dtype == E8M0 and codes.shape == x.shape
    assert scales.shape == (-(-x.size // 32),)
    assert list(scales["e8m0"]) == want_scale, name
    for pos, code in want.items():
        assert codes["e4m3fn"][pos] == code, (name, pos, hex(codes["e4m3fn"][pos]), hex(code))


def test_scale_bump_at_464():
    """amax == 464 * 2^e stays (it rounds to 448), the next float above moves to the next scale."""
    for e in (-20, 0, 9):
        a = np.float32(464.0 * 2.0 ** e)
        for amax, s, code in ((a, e + 127, 0x7E), (np.nextafter(a, np.float32(np.inf)), e + 128, 0x77)):
            x = np.zeros(32, np.float32)
            x[3] = -amax
            codes, scales = wire.float32_to_mxfp8(x)
            assert scales["e8m0"][0] == s and codes["e4m3fn"][3] == (0x80 | code), (e, float(amax))
    # 0x77 = 1.875 * 2^7 = 240 = round(232.0000x): the block maximum never saturates


def test_encode_of_decode_is_the_identity():
    rng = np.random.default_rng(11)
    M = 32 * 4000 + 19
    c = rng.integers(0, 256, M).astype(np.uint8)
    c[(c & 0x7F) == 0x7F] = 0x3C  # NaN codes have no canonical encoding
    # scales away from the clamp of e at the bottom (the hand-made blocks cover it) and from
    # overflow at the top (448 * 2^(247-127) is still finite)
    s = rng.integers(10, 247, -(-M // 32)).astype(np.uint8)
    # canonical blocks only: the block maximum must be one the scale rule gives this scale, i.e.
    # an element in [256, 448] * 2^e (exponent field 15): plant 0x78
    c[::32] = 0x78 | (c[::32] & 0x80)
    x = wire.mxfp8_to_float32(_codes(c), _scales(s))
    assert np.isfinite(x).all()
    c2, s2 = wire.float32_to_mxfp8(x)
    assert np.array_equal(s2["e8m0"], s) and np.array_equal(c2["e4m3fn"], c)
    # and decode(encode(.)) of those values is exact
    assert np.array_equal(wire.mxfp8_to_float32(c2, s2).view(np.uint32), x.view(np.uint32))


def test_error_bound():
    """An element's error is at most 2^-4 relative where it is an e4m3fn normal under the block's
    scale, and at most 2^-10 * 2^e (half the subnormal granule) otherwise: 6.25 % of 256 * 2^e <=
    the block maximum at worst for the relative part."""
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(32 * 3000) * np.exp(rng.uniform(-30, 30, 32 * 3000))).astype(np.float32)
    codes, scales = wire.float32_to_mxfp8(x)
    dec = wire.mxfp8_to_float32(codes, scales).astype(np.float64)
    e = np.repeat(scales["e8m0"].astype(np.int64) - 127, 32)
    err = np.abs(dec - x.astype(np.float64))
    bound = np.maximum(np.abs(x.astype(np.float64)) * 2.0 ** -4, 2.0 ** (e - 10.0))
    assert (err <= bound).all()
    amax = np.repeat(np.abs(x).reshape(-1, 32).max(axis=1).astype(np.float64), 32)
    assert (err <= 0.0625 * amax).all()


def test_layers_share_blocks_across_their_boundaries():
    rng = np.random.default_rng(2)
    layers = [rng.standard_normal((5, 3)).astype(np.float32), np.float32([1e-3]), rng.standard_normal(50).astype(np.float32)]
    codes, scales = wire.float32_to_mxfp8(layers)
    flat_codes, flat_scales = wire.float32_to_mxfp8(np.concatenate([a.reshape(-1) for a in layers]))
    assert [c.shape for c in codes] == [(5, 3), (1,), (50,)] and scales.shape == (3,)
    assert np.array_equal(np.concatenate([c.reshape(-1) for c in codes]), flat_codes)
    assert np.array_equal(scales, flat_scales)
    dec = wire.mxfp8_to_float32(codes, scales)
    assert [d.shape for d in dec] == [(5, 3), (1,), (50,)]
    assert np.array_equal(np.concatenate([d.reshape(-1) for d in dec]), wire.mxfp8_to_float32(flat_codes, flat_scales))
    pu = list(codes) + [scales]
    assert wire.is_mxfp8(pu) and wire.has_mxfp8(pu) and wire.mxfp8_check(pu) == 66
    assert not wire.is_mxfp8(layers) and not wire.has_mxfp8(layers)
    assert not wire.is_mxfp8(list(codes)) and wire.has_mxfp8(list(codes))
    for bad in (list(codes), list(codes) + [scales[:2]], list(codes) + [scales["e8m0"]], [scales],
                list(codes) + [np.zeros((3, 1), E8M0)]):
        with pytest.raises(ValueError):
            wire.mxfp8_check(bad)


@pytest.mark.parametrize("protocol", [2, 3, 4, 5])
def test_pickle_round_trip_as_one_buffer(protocol):
    rng = np.random.default_rng(7)
    layers = [rng.standard_normal(s).astype(np.float32) for s in [(64, 33), (33,), (1,), (5, 1)]]
    codes, scales = wire.float32_to_mxfp8(layers)
    M = sum(a.size for a in layers)
    pu = wire.pack(list(codes) + [scales])
    assert wire.is_mxfp8(pu)
    buffers = []
    blob = pickle.dumps(pu, protocol=protocol, buffer_callback=buffers.append if protocol == 5 else None)
    back = pickle.loads(blob, buffers=buffers) if protocol == 5 else pickle.loads(blob)
    assert protocol != 5 or len(buffers) == 1  # out of band: one buffer for the whole update
    assert len(blob) < (M + scales.size + 2000 if protocol != 5 else 2000)
    assert wire.is_mxfp8(back) and wire.mxfp8_check(back) == M
    assert all(isinstance(a, wire.BucketArray) for a in back) and len({id(a._bucket) for a in back}) == 1
    for a, b in zip(pu, back):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    flat = wire.flat_of(back[:-1])  # the aggregator stages a client's codes as one segment
    assert flat is not None and flat.dtype == E4M3 and flat.size == M


@pytest.mark.parametrize("dt", [E4M3, E8M0])
def test_numpy_arithmetic_raises(dt):
    a = np.zeros(4, np.uint8).view(dt)
    assert a.dtype.itemsize == 1
    for op in (lambda: a * 0.5, lambda: a + a, lambda: np.sum(a), lambda: np.result_type(dt, 1.0),
               lambda: np.sum([a, a], axis=0)):
        with pytest.raises(TypeError):
            op()
    with pytest.raises(TypeError):
        wire.mxfp8_to_float32(np.zeros(4, np.uint8), np.zeros(1, np.uint8))
