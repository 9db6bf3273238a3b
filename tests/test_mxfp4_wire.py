"""The MXFP4 wire without a GPU: the NumPy codec of wire.py against the rules of
include/fedagg_mx4.h, error feedback in NumPy, every refusal that precedes the library load or any
device work, and the argument refusals of the built library (they precede its first HIP call)."""

import ctypes

import numpy as np
import pytest

from substrafl_amd import _native, _native_mx4, wire

VALUES = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6], np.float64)
F32, BF16, F16, F64 = _native.FEDAGG_F32, _native.FEDAGG_BF16, _native.FEDAGG_F16, _native.FEDAGG_F64


def block(first, fill=0.0):
    """One 32-element fp32 block: ``first`` values, then ``fill``."""
    x = np.full(32, fill, np.float32)
    x[: len(first)] = first
    return x


def nibbles(codes, M):
    c = codes["e2m1x2"]
    return np.stack([c & 15, c >> 4], axis=1).reshape(-1)[:M]


@pytest.mark.parametrize("s", [0, 1, 126, 127, 128, 253, 254, 255])
def test_decode_is_the_table(s):
    packed = (np.arange(16, dtype=np.uint8) | (np.arange(16, dtype=np.uint8)[::-1] << 4)).view(wire.E2M1X2)
    got = wire.mxfp4_to_float32(packed, np.array([s], np.uint8).view(wire.E8M0), 32)
    code = np.stack([np.arange(16), np.arange(16)[::-1]], axis=1).reshape(-1)
    with np.errstate(over="ignore"):
        want = (np.where(code & 8, -1.0, 1.0) * VALUES[code & 7] * 2.0 ** (s - 127)).astype(np.float32)
    if s == 255:
        assert np.isnan(got).all()
    else:
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))  # -0.0 and +-inf (s >= 253) included
        assert np.isinf(got).sum() == {253: 8, 254: 16}.get(s, 0)


@pytest.mark.parametrize("e", [-127, -126, -60, 0, 1, 60, 125])
def test_representable_values_round_trip(e):
    """Every e2m1 value times 2^e, both signs, with 6 * 2^e in the block so that its scale is e."""
    x = block(np.concatenate([VALUES[::-1], -VALUES]) * 2.0 ** e)
    codes, scales, shapes = wire.float32_to_mxfp4(x)
    assert scales["e8m0"][0] == e + 127 and shapes.tolist() == [1, 1, 32]
    assert np.array_equal(wire.mxfp4_to_float32(codes, scales, shapes)[0].view(np.uint32), x.view(np.uint32))


@pytest.mark.parametrize("amax,s", [(np.nextafter(np.float32(7), np.float32(0)), 127), (7.0, 128), (7.5, 128),
                                    (np.nextafter(np.float32(8), np.float32(0)), 128), (4.0, 127), (8.0, 128)])
def test_the_bump_at_seven(amax, s):
    codes, scales, _ = wire.float32_to_mxfp4(block([amax]))
    assert scales["e8m0"][0] == s
    assert nibbles(codes, 1)[0] == {127: 7 if amax > 5 else 6, 128: 6}[s]  # 6 under e, or 4 * 2 after the bump


def test_ties_go_to_even_and_six_clamps():
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    up = [float(np.nextafter(np.float32(t), np.float32(9))) for t in ties]
    down = [float(np.nextafter(np.float32(t), np.float32(0))) for t in ties]
    x = block([6.0] + ties + up + down + [-t for t in ties] + [5.5, 6.0, -6.0])  # 6.0 first: e = 0
    codes, scales, _ = wire.float32_to_mxfp4(x)
    assert scales["e8m0"][0] == 127
    n = nibbles(codes, 32)
    assert n[1:8].tolist() == [0, 2, 2, 4, 4, 6, 6]
    assert n[8:15].tolist() == [1, 2, 3, 4, 5, 6, 7] and n[15:22].tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert n[22:29].tolist() == [8, 10, 10, 12, 12, 14, 14] and n[29:32].tolist() == [7, 7, 15]


def test_special_blocks_and_the_clamps_of_e():
    tiny = np.float32(2.0 ** -149)
    x = np.concatenate([
        block([1.0, np.inf, -2.0]), block([np.nan], 3.0),     # Inf / NaN: s = 255, every code 0
        block([0.0, -0.0, 0.0, -0.0]),                        # zeros: s = 127, signs kept
        block([tiny, -tiny, 3 * tiny]),                       # subnormals: e clamped to -127
        block([np.float32(3.4e38), -1e38]),                   # the largest: e = 126, decodes to inf
        np.array([1.0, -0.0, 3.0], np.float32)])              # a partial block, odd M
    M = x.size
    codes, scales, _ = wire.float32_to_mxfp4(x)
    n, s = nibbles(codes, M), scales["e8m0"]
    assert codes.size == (M + 1) // 2 and codes["e2m1x2"][-1] >> 4 == 0  # the unused nibble is 0
    assert s.tolist() == [255, 255, 127, 0, 253, 126]
    assert not n[:64].any() and n[64:68].tolist() == [0, 8, 0, 8]
    d = wire.mxfp4_to_float32(codes, scales, M)
    assert np.isnan(d[:64]).all() and np.array_equal(d[64:96].view(np.uint32), x[64:96].view(np.uint32))
    assert d[96:99].view(np.uint32).tolist() == [0, 0x80000000, 0]  # the granule is 2^-128: all three round to zero
    assert d[128] == np.inf and d[129] == -np.float32(2.0 ** 126)
    assert d[160:].tolist() == [1.0, -0.0, 3.0] and np.signbit(d[161])


def test_error_feedback_in_numpy():
    rng = np.random.default_rng(4)
    x = (rng.standard_normal(32 * 9 + 5) * np.exp(rng.uniform(-4, 4, 32 * 9 + 5))).astype(np.float32)
    x[32:64] = 0
    x[70] = np.inf
    x[96] = 3.3e38
    res = np.zeros_like(x)
    for _ in range(2):  # the second step takes a non-zero residual in
        r = x + res
        codes, scales, res = wire.mxfp4_error_feedback(x, res)
        c2, s2, _ = wire.float32_to_mxfp4(r)
        assert np.array_equal(codes, c2) and np.array_equal(scales, s2)
        d = wire.mxfp4_to_float32(codes, scales, x.size)
        ok = np.isfinite(d)
        assert not ok[64:96].any() and not ok[96] and ok.sum() == x.size - 33
        assert np.array_equal(res[ok].astype(np.float64), r[ok].astype(np.float64) - d[ok])  # r - d is exact
        assert not res[~ok].any()


def update(shapes, seed):
    rng = np.random.default_rng(seed)
    return list(wire.float32_to_mxfp4([rng.standard_normal(s).astype(np.float32) for s in shapes]))


def test_routes_refuse_before_any_device_work(monkeypatch):
    from substrafl_amd import handoff, runtime
    from substrafl_amd.engine import AggregationEngine, reject_mxfp8
    from substrafl_amd.multi_device import MultiDeviceEngine

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(runtime, "session", no_device)
    monkeypatch.setattr(runtime, "device_lock", no_device)
    shapes = [(4, 5), (1,), (7,)]
    mx = [update(shapes, k) for k in range(3)]
    assert all(wire.is_mxfp4(u) and wire.mxfp4_check(u) == 28 and not wire.is_mxfp8(u) for u in mx)
    plain = [np.zeros(s, np.float32) for s in shapes]
    eng, ns = AggregationEngine(device=0), [1, 2, 3]
    for entry in (eng.fedavg_mxfp4, eng.fedavg_routed, eng.fedavg):
        with pytest.raises(NotImplementedError, match="2 of 3 clients sent MXFP4"):
            entry([mx[0], plain, mx[2]], ns)
        with pytest.raises(ValueError, match="shape tables differ"):
            entry([mx[0], update([(5, 4), (1,), (7,)], 9), mx[2]], ns)
        with pytest.raises(ValueError, match="need a 1-D scale array of 1 bytes"):
            entry([[m[0], np.zeros(2, wire.E8M0), m[2]] for m in mx], ns)
        with pytest.raises(ValueError, match="need a 1-D code array of 14 bytes"):
            entry([[np.zeros(15, wire.E2M1X2), m[1], m[2]] for m in mx], ns)
        with pytest.raises(ValueError, match="expected \\[codes"):
            entry([[m[0], m[1]["e8m0"], m[2]] for m in mx], ns)  # plain uint8 scales: the wrong dtype
        with pytest.raises(NotImplementedError, match="MXFP4 route serves numel == 1 layers up to 256 clients"):
            entry([mx[0]] * 257, [1] * 257)
    monkeypatch.setattr(handoff, "_enabled", True)
    with pytest.raises(NotImplementedError, match="hand-off has no MXFP4 route"):
        eng.fedavg_routed(mx, ns)
    monkeypatch.setattr(handoff, "_enabled", False)
    multi = MultiDeviceEngine.__new__(MultiDeviceEngine)
    with pytest.raises(NotImplementedError, match="MultiDeviceEngine.fedavg_routed.*no MXFP4 path"):
        multi.fedavg_routed(mx, ns)
    with pytest.raises(NotImplementedError, match="Scaffold engine: no MXFP4 path"):
        reject_mxfp8(mx, "Scaffold engine")


def test_client_option_and_export_refusals():
    import torch
    from standin_substrafl.algorithms.pytorch import TorchFedAvgAlgo, TorchScaffoldAlgo
    from standin_substrafl.algorithms.pytorch.torch_newton_raphson_algo import TorchNewtonRaphsonAlgo

    from substrafl_amd.algorithms import weight_manager as wm
    from substrafl_amd.integration import accelerate_algo

    for ef in (False, True):
        cls = accelerate_algo(TorchFedAvgAlgo, wire="mxfp4", error_feedback=ef)
        assert cls._fedagg_mxfp4 is True and cls._fedagg_mxfp8 is False
        assert getattr(cls, "_fedagg_error_feedback", False) is ef
    assert accelerate_algo(TorchFedAvgAlgo, wire="mxfp8")._fedagg_mxfp4 is False
    with pytest.raises(ValueError, match="wire must be True, False or 'mxfp8'.*mxfp4"):
        accelerate_algo(TorchFedAvgAlgo, wire="MXFP4")
    for cls in (TorchScaffoldAlgo, TorchNewtonRaphsonAlgo):
        with pytest.raises(TypeError, match="wire='mxfp4' is an option of TorchFedAvgAlgo"):
            accelerate_algo(cls, wire="mxfp4")
    with pytest.raises(TypeError, match="error_feedback is an option of wire='mxfp8'"):
        accelerate_algo(TorchFedAvgAlgo, wire=True, error_feedback=True)
    for dt in (torch.float32, torch.float16, torch.float64):  # CPU tensors, and no fp16 / fp64 quantiser
        with pytest.raises(NotImplementedError, match="wire='mxfp4'"):
            wm.export_mxfp4([torch.zeros(8, dtype=dt)])


def test_the_library_refuses_bad_arguments_before_any_hip_call():
    """Fake non-NULL pointers: a refused call has made no HIP call, so nothing is dereferenced."""
    lib = _native_mx4.load()
    A, B, C = 0x100000, 0x200000, 0x300000
    w, idx = (ctypes.c_float * 2)(), (ctypes.c_uint64 * 1)(64)

    def fedavg(codes, scales, K, out=C, h_w=w, P=0, h_idx=None):
        return lib.fedagg_mx4_fedavg_e2m1(_native.ptr_array(codes) if codes else None,
                                          _native.ptr_array(scales) if scales else None, h_w, K, 64, h_idx, P, out, None)

    q = lib.fedagg_mx4_quantize
    cases = [
        (lambda: fedavg([A], [B], 0), b"K must be positive (K=0)"),
        (lambda: fedavg([A], [B], -3), b"K must be positive (K=-3)"),
        (lambda: fedavg(None, [B], 1), b"d_codes is NULL"),
        (lambda: fedavg([A], None, 1), b"d_scales is NULL"),
        (lambda: fedavg([A], [B], 1, h_w=None), b"h_w is NULL"),
        (lambda: fedavg([A, 0], [B, B], 2), b"code row 1 is NULL"),
        (lambda: fedavg([A, A + 8], [B, B], 2), b"code row 1 is not 16-B aligned"),
        (lambda: fedavg([A], [0], 1), b"scale row 0 is NULL"),
        (lambda: fedavg([A], [B], 1, out=None), b"d_out is NULL"),
        (lambda: fedavg([A], [B], 1, out=C + 2), b"d_out is not 4-B aligned"),
        (lambda: fedavg([A], [B], 1, P=1), b"h_idx is NULL"),
        (lambda: fedavg([A], [B], 1, P=1, h_idx=idx), b"index 0 is out of range"),
        (lambda: q(A, F16, 64, None, B, C, None), b"kind %d is not FEDAGG_F32 / FEDAGG_BF16" % F16),
        (lambda: q(A, F64, 64, A + 4096, B, C, None), b"is not FEDAGG_F32 / FEDAGG_BF16"),
        (lambda: q(None, F32, 64, None, B, C, None), b"d_x is NULL"),
        (lambda: q(A + 1, BF16, 64, None, B, C, None), b"d_x is not aligned"),
        (lambda: q(A, F32, 64, A + 4098, B, C, None), b"d_res is not 4-B aligned"),
        (lambda: q(A, F32, 64, None, None, C, None), b"d_codes is NULL"),
        (lambda: q(A, F32, 64, None, B, None, None), b"d_scales is NULL"),
        (lambda: q(A, F32, 64, A + 128, B, C, None), b"d_res overlaps d_x"),
        (lambda: q(A, F32, 64, B - 128, B, C, None), b"d_res overlaps d_codes"),
    ]
    for call, text in cases:
        assert call() == -1 and text in lib.fedagg_mx4_last_error(), text
    assert lib.fedagg_mx4_fedavg_e2m1(_native.ptr_array([0]), _native.ptr_array([0]), w, 1, 0, None, 0, None, None) == 0
    assert q(None, F32, 0, None, None, None, None) == 0  # nothing to do launches nothing
    tile, group = _native_mx4.blocking()
    assert tile % (64 * 32) == 0 and group >= 2 and lib.fedagg_mx4_abi_version() == _native_mx4.ABI_VERSION
