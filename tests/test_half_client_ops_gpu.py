"""The client flat ops on fp16 and bf16 layers (``fedagg_flat_gather`` / ``fedagg_flat_wsum`` with
kinds F16 / BF16, ``fedagg_flat_increment_kind``, and :mod:`substrafl_amd.algorithms.weight_manager`
on 16-bit models) against the same torch ops on the device (weight_manager.py:103-212 restated
inline).  Bit for bit on int16 views; where torch gives NaN only NaN-ness is compared."""

import ctypes

import numpy as np
import pytest
import torch

from substrafl_amd import _native, wire
from substrafl_amd.algorithms import weight_manager as wm

KINDS = {"f16": (torch.float16, _native.FEDAGG_F16), "bf16": (torch.bfloat16, _native.FEDAGG_BF16)}
# odd and even flat offsets, an empty layer, the 8192-element chunk edges; 70 layers cross the
# 32-layer launch group twice
GEOMETRY = {"edges": [3, 1, 8, 7, 0, 9, 8191, 8192, 8193, 16384 + 5], "many": list(range(1, 71))}
GUARD = 64
SENTINEL = 0x5A5A
# +-0, +-inf, NaN, subnormals, max finite
SPECIALS = {torch.float16: [0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0x0001, 0x83FF, 0x7BFF, 0xFBFF],
            torch.bfloat16: [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0x0001, 0x807F, 0x7F7F, 0xFF7F]}
WSUM_COEFFS = [[1, -1], [1, 1], [-1.0, -1.0 / (0.05 * 100)], [0.3, 1 / 3, -1e-3, 7.7], [0.3, 1 / 3, -1e-3], [0.3]]


@pytest.fixture(params=[1, 0], ids=["vec16", "scalar"])
def flat_path(request):
    _native.tune(flat_vec=request.param)
    yield request.param
    _native.tune(flat_vec=1)


def _values(n, dtype, seed):
    """n elements on the device: ~45 % random bit patterns, ~10 % specials, the rest N(0, 1)."""
    rng = np.random.default_rng(seed)
    normal = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dtype).view(torch.int16).numpy()
    bits = rng.integers(0, 1 << 16, n, dtype=np.uint16).view(np.int16)
    special = rng.choice(np.array(SPECIALS[dtype], dtype=np.uint16), n).view(np.int16)
    pick = rng.random(n)
    out = np.where(pick < 0.45, bits, np.where(pick < 0.55, special, normal)).astype(np.int16)
    return torch.from_numpy(out).view(dtype).cuda()


def _guarded(numel, dtype, seed):
    """Per layer a buffer of n + GUARD elements (the guard holds a sentinel) and its first n
    elements as the layer; every layer buffer is its own allocation."""
    bufs, layers = [], []
    for i, n in enumerate(numel):
        buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.int16, device="cuda").view(dtype)
        buf[:n] = _values(n, dtype, seed * 1000 + i)
        bufs.append(buf)
        layers.append(buf[:n])
    return bufs, layers


def _guards_intact(bufs, numel):
    return all(bool((b.view(torch.int16)[n:] == SENTINEL).all()) for b, n in zip(bufs, numel))


def _flat_out(total, dtype):
    return torch.full((total + GUARD,), SENTINEL, dtype=torch.int16 if dtype != torch.float32 else torch.int32,
                      device="cuda").view(dtype)


def _assert_same(got, ref, what=""):
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), what
    bad = (~nan) & (got.view(torch.int16) != ref.view(torch.int16))
    if bool(bad.any()):
        idx = torch.nonzero(bad.reshape(-1)).flatten()
        first = [(int(i), hex(int(got.reshape(-1).view(torch.int16)[i]) & 0xFFFF),
                  hex(int(ref.reshape(-1).view(torch.int16)[i]) & 0xFFFF)) for i in idx[:8].cpu().tolist()]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; (index, got, torch) {first}")


def _ptrs(lists):
    return _native.ptr_array([t.data_ptr() for lst in lists for t in lst])


def _stream():
    return int(torch.cuda.current_stream().cuda_stream)


BLOCK = 1 << 16


def _padded(tensors):
    """The tensors back to back at the start of one fresh allocation padded to a multiple of
    64 Ki elements.  The torch reference runs on such buffers because torch's own elementwise
    kernels on ROCm answer differently depending on where an element sits: whole aligned blocks
    take a vectorised path, the remainder of a tensor and every small or unaligned tensor an
    unrolled one, and for fp16 the unrolled path (torch 2.10, MI355X) does not give IEEE results
    at the edges: ``-0.0 + 1.0 * -0.0`` came out ``+0.0`` (what a product formed as a fused
    multiply-add with a +0.0 addend gives), fp16 subnormal inputs multiplied by a scalar differ
    between a 100-element tensor and the same elements inside a 65536-element one, and sums
    that sit on a rounding boundary then move by one ulp (measured: 8 of 2485 elements of the
    70-layer geometry, 5 of 40993 of the other, all inside tensor remainders; all 65536 bit
    patterns through the vectorised path: 0 differences from the CPU's result and from the rules
    in fedagg.h, for every coefficient and multiplier used here).
    Padded, every element takes the vectorised path, whatever the layer sizes."""
    n = sum(t.numel() for t in tensors)
    buf = torch.zeros(-(-max(n, 1) // BLOCK) * BLOCK, dtype=tensors[0].dtype, device=tensors[0].device)
    if n:
        buf[:n] = torch.cat([t.reshape(-1) for t in tensors])
    return buf


def _unpadded(flat, like):
    return [v.reshape(t.shape) for v, t in zip(torch.split(flat[: sum(t.numel() for t in like)],
                                                           [t.numel() for t in like]), like)]


def ref_wsum(lists, coeffs):  # weight_manager.py:205-210, every layer at once
    return _unpadded(sum(_padded(lst) * c for lst, c in zip(lists, coeffs)), lists[0])


def ref_increment(w, u, mult):  # weight_manager.py:137
    flat = _padded(w)
    flat += mult * _padded(u)
    return _unpadded(flat, w)


@pytest.mark.gpu
@pytest.mark.parametrize("geometry", sorted(GEOMETRY))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_native_half_ops_bit_exact_with_guard_bands(kind, geometry, flat_path):
    assert torch.cuda.is_available()
    dtype, code = KINDS[kind]
    numel = GEOMETRY[geometry]
    total = sum(numel)
    lib = _native.load()
    n_arr = (ctypes.c_uint64 * len(numel))(*numel)
    bufs = [_guarded(numel, dtype, seed) for seed in range(4)]
    lists = [b[1] for b in bufs]

    # gather: plain copies (every bit pattern, NaN payloads included)
    flat = _flat_out(total, dtype)
    _native.check(lib.fedagg_flat_gather(_ptrs(lists[:1]), code, n_arr, len(numel), flat.data_ptr(), _stream()),
                  "flat_gather")
    assert torch.equal(flat[:total].view(torch.int16), torch.cat(lists[0]).view(torch.int16))
    assert bool((flat.view(torch.int16)[total:] == SENTINEL).all())

    # wsum: 1 to 4 lists
    for coeffs in WSUM_COEFFS:
        nl = len(coeffs)
        flat = _flat_out(total, dtype)
        kinds = (ctypes.c_int * nl)(*([code] * nl))
        c_arr = (ctypes.c_double * nl)(*[float(c) for c in coeffs])
        _native.check(lib.fedagg_flat_wsum(_ptrs(lists[:nl]), kinds, nl, c_arr, n_arr, len(numel), flat.data_ptr(),
                                           code, _stream()), "flat_wsum")
        ref = torch.cat([r.reshape(-1) for r in ref_wsum(lists[:nl], coeffs)])
        _assert_same(flat[:total], ref, f"wsum {coeffs}")
        assert bool((flat.view(torch.int16)[total:] == SENTINEL).all()), coeffs
    assert all(_guards_intact(b[0], numel) for b in bufs)


TORCH_MIXED_BLOCK = 16384


def _promoted_add_as_rocm_torch(r, uu, mult):
    """The (BF16, F32) rule of fedagg.h spelled out in single-dtype torch ops: ``t = fl32(m * u)``,
    ``w = bf16(fl32(w) + t)``, with ``t`` rounded to bf16 first in the layer's leading full blocks
    of 16384 elements -- how torch on ROCm adds an aligned contiguous bf16 tensor and an fp32
    tensor (its type-specialised vectorised kernel converts both inputs to the output type in
    every full block and leaves the remainder to the generic kernel, which rounds once)."""
    t = (mult * uu).reshape(-1).clone()
    full = t.numel() // TORCH_MIXED_BLOCK * TORCH_MIXED_BLOCK
    t[:full] = t[:full].to(torch.bfloat16).float()
    r.copy_((r.float() + t.reshape(r.shape)).to(torch.bfloat16))


def _native_increment(kind, geometry, u_dtype, u_code, explicit_rule=False):
    dtype, code = KINDS[kind]
    numel = GEOMETRY[geometry]
    total = sum(numel)
    lib = _native.load()
    n_arr = (ctypes.c_uint64 * len(numel))(*numel)
    for mult in (1.0, 0.05, -2.5):
        w_bufs, w = _guarded(numel, dtype, 7)
        if u_dtype == torch.float32:
            u = _flat_out(total, torch.float32)
            # bf16-representable specials and ordinary fp32 values
            u[:total] = torch.where(torch.rand(total, device="cuda") < 0.5, _values(total, dtype, 8).float(),
                                    torch.randn(total, device="cuda"))
        else:
            u = _flat_out(total, dtype)
            u[:total] = _values(total, dtype, 9)
        if u_dtype == dtype:
            ref = ref_increment(w, list(torch.split(u[:total], numel)), mult)
        else:
            ref = [t.clone() for t in w]
            for r, uu in zip(ref, torch.split(u[:total], numel)):
                if explicit_rule:
                    _promoted_add_as_rocm_torch(r, uu, mult)
                else:  # the update a tensor of its own, as the reference brings each layer to the device
                    r.data += mult * uu.clone().data  # weight_manager.py:137
        u_before = u.clone()
        _native.check(lib.fedagg_flat_increment_kind(_ptrs([w]), code, n_arr, len(numel), u.data_ptr(), u_code,
                                                     mult, _stream()), "flat_increment_kind")
        for li, (g, r) in enumerate(zip(w, ref)):
            _assert_same(g, r, f"increment {u_dtype} x {mult}, layer {li} of {numel[li]}")
        assert _guards_intact(w_bufs, numel)
        assert torch.equal(u.view(torch.int16), u_before.view(torch.int16))  # the update is only read


@pytest.mark.gpu
@pytest.mark.parametrize("geometry", sorted(GEOMETRY))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_native_increment_same_kind_bit_exact(kind, geometry, flat_path):
    """(F16, F16) and (BF16, BF16): ``w += m * u`` with the update of the model's kind."""
    assert torch.cuda.is_available()
    _native_increment(kind, geometry, *KINDS[kind])


@pytest.mark.gpu
@pytest.mark.parametrize("geometry", sorted(GEOMETRY))
def test_native_increment_bf16_by_fp32_promoted_add(geometry, flat_path):
    """(BF16, F32) against the rule of fedagg.h spelled out in single-dtype torch ops."""
    assert torch.cuda.is_available()
    _native_increment("bf16", geometry, torch.float32, _native.FEDAGG_F32, explicit_rule=True)


@pytest.mark.gpu
@pytest.mark.parametrize("geometry", sorted(GEOMETRY))
def test_native_increment_bf16_by_fp32_vs_torch_inplace_add(geometry, flat_path):
    """(BF16, F32) against ``w.data += m * u`` on the device, each layer's operands tensors of
    their own as in the reference.  The 16384 + 5 element layer of "edges" is where torch on ROCm
    rounds twice: with the one-rounding rule alone, 1073 to 1162 of its 16389 elements were one
    bf16 ulp off at m = 1.0 (torch 2.10, MI355X), and none in the smaller layers."""
    assert torch.cuda.is_available()
    _native_increment("bf16", geometry, torch.float32, _native.FEDAGG_F32)


@pytest.mark.gpu
def test_native_half_ops_reject_mixed_kinds():
    assert torch.cuda.is_available()
    lib = _native.load()
    a = torch.zeros(64, dtype=torch.float16, device="cuda")
    b = torch.zeros(64, dtype=torch.float32, device="cuda")
    c = torch.zeros(64, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(64, dtype=torch.float32, device="cuda")
    numel = (ctypes.c_uint64 * 1)(64)
    two = (ctypes.c_double * 2)(1.0, -1.0)
    for kinds, lists, flat_kind in (([_native.FEDAGG_F16, _native.FEDAGG_F32], [[a], [b]], _native.FEDAGG_F32),
                                    ([_native.FEDAGG_F16, _native.FEDAGG_F32], [[a], [b]], _native.FEDAGG_F16),
                                    ([_native.FEDAGG_F16, _native.FEDAGG_BF16], [[a], [c]], _native.FEDAGG_F16),
                                    ([_native.FEDAGG_BF16, _native.FEDAGG_BF16], [[c], [c]], _native.FEDAGG_F32)):
        assert lib.fedagg_flat_wsum(_ptrs(lists), (ctypes.c_int * 2)(*kinds), 2, two, numel, 1, out.data_ptr(),
                                    flat_kind, None) == -1
    for layer_kind, flat_kind in ((_native.FEDAGG_F16, _native.FEDAGG_F32), (_native.FEDAGG_F16, _native.FEDAGG_BF16),
                                  (_native.FEDAGG_BF16, _native.FEDAGG_F16), (_native.FEDAGG_F32, _native.FEDAGG_F32),
                                  (_native.FEDAGG_BF16, _native.FEDAGG_F64)):
        assert lib.fedagg_flat_increment_kind(_ptrs([[a]]), layer_kind, numel, 1, out.data_ptr(), flat_kind, 1.0,
                                              None) == -1
    torch.cuda.synchronize()
    assert not a.any() and not out.any()  # nothing ran


class _Layers(torch.nn.Module):
    def __init__(self, numel, dtype, seed):
        super().__init__()
        self.ps = torch.nn.ParameterList(
            [torch.nn.Parameter(_values(n, dtype, seed * 100 + i), requires_grad=False) for i, n in enumerate(numel)])


def _host_as_device(u, dtype):
    """A host layer as torch brings it to the device (``wire.BF16``: its bit patterns as bf16)."""
    u = np.asarray(u)
    t = torch.from_numpy(u.view(np.int16)).view(torch.bfloat16) if u.dtype == wire.BF16 else torch.from_numpy(u)
    assert t.dtype == dtype
    return t.cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_weight_manager_half_model_round(kind, flat_path):
    """One client round of weight moves on a 16-bit model: every result is ONE flat bucket and
    equals the per-layer torch ops; the layers of the later ops are views of earlier buckets, at
    whatever alignment their offsets give."""
    assert torch.cuda.is_available()
    dtype, _ = KINDS[kind]
    numel = [n for n in GEOMETRY["edges"] if n]  # a Parameter of 0 elements is legal but no model has one
    model = _Layers(numel, dtype, 1)
    params = lambda m: list(wm.model_parameters(m, False)())  # noqa: E731

    before = wm.get_parameters(model, False)
    assert wm.flat_bucket(before) is not None
    for g, p in zip(before, params(model)):
        assert g.data_ptr() != p.data_ptr() and torch.equal(g.view(torch.int16), p.data.view(torch.int16))

    trained = [_values(n, dtype, 50 + i) for i, n in enumerate(numel)]
    wm.set_parameters(model, trained, False)
    after = wm.get_parameters(model, False)
    for lists, coeffs, fn in (([after, before], [1, -1], wm.subtract_parameters),
                              ([after, before], [1, 1], wm.add_parameters)):
        got = fn(*lists)
        assert wm.flat_bucket(got) is not None
        for g, r in zip(got, ref_wsum(lists, coeffs)):
            _assert_same(g, r, str(coeffs))
    for coeffs in WSUM_COEFFS:
        lists = [after, before, trained, after][: len(coeffs)]
        got = wm.weighted_sum_parameters(lists, coeffs)
        assert wm.flat_bucket(got) is not None
        for g, r in zip(got, ref_wsum(lists, coeffs)):
            _assert_same(g, r, str(coeffs))
    # a 16-bit list next to an fp32 list: torch's promotion, on torch
    mixed = wm.weighted_sum_parameters([after, [t.float() for t in before]], [1, -1])
    assert all(m.dtype == torch.float32 for m in mixed)

    delta = wm.subtract_parameters(after, before)
    wm.set_parameters(model, before, False)  # the parameters are now views of one bucket

    # export: one buffer, fp16 as np.float16 and bf16 as wire.BF16 bit patterns
    for as_wire in (True, False):
        host = wm.export_numpy(delta, wire=as_wire, tag=f"half-{kind}-{as_wire}")
        want = np.dtype(np.float16) if kind == "f16" else wire.BF16
        assert all(isinstance(h, np.ndarray) and h.dtype == want and h.shape == d.shape for h, d in zip(host, delta))
        assert (wire.flat_of(host) is not None) == as_wire
        addr = [h.__array_interface__["data"][0] for h in host]
        assert addr == [addr[0] + 2 * int(o) for o in np.cumsum([0] + numel[:-1])]  # back to back in one buffer
        for h, d in zip(host, delta):
            assert np.array_equal(np.asarray(h).view(np.int16), d.view(torch.int16).cpu().numpy())
    host = wm.export_numpy(delta, wire=True, tag=f"half-{kind}")

    # increment: a host bucket and device tensors of the model's kind
    for name, u in (("host", host), ("device", delta)):
        for mult in (1.0, 0.05, -2.5):
            ref = ref_increment([p.data for p in params(model)],
                                [uu if isinstance(uu, torch.Tensor) else _host_as_device(uu, dtype) for uu in u], mult)
            wm.increment_parameters(model, list(u), with_batch_norm_parameters=False, updates_multiplier=mult)
            for li, (p, r) in enumerate(zip(params(model), ref)):
                _assert_same(p.data, r, f"increment {name} x {mult}, layer {li}")
    assert wm.flat_bucket([p.data for p in params(model)]) is not None  # updated in place


def _bf16_model_incremented_by_fp32(explicit_rule):
    """A bf16 model whose parameters are views of one bucket, incremented by fp32 views of one
    host array (the engine's average) and by fp32 device tensors."""
    numel = [n for n in GEOMETRY["edges"] if n]
    model = _Layers(numel, torch.bfloat16, 1)
    params = lambda: list(wm.model_parameters(model, False)())  # noqa: E731
    wm.set_parameters(model, wm.get_parameters(model, False), False)
    f32 = np.random.default_rng(5).standard_normal(sum(numel)).astype(np.float32)
    f32[::7] = _values(sum(numel), torch.bfloat16, 6).float().cpu().numpy()[::7]  # specials, bf16-exact values
    views = list(np.split(f32, np.cumsum(numel)[:-1]))
    for name, u in (("host", views), ("device", [torch.from_numpy(v).cuda() for v in views])):
        for mult in (1.0, 0.05, -2.5):
            ref = [p.data.clone() for p in params()]
            for r, uu in zip(ref, u):
                uu = uu if isinstance(uu, torch.Tensor) else _host_as_device(uu, torch.float32)
                if explicit_rule:
                    _promoted_add_as_rocm_torch(r, uu, mult)
                else:
                    r.data += mult * uu.data  # weight_manager.py:137
            wm.increment_parameters(model, list(u), with_batch_norm_parameters=False, updates_multiplier=mult)
            for li, (p, r) in enumerate(zip(params(), ref)):
                _assert_same(p.data, r, f"increment fp32 {name} x {mult}, layer {li}")
    assert wm.flat_bucket([p.data for p in params()]) is not None  # the flat kernel ran, in place


@pytest.mark.gpu
def test_weight_manager_bf16_model_fp32_update_promoted_add(flat_path):
    """A bf16 model receives the engine's fp32 average: the rule of fedagg.h spelled out."""
    assert torch.cuda.is_available()
    _bf16_model_incremented_by_fp32(explicit_rule=True)


@pytest.mark.gpu
def test_weight_manager_bf16_model_fp32_update_vs_torch_inplace_add(flat_path):
    """The same against ``w.data += m * u`` on the device (the reference's own expression)."""
    assert torch.cuda.is_available()
    _bf16_model_incremented_by_fp32(explicit_rule=False)
