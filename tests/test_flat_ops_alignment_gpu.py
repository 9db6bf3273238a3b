"""The client flat ops on layers that are not 16-B aligned: every layer is a view that starts
``o`` elements past a 16-B boundary of its own allocation.  Alignment may change which accesses a
kernel uses (16-B or element by element) but never a bit: each op must give, on bit patterns, what
the same call gives on 16-B aligned copies of the same data, and must leave the sentinel elements
before and after every view untouched.  (What the ops compute is pinned against torch in
test_client_buckets.py and test_half_client_ops_gpu.py; their value generators -- +-0,
subnormals, +-inf, NaN, rounding ties -- are the ones used here.)"""

import ctypes
import functools

import pytest
import torch

from substrafl_amd import _native

from test_client_buckets import _operand
from test_half_client_ops_gpu import _values

# 1 element, one short of / exactly / one past a 16-bit vector, and the 8192-element chunk edge
SIZES = [1, 7, 8, 9, 8185, 8192, 8193]
MIXED_SIZES = SIZES + [16384 + 9]  # one full 16384-element block of the bf16-by-fp32 rule and a remainder
GUARD = 64  # elements: 128 or 256 bytes, so a view at GUARD + o sits o elements past a 16-B boundary
KINDS = {"f16": (torch.float16, _native.FEDAGG_F16), "bf16": (torch.bfloat16, _native.FEDAGG_BF16)}
WSUM_COEFFS = [(1, -1), (0.3, 0.7)]
MULT = 0.3


@pytest.fixture(params=[1, 0], ids=["vec16", "scalar"])
def flat_path(request):
    _native.tune(flat_vec=request.param)
    yield request.param
    _native.tune(flat_vec=1)


def _int(dtype):
    return torch.int32 if dtype == torch.float32 else torch.int16


def _sentinel(dtype):
    return 0x5A5A5A5A if dtype == torch.float32 else 0x5A5A


def _place(tensors, o):
    """Each tensor copied into an allocation of its own, GUARD + o sentinel elements in front of
    it and GUARD behind: (allocations, views)."""
    bufs, views = [], []
    for t in tensors:
        buf = torch.full((GUARD + o + t.numel() + GUARD,), _sentinel(t.dtype), dtype=_int(t.dtype),
                         device="cuda").view(t.dtype)
        view = buf[GUARD + o: GUARD + o + t.numel()]
        view.copy_(t)
        assert view.data_ptr() % 16 == (o * t.element_size()) % 16
        bufs.append(buf)
        views.append(view)
    return bufs, views


def _guards_intact(bufs, views, o):
    for buf, v in zip(bufs, views):
        b = buf.view(_int(buf.dtype))
        if not (bool((b[:GUARD + o] == _sentinel(buf.dtype)).all())
                and bool((b[GUARD + o + v.numel():] == _sentinel(buf.dtype)).all())):
            return False
    return True


def _bits(tensors):
    return torch.cat([t.reshape(-1) for t in tensors]).view(_int(tensors[0].dtype)).clone()


def _ptrs(*lists):
    return _native.ptr_array([t.data_ptr() for lst in lists for t in lst])


def _n_arr(sizes):
    return (ctypes.c_uint64 * len(sizes))(*sizes)


def _stream():
    return int(torch.cuda.current_stream().cuda_stream)


def _assert_same_bits(got, want, o):
    assert got.keys() == want.keys()
    for name in got:
        bad = torch.nonzero(got[name] != want[name]).flatten()
        assert bad.numel() == 0, (f"{name} at offset {o}: {bad.numel()} of {got[name].numel()} elements differ "
                                  f"from the aligned call, first at {bad[:8].tolist()}")


@functools.lru_cache(maxsize=None)
def _data16(kind):
    dtype, _ = KINDS[kind]
    lists = [[_values(n, dtype, 100 * j + i) for i, n in enumerate(SIZES)] for j in range(2)]
    return lists, _values(sum(SIZES), dtype, 7)


def _ops16(kind, o):
    """gather, the two weighted sums and the same-kind increment on layers placed at offset o:
    {op: bit patterns of its result}."""
    dtype, code = KINDS[kind]
    lib = _native.load()
    lists, update = _data16(kind)
    total, n_arr, L = sum(SIZES), _n_arr(SIZES), len(SIZES)
    (bufs0, l0), (bufs1, l1) = _place(lists[0], o), _place(lists[1], o)
    out = {}
    (fbuf,), (flat,) = _place([torch.zeros(total, dtype=dtype, device="cuda")], 0)
    _native.check(lib.fedagg_flat_gather(_ptrs(l0), code, n_arr, L, flat.data_ptr(), _stream()), "flat_gather")
    out["gather"] = _bits([flat])
    assert torch.equal(out["gather"], _bits(lists[0]))
    for coeffs in WSUM_COEFFS:
        _native.check(lib.fedagg_flat_wsum(_ptrs(l0, l1), (ctypes.c_int * 2)(code, code), 2,
                                           (ctypes.c_double * 2)(*map(float, coeffs)), n_arr, L, flat.data_ptr(), code,
                                           _stream()), "flat_wsum")
        out[f"wsum {coeffs}"] = _bits([flat])
    assert _guards_intact([fbuf], [flat], 0)
    (ubuf,), (u,) = _place([update], 0)
    _native.check(lib.fedagg_flat_increment_kind(_ptrs(l0), code, n_arr, L, u.data_ptr(), code, MULT, _stream()),
                  "flat_increment_kind")
    out["increment"] = _bits(l0)
    assert torch.equal(_bits([u]), _bits([update])) and _guards_intact([ubuf], [u], 0)  # the update is only read
    assert _guards_intact(bufs0, l0, o) and _guards_intact(bufs1, l1, o)
    assert torch.equal(_bits(l1), _bits(lists[1]))
    return out


@functools.lru_cache(maxsize=None)
def _aligned16(kind, flat_vec):
    return _ops16(kind, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("o", [0, 1, 2, 4, 8])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_16bit_ops_same_bits_at_every_layer_alignment(kind, o, flat_path):
    assert torch.cuda.is_available()
    _assert_same_bits(_ops16(kind, o), _aligned16(kind, flat_path), o)


@functools.lru_cache(maxsize=None)
def _data_mixed():
    w = [_values(n, torch.bfloat16, 300 + i) for i, n in enumerate(MIXED_SIZES)]
    total = sum(MIXED_SIZES)
    g = torch.Generator(device="cuda").manual_seed(5)
    # bf16-representable specials and ordinary fp32 values (most of them no bf16 value: rounding matters)
    u = torch.where(torch.rand(total, device="cuda", generator=g) < 0.5, _values(total, torch.bfloat16, 8).float(),
                    torch.randn(total, device="cuda", generator=g))
    return w, u


def _increment_mixed(o, mult):
    lib = _native.load()
    w, update = _data_mixed()
    bufs, layers = _place(w, o)
    (ubuf,), (u,) = _place([update], 0)
    _native.check(lib.fedagg_flat_increment_kind(_ptrs(layers), _native.FEDAGG_BF16, _n_arr(MIXED_SIZES),
                                                 len(MIXED_SIZES), u.data_ptr(), _native.FEDAGG_F32, mult, _stream()),
                  "flat_increment_kind")
    assert _guards_intact(bufs, layers, o) and _guards_intact([ubuf], [u], 0)
    assert torch.equal(_bits([u]), _bits([update]))
    return {f"bf16 += {mult} * fp32": _bits(layers)}


@functools.lru_cache(maxsize=None)
def _aligned_mixed(mult, flat_vec):
    return _increment_mixed(0, mult)


@pytest.mark.gpu
@pytest.mark.parametrize("o", [0, 1, 2, 4, 8])
def test_bf16_by_fp32_increment_same_bits_at_every_layer_alignment(o, flat_path):
    """The rule that rounds the update twice counts elements from the start of the layer, not from
    an address, so it too is blind to the layer's alignment."""
    assert torch.cuda.is_available()
    for mult in (1.0, MULT):
        _assert_same_bits(_increment_mixed(o, mult), _aligned_mixed(mult, flat_path), o)


@functools.lru_cache(maxsize=None)
def _data32():
    return [[t.cuda() for t in _operand(SIZES, torch.float32, 30 + j)] for j in range(3)]


def _ops32(o):
    """The fp32 entry points on layers at offset o: gather, the weighted sums, increment, and
    gather -> scatter into fresh layers at the same offset."""
    lib = _native.load()
    lists = _data32()
    total, n_arr, L = sum(SIZES), _n_arr(SIZES), len(SIZES)
    (bufs0, l0), (bufs1, l1) = _place(lists[0], o), _place(lists[1], o)
    out = {}
    (fbuf,), (flat,) = _place([torch.zeros(total, device="cuda")], 0)
    _native.check(lib.fedagg_flat_gather_f32(_ptrs(l0), n_arr, L, flat.data_ptr(), _stream()), "flat_gather_f32")
    out["gather"] = _bits([flat])
    assert torch.equal(out["gather"], _bits(lists[0]))
    bufs2, l2 = _place([torch.zeros_like(t) for t in lists[0]], o)
    _native.check(lib.fedagg_flat_scatter_f32(_ptrs(l2), n_arr, L, flat.data_ptr(), _stream()), "flat_scatter_f32")
    out["gather -> scatter"] = _bits(l2)
    assert torch.equal(out["gather -> scatter"], _bits(lists[0])) and _guards_intact(bufs2, l2, o)
    for coeffs in WSUM_COEFFS:
        _native.check(lib.fedagg_flat_wsum_f32(_ptrs(l0, l1), 2, (ctypes.c_double * 2)(*map(float, coeffs)), n_arr, L,
                                               flat.data_ptr(), _stream()), "flat_wsum_f32")
        out[f"wsum {coeffs}"] = _bits([flat])
    assert _guards_intact([fbuf], [flat], 0)
    (ubuf,), (u,) = _place([torch.cat(lists[2])], 0)
    _native.check(lib.fedagg_flat_increment_f32(_ptrs(l0), n_arr, L, u.data_ptr(), MULT, _stream()),
                  "flat_increment_f32")
    out["increment"] = _bits(l0)
    assert torch.equal(_bits([u]), _bits(lists[2])) and _guards_intact([ubuf], [u], 0)
    assert _guards_intact(bufs0, l0, o) and _guards_intact(bufs1, l1, o)
    assert torch.equal(_bits(l1), _bits(lists[1]))
    return out


@functools.lru_cache(maxsize=None)
def _aligned32(flat_vec):
    return _ops32(0)


@pytest.mark.gpu
@pytest.mark.parametrize("o", [0, 1, 2, 3])
def test_fp32_ops_same_bits_at_every_layer_alignment(o, flat_path):
    assert torch.cuda.is_available()
    _assert_same_bits(_ops32(o), _aligned32(flat_path), o)
