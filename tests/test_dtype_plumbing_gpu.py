"""The dtype plumbing that feeds the aggregation kernels, bit for bit against NumPy:

* ``fedagg_cast`` / ``fedagg_scale_cast`` directly (``runtime.Session.cast`` / ``.scale_cast`` on
  torch device buffers): every pair the C ABI accepts, on a table of edge values (integer -> float
  ties past 2^24 / 2^53, fp16 overflow and subnormal edges, double-rounding traps) plus seeded
  random bit patterns, with a guard band behind every output;
* the same conversions from the strategies: FedAvg with per-client dtype mixes inside one layer
  and whole-layer integer kinds, Scaffold inputs other than fp32 / fp64, and NewtonRaphson's
  widen, add, round-back step.

References: ``x.astype(out)`` and ``(x * w).astype(out)`` (``w`` a Python float: NEP 50, the
product in ``x``'s own type), the oracle's ``*_reference_structure`` (the reference's own NumPy
calls) and ``newton_raphson_sums``.  Where the reference is NaN only NaN-ness is compared (NaN
payloads are not part of the reference's behaviour, see tests/test_gpu_parity.py).

One CPU test keeps the table honest: every trap input must still separate NumPy's single
rounding from the two-step conversion it is there to catch.  It is the one test of this file
without the ``gpu`` mark, which is why the mark is set per test and not per module."""

import numpy as np
import pytest

from oracle import fedavg_reference_structure, newton_raphson_sums, scaffold_reference_structure

gpu = pytest.mark.gpu

KINDS = {"f16": np.float16, "f32": np.float32, "f64": np.float64, "i8": np.int8, "i16": np.int16, "i32": np.int32,
         "i64": np.int64, "u8": np.uint8, "u16": np.uint16, "u32": np.uint32, "u64": np.uint64, "bool": np.bool_}
FLOATS = ("f16", "f32", "f64")
NRAND = 1000
GUARD = 0xA5

# ------------------------------------------------------------------------------------------
# the edge-value tables
# ------------------------------------------------------------------------------------------
T60 = 2**60 + 2**36 + 1  # -> f32: one rounding goes up; through double the +1 is lost and the tie goes to even
INT_EDGES = [
    0, 1, -1, 2, 3, 127, 128, 255, 256,
    2**24 + 1, 2**24 + 3, -(2**24 + 1), 2**24, 2**31 - 1, 2**31 + 129,  # f32 ties; >= 2^24 is +-inf in fp16
    T60, -T60, 2**63 - 1, -2**63, 2**63, 2**64 - 1,
    2**53 + 1, -(2**53 + 1), 2**53 + 3, 2**63 + 2**10 + 1,  # f64 ties
    2049, 2051, 65504, 65519, 65520, -65520, -2049, 2047, 4097, 32767 - 15,  # fp16 ties and the overflow edge
]


def _int_table(dt):
    info = np.iinfo(dt)
    vals = [info.min, info.min + 1, info.max, info.max - 1] + [v for v in INT_EDGES if info.min <= v <= info.max]
    return np.array(vals, dtype=dt)


W16 = 1 + 2**-11 + 2**-30  # double -> fp16: 0x3C01 in one rounding, 0x3C00 through float
D_SUB16 = 2**-25 * (1 + 2**-40)  # -> fp16: the smallest subnormal in one rounding, 0 through float
D_OVF16 = 65519.999  # -> fp16: 65504 in one rounding, inf through float
F32_MAX = float(np.finfo(np.float32).max)

F64_EDGES = [
    W16, -W16, D_SUB16, -D_SUB16, D_OVF16, -D_OVF16,  # the three double-rounding traps (f64 -> f16)
    2**-25, 65520.0, -65520.0, 65504.0, 65519.0, 1 + 2**-11, 1 + 3 * 2**-11, 2**-24 * 1.5, 2**-24 * 2.5,
    2**-14 - 2**-25, 2**-14 - 2**-26,  # ties and edges of f64 -> f16
    # f64 -> f32 ties and their neighbours (the first IS 1 + 2^-24 in fp64: a tie)
    1 + 2**-24 + 2**-60, 1 + 2**-24 + 2**-52, 1 + 3 * 2**-24, 1 + 2**-24 - 2**-53,
    F32_MAX + 2**103, float(np.nextafter(F32_MAX + 2**103, 0)), -(F32_MAX + 2**103), F32_MAX * 2,  # f32 overflow edge
    2**-150, 2**-150 * (1 + 2**-40), 2**-149 * 1.5, 2**-149 * 2.5, 2**-126 - 2**-150,  # f32 subnormal edge
    1e-320, 1e300, -1e300, 0.1, 1 / 3,
]
F32_EDGES = [
    1 + 2**-11, 1 + 3 * 2**-11, 1 + 2**-11 + 2**-23, 1 + 2**-11 - 2**-24,  # f32 -> f16 ties and their neighbours
    65520.0, -65520.0, float(np.nextafter(np.float32(65520), np.float32(0))), 65504.0, 65519.0, 70000.0,
    2**-25, float(np.nextafter(np.float32(2**-25), np.float32(1))), 2**-24 * 1.5, 2**-24 * 2.5, 2**-14 - 2**-25,
    1e-40, 9.0, 13.0, 0.1, 1 / 3, 3.0e38, -3.0e38,
]
F16_EDGES = [1.0, 3.0, 2049.0, 0.1, 1 / 3, 1e-7, 6e-5, 300.0, -300.0, 60000.0]


def _float_table(dt):
    info = np.finfo(dt)
    bits = {2: np.uint16, 4: np.uint32, 8: np.uint64}[np.dtype(dt).itemsize]
    qnan = np.array([np.nan], dt).view(bits)
    top = bits(1) << bits(8 * np.dtype(dt).itemsize - 1)
    nans = np.concatenate([qnan, qnan | top, qnan | bits(5),  # quiet: plain, negative, with a payload
                           np.array([np.inf], dt).view(bits) | bits(3),  # signalling
                           np.array([np.inf], dt).view(bits) | bits(3) | top]).view(dt)
    common = [0.0, -0.0, np.inf, -np.inf, info.max, -info.max, info.tiny, -info.tiny, info.smallest_subnormal,
              -info.smallest_subnormal, info.tiny / 4, info.tiny - info.smallest_subnormal, 1.0, -1.0, 3.0, 0.5]
    extra = {np.float16: F16_EDGES, np.float32: F32_EDGES + F16_EDGES, np.float64: F64_EDGES + F32_EDGES + F16_EDGES}[dt]
    return np.concatenate([nans, np.array(common + extra, dtype=dt)])


def _ties_into(narrow, wide, rng, count=200):
    """Halfway points between neighbouring finite ``narrow`` values and their two neighbours in
    ``wide``: exact ties (to even) and the nearest values either side of them."""
    nbits = {2: np.uint16, 4: np.uint32}[np.dtype(narrow).itemsize]
    top = 1 << (8 * np.dtype(narrow).itemsize - 1)
    lo = rng.integers(0, int(np.array([np.finfo(narrow).max], narrow).view(nbits)[0]), count).astype(nbits)
    lo |= (rng.integers(0, 2, count) * top).astype(nbits)
    a = lo.view(narrow).astype(wide)
    b = (lo + nbits(1)).view(narrow).astype(wide)  # the next value away from zero
    mid = (a + b) / wide(2)  # exact: one more bit than narrow has
    return np.concatenate([mid, np.nextafter(mid, wide(0)), np.nextafter(mid, np.copysign(wide(np.inf), mid))])


_INPUTS = {}


def inputs(kind):
    """Table + ~1000 seeded random bit patterns (+ generated ties for the wider float kinds)."""
    if kind not in _INPUTS:
        dt = KINDS[kind]
        rng = np.random.default_rng(sorted(KINDS).index(kind) + 77)
        with np.errstate(all="ignore"):
            if kind == "bool":
                x = np.concatenate([np.array([False, True]), rng.integers(0, 2, NRAND).astype(np.bool_)])
            elif kind in FLOATS:
                isz = np.dtype(dt).itemsize
                rand = rng.integers(0, 256, NRAND * isz, dtype=np.uint8).view(dt)
                parts = [_float_table(dt), rand]
                if kind != "f16":
                    parts.append(_ties_into(np.float16, dt, rng))
                if kind == "f64":
                    parts.append(_ties_into(np.float32, dt, rng))
                x = np.concatenate(parts)
            else:
                isz = np.dtype(dt).itemsize
                x = np.concatenate([_int_table(dt), rng.integers(0, 256, NRAND * isz, dtype=np.uint8).view(dt)])
        assert x.dtype == dt
        x.setflags(write=False)
        _INPUTS[kind] = x
    return _INPUTS[kind]


W32 = 0.7  # fl32(9 * 0.7) != fl32(9) * fl32(0.7): the product must be formed with the weight rounded to fp32
WEIGHTS = [1 / 3, 0.1, -0.25, 0.0, -0.0, 1.0, W16, W32]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _via(x, *steps):
    with np.errstate(all="ignore"):
        for dt in steps:
            x = x.astype(dt)
    return x


# ------------------------------------------------------------------------------------------
# CPU: the traps still discriminate under the installed NumPy
# ------------------------------------------------------------------------------------------
def test_trap_inputs_discriminate_one_rounding_from_two():
    """A test on these inputs is evidence only while NumPy's own (single-rounding) result differs
    from the two-step result: checked per trap, and that each trap is in the table the GPU tests
    run on."""
    # 64-bit integer -> f32: direct vs through double
    for kind, v in (("i64", T60), ("i64", -T60), ("u64", T60)):
        x = np.array([v], KINDS[kind])
        assert v in inputs(kind).tolist()
        assert _bits(_via(x, np.float32))[0] != _bits(_via(x, np.float64, np.float32))[0], (kind, v)
    # f64 -> f16: direct vs through float
    for v, direct in ((W16, 0x3C01), (D_SUB16, 0x0001), (D_OVF16, 0x7BFF), (-W16, 0xBC01)):
        x = np.array([v], np.float64)
        assert v in inputs("f64").tolist()
        assert _bits(_via(x, np.float16))[0] == direct, v
        assert _bits(_via(x, np.float32, np.float16))[0] != direct, v
    # the neighbours that make them edges: 2^-25 -> 0, 65520 -> inf, integer -> fp16 through float like NumPy
    assert _bits(_via(np.array([2**-25, 65520.0]), np.float16)).tolist() == [0x0000, 0x7C00]
    got = _via(np.array([2049, 2051, 65504, 65519, 65520, 2**24 + 1, 2**62], np.int64), np.float16)
    assert _bits(got).tolist() == _bits(np.array([2048, 2052, 65504, 65504, np.inf, np.inf, np.inf], np.float16)).tolist()
    # integer -> f32 / f64 ties (no two-step form to tell apart: the expected roundings themselves)
    assert _via(np.array([2**24 + 1, 2**24 + 3], np.int64), np.float32).tolist() == [2.0**24, 2.0**24 + 4]
    assert _via(np.array([2**53 + 1, 2**53 + 3], np.int64), np.float64).tolist() == [2.0**53, 2.0**53 + 4]
    assert _via(np.array([2**63 + 2**10 + 1, 2**64 - 1], np.uint64), np.float64).tolist() == [2.0**63 + 2048, 2.0**64]
    # the fp16 weight: np.float16(w) is one rounding of the double
    assert _bits(np.float16(W16)) == 0x3C01 and _bits(np.float16(np.float32(W16))) == 0x3C00
    prod = np.array([1, 3], np.float16) * W16
    assert prod.dtype == np.float16 and _bits(prod).tolist() == [0x3C01, 0x4202]
    assert 1.0 in inputs("f16").tolist() and 3.0 in inputs("f16").tolist() and W16 in WEIGHTS
    # the fp32 weight: the product in fp32 with the weight rounded to fp32 differs from the rounded double product
    x9 = np.array([9.0], np.float32)
    assert 9.0 in inputs("f32").tolist() and W32 in WEIGHTS
    assert (x9 * W32).dtype == np.float32
    assert _bits(x9 * W32)[0] != _bits(np.array([9.0 * W32]).astype(np.float32))[0]
    # every integer kind's extremes, and a value >= 2^24 wherever it fits
    for kind, dt in KINDS.items():
        if kind in FLOATS or kind == "bool":
            continue
        vals, info = inputs(kind).tolist(), np.iinfo(dt)
        assert info.min in vals and info.max in vals
        assert info.max < 2**24 or any(v >= 2**24 for v in vals[:60])


# ------------------------------------------------------------------------------------------
# GPU: the two entry points directly
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from substrafl_amd import _native, runtime

    _native.load()
    return torch, runtime.session(0)


def _run(dev, x, out_dt, w=None, n=None, offset=0):
    """``x[:n]`` through ``Session.cast`` (or ``.scale_cast`` with ``w``) into a guarded device
    buffer; input and output start ``offset`` elements past a 256-B boundary.  Returns the ``n``
    outputs after checking that no byte around them changed."""
    torch, s = dev
    x = np.ascontiguousarray(x if n is None else x[:n])
    n = x.size
    isz, osz = x.dtype.itemsize, np.dtype(out_dt).itemsize
    band = 256 + 8 * n  # holds any element-width mix-up (8-byte stores at fp16 indices included)
    t_in = torch.zeros(512 + n * isz, dtype=torch.uint8, device="cuda")
    i0 = (-t_in.data_ptr()) % 256 + offset * isz
    if n:
        t_in[i0:i0 + n * isz] = torch.from_numpy(x.view(np.uint8).copy()).cuda()
    t_out = torch.full((512 + n * osz + band,), GUARD, dtype=torch.uint8, device="cuda")
    o0 = (-t_out.data_ptr()) % 256 + offset * osz
    torch.cuda.synchronize()
    if w is None:
        s.cast(t_in.data_ptr() + i0, x.dtype, t_out.data_ptr() + o0, out_dt, n)
    else:
        s.scale_cast(t_in.data_ptr() + i0, x.dtype, w, t_out.data_ptr() + o0, out_dt, n)
    s.sync()
    raw = t_out.cpu().numpy()
    assert (raw[:o0] == GUARD).all(), "bytes before the output were written"
    assert (raw[o0 + n * osz:] == GUARD).all(), "bytes behind the n outputs were written (overrun)"
    return raw[o0:o0 + n * osz].copy().view(out_dt)


def _check(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    if ref.dtype.kind == "f":
        rn = np.isnan(ref)
        assert np.array_equal(np.isnan(got), rn), what
        bad = np.flatnonzero((_bits(got) != _bits(ref)) & ~rn)
    else:
        bad = np.flatnonzero(_bits(got) != _bits(ref))
    assert bad.size == 0, (what, bad[:8].tolist(), _bits(got)[bad[:8]].tolist(), _bits(ref)[bad[:8]].tolist())


def _cast_ref(x, out_dt):
    with np.errstate(all="ignore"):
        return x.astype(out_dt)


def _scale_ref(x, w, out_dt):
    assert type(w) is float
    with np.errstate(all="ignore"):
        return (x * w).astype(out_dt)


SIZES = (1, 255, 256, 257)


@gpu
@pytest.mark.parametrize("out_kind", FLOATS)
@pytest.mark.parametrize("in_kind", list(KINDS))
def test_cast_every_pair_bit_exact(dev, in_kind, out_kind):
    x, out_dt = inputs(in_kind), KINDS[out_kind]
    _check(_run(dev, x, out_dt), _cast_ref(x, out_dt), (in_kind, out_kind, "all"))
    for n in SIZES:
        xs = x[n:2 * n]  # another stretch of the vector per size
        _check(_run(dev, xs, out_dt), _cast_ref(xs, out_dt), (in_kind, out_kind, n))


@gpu
@pytest.mark.parametrize("out_kind", FLOATS)
@pytest.mark.parametrize("in_kind", FLOATS)
def test_scale_cast_every_pair_bit_exact(dev, in_kind, out_kind):
    x, out_dt = inputs(in_kind), KINDS[out_kind]
    for w in WEIGHTS:
        _check(_run(dev, x, out_dt, w=w), _scale_ref(x, w, out_dt), (in_kind, out_kind, w))
    for n in SIZES:
        xs = x[n:2 * n]
        _check(_run(dev, xs, out_dt, w=1 / 3), _scale_ref(xs, 1 / 3, out_dt), (in_kind, out_kind, n))


@gpu
@pytest.mark.parametrize("in_kind, out_kind", [("i64", "f16"), ("u64", "f32"), ("f64", "f16"), ("f16", "f64"),
                                               ("bool", "f32"), ("i8", "f64")])
def test_cast_grid_stride_loop(dev, in_kind, out_kind):
    """grid_cap = 3 with n = 2 * 3 * 256 + 5: every thread of the three workgroups takes two
    elements and the first five a third (the default grid gives every element its own thread)."""
    from substrafl_amd import _native

    n = 2 * 3 * 256 + 5
    x = np.resize(inputs(in_kind), n)
    _native.tune(grid_cap=3)
    try:
        got = _run(dev, x, KINDS[out_kind])
        sc = _run(dev, x, KINDS[out_kind], w=W16) if in_kind in FLOATS else None
    finally:
        _native.tune(grid_cap=0)
    _check(got, _cast_ref(x, KINDS[out_kind]), (in_kind, out_kind))
    if sc is not None:
        _check(sc, _scale_ref(x, W16, KINDS[out_kind]), (in_kind, out_kind, "scale"))


@gpu
@pytest.mark.parametrize("in_kind, out_kind", [("i64", "f16"), ("u8", "f16"), ("f64", "f32"), ("f32", "f16"),
                                               ("u64", "f64"), ("i16", "f32")])
def test_cast_pointers_one_element_past_a_256B_boundary(dev, in_kind, out_kind):
    x = inputs(in_kind)[:300]
    _check(_run(dev, x, KINDS[out_kind], offset=1), _cast_ref(x, KINDS[out_kind]), (in_kind, out_kind))
    if in_kind in FLOATS:
        _check(_run(dev, x, KINDS[out_kind], w=0.1, offset=1), _scale_ref(x, 0.1, KINDS[out_kind]), (in_kind, out_kind))


@gpu
def test_cast_of_nothing_touches_nothing(dev):
    for in_kind, out_kind in (("i64", "f16"), ("f32", "f64"), ("bool", "f32")):
        x = inputs(in_kind)[:0]
        assert _run(dev, x, KINDS[out_kind]).size == 0  # OK, and _run saw the whole buffer unchanged
        if in_kind in FLOATS:
            assert _run(dev, x, KINDS[out_kind], w=0.5).size == 0


# ------------------------------------------------------------------------------------------
# GPU: the same paths from the strategies
# ------------------------------------------------------------------------------------------
SHAPES = [(9, 7), (1,), (0, 3), (2049,)]  # a numel == 1 layer, an empty layer, a layer with a vector tail
_NP = {"f16": np.float16, "f32": np.float32, "f64": np.float64, "int32": np.int32, "int64": np.int64,
       "int8": np.int8, "int16": np.int16, "uint8": np.uint8, "uint16": np.uint16, "uint32": np.uint32,
       "uint64": np.uint64, "bool": np.bool_}


def _full_range(dt, shape, rng):
    """Values over the whole range of an integer kind, its extremes included."""
    dt = np.dtype(dt)
    if dt == np.bool_:
        return rng.integers(0, 2, shape).astype(np.bool_)
    n = int(np.prod(shape))
    a = rng.integers(0, 256, n * dt.itemsize, dtype=np.uint8).view(dt).copy()
    info = np.iinfo(dt)
    edge = np.array([info.min, info.max, info.min + 1, info.max - 1, 0], dt)
    pick = rng.random(n) < 0.1
    a[pick] = edge[rng.integers(0, edge.size, int(pick.sum()))]
    return a.reshape(shape)


def _layer(dt, shape, rng):
    dt = np.dtype(dt)
    if dt.kind == "f":
        return (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 3)).astype(dt)
    return _full_range(dt, shape, rng)


def _assert_same_nan_aware(got, ref):
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert isinstance(g, np.ndarray)
        assert g.dtype == r.dtype and g.shape == r.shape, (g.dtype, r.dtype, g.shape, r.shape)
        rn = np.isnan(r)
        assert np.array_equal(np.isnan(g), rn)
        assert np.array_equal(_bits(g)[~rn], _bits(r)[~rn])


def _assert_same(got, ref):
    _assert_same_nan_aware(got, ref)
    assert not any(np.isnan(r).any() for r in ref)  # nothing was compared by NaN-ness only


def _fedavg(dummy_algo_class, pus, ns):
    from substrafl_amd.schemas import FedAvgSharedState
    from substrafl_amd.strategies import FedAvg

    states = [FedAvgSharedState(n_samples=n, parameters_update=p) for n, p in zip(ns, pus)]
    return FedAvg(algo=dummy_algo_class()).avg_shared_states(shared_states=states, _skip=True).avg_parameters_update


MIXES = [("f16", "f32", "f16"), ("f16", "f64", "f16"), ("f16", "f32", "f64"), ("int32", "f32", "f32"),
         ("uint64", "f16", "int8"), ("f16", "f32", "int64", "uint8", "bool")]


@gpu
@pytest.mark.parametrize("K", [3, 9, 130])
@pytest.mark.parametrize("dts", MIXES, ids="-".join)
def test_fedavg_per_client_dtype_mix_in_one_layer(dev, dummy_algo_class, dts, K):
    """Client k carries ``dts[k % len(dts)]`` in every layer: each client's product is formed in
    its own type (``fedagg_scale_cast``), the sum in the promoted type.  K = 130 continues the
    chain across client chunks and runs a separate pairwise tree for the numel == 1 layer."""
    rng = np.random.default_rng(K * 31 + MIXES.index(dts))
    pus = [[_layer(_NP[dts[k % len(dts)]], s, rng) for s in SHAPES] for k in range(K)]
    ns = [int(v) for v in rng.integers(1, 5000, K)]
    with np.errstate(all="ignore"):
        ref = fedavg_reference_structure(pus, ns)
    _assert_same_nan_aware(_fedavg(dummy_algo_class, pus, ns), ref)


def _with_specials(a, rng):
    """30 % of a float layer replaced by the special values of ``_nonfinite_updates``
    (tests/test_gpu_parity.py): NaNs (plain, negative, quiet with a payload, signalling), +-inf,
    +-max, tiny, a subnormal, the smallest subnormal and signed zeros."""
    dt = a.dtype.type
    info = np.finfo(dt)
    bits = {2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    qpay = np.array([np.nan], dt).view(bits) | bits(5)
    spay = np.array([np.inf], dt).view(bits) | bits(3)
    nneg = qpay | (bits(1) << bits(8 * a.dtype.itemsize - 1))
    specials = np.array([np.nan, -np.nan, np.inf, -np.inf, info.max, -info.max, info.tiny, info.tiny / 4, -0.0, 0.0,
                         info.smallest_subnormal, qpay.view(dt)[0], spay.view(dt)[0], nneg.view(dt)[0]], dt)
    flat = a.reshape(-1)
    pick = rng.random(flat.size) < 0.3
    flat[pick] = specials[rng.integers(0, specials.size, int(pick.sum()))]
    return a


@gpu
def test_fedavg_dtype_mix_with_nonfinite_values(dev, dummy_algo_class):
    """The (f16, f32, f64) mix again with 30 % special values in every client, NaN-aware."""
    K, dts = 9, ("f16", "f32", "f64")
    rng = np.random.default_rng(2024)
    with np.errstate(all="ignore"):
        pus = [[_with_specials((rng.standard_normal(s) * 10.0).astype(_NP[dts[k % 3]]), rng) for s in SHAPES]
               for k in range(K)]
        ns = [int(v) for v in rng.integers(1, 5000, K)]
        ref = fedavg_reference_structure(pus, ns)
    assert any(np.isnan(r).any() for r in ref) and any(np.isinf(r).any() for r in ref)
    _assert_same_nan_aware(_fedavg(dummy_algo_class, pus, ns), ref)


@gpu
@pytest.mark.parametrize("kind", ["int8", "int16", "uint8", "uint16", "uint32", "uint64", "bool", "int64"])
def test_fedavg_whole_layer_integer_kinds(dev, dummy_algo_class, kind):
    """Integer layers promote to fp64 (``fedagg_cast``); values over the kind's whole range, so
    uint64 >= 2^63 and int64 past +-2^53 round on the device."""
    K = 11
    rng = np.random.default_rng(sorted(_NP).index(kind))
    pus = [[_full_range(_NP[kind], s, rng) for s in SHAPES] for _ in range(K)]
    if kind != "bool":
        info = np.iinfo(_NP[kind])
        pus[0][3][:2] = [info.min, info.max]
    ns = [int(v) for v in rng.integers(1, 5000, K)]
    ref = fedavg_reference_structure(pus, ns)
    assert all(r.dtype == np.float64 for r in ref)
    _assert_same(_fedavg(dummy_algo_class, pus, ns), ref)


@gpu
@pytest.mark.parametrize("K", [3, 17])
@pytest.mark.parametrize("dts", [("f16", "f16", "f16"), ("int32", "f32", "f64"), ("uint64", "bool", "int8"),
                                 ("f32", "f16", "f32")], ids="-".join)
def test_scaffold_inputs_of_other_dtypes(dev, dummy_algo_class, dts, K):
    """(delta, control-variate update, server control variate) dtypes: everything is cast to fp64
    on the device, as the reference's ``float64 weight * array`` does; outputs are fp64."""
    from substrafl_amd.schemas import ScaffoldSharedState
    from substrafl_amd.strategies import Scaffold

    rng = np.random.default_rng(K * 13 + len("".join(dts)))
    d_dt, cv_dt, c_dt = (_NP[d] for d in dts)
    pus = [[_layer(d_dt, s, rng) for s in SHAPES] for _ in range(K)]
    cvs = [[_layer(cv_dt, s, rng) for s in SHAPES] for _ in range(K)]
    c = [_layer(c_dt, s, rng) for s in SHAPES]
    ns = [int(v) for v in rng.integers(1, 5000, K)]
    states = [ScaffoldSharedState(parameters_update=pus[k], control_variate_update=cvs[k], n_samples=ns[k],
                                  server_control_variate=c) for k in range(K)]
    res = Scaffold(algo=dummy_algo_class(), aggregation_lr=0.7).avg_shared_states(shared_states=states, _skip=True)
    ref_c, ref_avg = scaffold_reference_structure(pus, cvs, c, ns, 0.7)
    assert all(r.dtype == np.float64 for r in ref_c + ref_avg)
    _assert_same(res.server_control_variate, ref_c)
    _assert_same(res.avg_parameters_update, ref_avg)


# NewtonRaphson: total = x_0 * c_0 keeps client 0's type; a wider client 1 is added in the wider
# type and the sum rounded back.  n_samples (1, 1): both coefficients are 0.5, every product is
# exact, so the rounded-back value is the rounding of a sum chosen here.
_NR_CASES = {
    # 1 + 2^-24 (tie -> 1), 1 + 3 * 2^-24 (tie -> 1 + 2^-22), just above / below a tie, f32 max + half
    # an ulp (tie -> inf) and just below it (-> max; the smallest step the wider sum still holds),
    # both signs, a tie among subnormal steps
    ("f32", "f64"): ([2.0, 2.0, 2.0, 2.0, F32_MAX, F32_MAX, -F32_MAX, 2.0**-125, 2.0],
                     [2.0**-23, 3 * 2.0**-23, 2.0**-23 + 2.0**-51, 2.0**-23 - 2.0**-51, F32_MAX + 2.0**104,
                      2.0**128 - 2.0**77, -(F32_MAX + 2.0**104), 3 * 2.0**-149, -4.0],
                     [1.0, 1 + 2.0**-22, 1 + 2.0**-23, 1.0, np.inf, F32_MAX, -np.inf, 2.0**-126 + 2.0**-148, -1.0]),
    # the same in fp16 below fp32: 1 + 2^-11 (tie -> 1), 1 + 3 * 2^-11, 65520 (-> inf), just below it (-> 65504)
    ("f16", "f32"): ([2.0, 2.0, 2.0, 2.0, 65504.0, 65504.0, -65504.0, 2.0**-14, 2.0],
                     [2.0**-10, 3 * 2.0**-10, 2.0**-10 + 2.0**-22, 2.0**-10 - 2.0**-22, 65536.0,
                      65536.0 - 2.0**-7, -65536.0, 3 * 2.0**-24, -4.0],
                     [1.0, 1 + 2.0**-9, 1 + 2.0**-10, 1.0, np.inf, 65504.0, -np.inf, 2.0**-15 + 2.0**-23, -1.0]),
}


@gpu
@pytest.mark.parametrize("pair", list(_NR_CASES), ids="-".join)
def test_sequential_sum_round_back_ties_and_overflow_edge(dev, pair):
    from substrafl_amd.engine import engine_for

    t0, t1 = (KINDS[k] for k in pair)
    x0, x1, want = _NR_CASES[pair]
    rng = np.random.default_rng(5)
    # the chosen elements, then random ones so the layer is longer than one 16-B vector
    x0 = np.concatenate([np.array(x0, t0), rng.standard_normal(300).astype(t0)])
    x1 = np.concatenate([np.array(x1, t1), rng.standard_normal(300).astype(t1)])
    assert np.isfinite(x0).all() and np.isfinite(x1).all()
    with np.errstate(all="ignore"):
        _, ref = newton_raphson_sums([[x0], [x1]], [x0.reshape(1, -1).copy(), x1.reshape(1, -1).copy()], [1, 1])
    assert ref.dtype == t0
    assert _bits(ref[:len(want)]).tolist() == _bits(np.array(want, t0)).tolist()  # the case hits what it says
    (got,) = engine_for(None).sequential_sum([[x0], [x1]], [1, 1])
    _assert_same([np.asarray(got)], [ref])
