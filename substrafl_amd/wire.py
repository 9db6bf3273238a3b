"""Flat-bucket wire format for shared states.

The reference ships a client's update as ``List[np.ndarray]`` -- one pickled array per layer
(``torch_fed_avg_algo.py:227-230``, ``remote/serializers/pickle_serializer.py:10-18``).  Here the
layers of one update are :class:`BucketArray` views of ONE contiguous host buffer (the flat
bucket that ``weight_manager.export_numpy`` brings home with a single D2H copy, or that the
aggregation engine fetches), and they pickle as that buffer plus ``(offset, shape, dtype)``
records, so that

* the loaded update is again L views of one buffer: the aggregator stages a client with one
  host→device segment and the client applies an averaged update with one H2D copy;
* a pickle stays a pickle: plain ``pickle.load`` (the reference's ``PickleSerializer``) reads it,
  any protocol; protocol 5 writes the buffer as an in-band ``bytearray`` or, with a
  ``buffer_callback``, out of band;
* every element stays an ``np.ndarray`` of the layer's shape and dtype (the schemas check
  ``isinstance(np.ndarray)``, ``strategies/schemas.py:29``), and arithmetic on one returns a
  plain ``np.ndarray``.

Nothing here is specific to the GPU; :func:`flat_of` is how the engine and the client ops
recognise a flat row.
"""

from __future__ import annotations

import pickle
from typing import List, Optional, Sequence, Tuple

import numpy as np

_SMALL = 4096  # below this a payload is copied on load (never alias a possibly shared bytes object)

# Host representation of bfloat16 (NumPy has none): a 2-byte structured dtype holding the bit
# pattern.  NumPy refuses arithmetic and promotion on it (``a * 0.5``, ``a + a``, ``np.sum``,
# ``np.result_type(BF16, 1.0)`` raise), so code that does not know the dtype fails loudly instead
# of averaging bit patterns; it pickles with plain NumPy and stays an ``np.ndarray``.
BF16 = np.dtype([("bfloat16", "<u2")])


def is_bf16(a) -> bool:
    """Whether ``a`` (an array or a dtype) has the :data:`BF16` host dtype."""
    return getattr(a, "dtype", a) == BF16


def bf16_to_float32(a) -> np.ndarray:
    """The exact fp32 values of a :data:`BF16` array (same shape)."""
    a = np.asarray(a)
    if a.dtype != BF16:
        raise TypeError(f"bf16_to_float32: expected dtype wire.BF16, got {a.dtype}")
    return (a["bfloat16"].astype(np.uint32) << np.uint32(16)).view(np.float32)


def float32_to_bf16(a) -> np.ndarray:
    """``a`` (cast to fp32) rounded to bfloat16 as a :data:`BF16` array of the same shape: round
    to nearest even, overflow to +-inf, NaN stays NaN (quiet, payload truncated)."""
    u = np.asarray(a, dtype=np.float32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    r = np.where(nan, (u >> np.uint32(16)) | np.uint32(0x0040), r).astype(np.uint16)
    return r.view(BF16)


# ------------------------------------------------------------------------------------------
# OCP MXFP8: 1-byte ``e4m3fn`` elements, one ``e8m0`` power-of-two scale per block of 32.
#
# A quantised update is ``[layer_0 .. layer_{L-1}, scales]``: every layer an array of the layer's
# shape and dtype :data:`E4M3`, then ONE trailing 1-D :data:`E8M0` array of ``ceil(M / 32)`` scale
# bytes, M the sum of the layers' numels.  Blocks run over the concatenation of the raveled layers
# in list order with no padding between layers: block b covers flat elements
# ``[32 b, min(32 b + 32, M))`` and may span layers.
#
# Decode.  A code c has sign S, exponent field E (4 bits) and mantissa field m (3 bits):
# ``v = (-1)^S m 2^-9`` if E == 0, else ``(-1)^S (8 + m) 2^(E - 10)``; 0x7F and 0xFF are NaN and
# there is no infinity (``e4m3fn``, not ``fnuz``).  With the block's scale byte s the element is
# ``fl32(v 2^(s - 127))``; s == 255 makes the whole block NaN.  Every finite product is an fp32
# value (the smallest granule is 2^-136, an fp32 subnormal; nothing is flushed); the one inexact
# case is overflow to +-inf (448 x 2^127).
#
# Encode, per block, amax = max |x_i|: any NaN or Inf: s = 255 and every code 0x00.  amax == 0:
# s = 127 and the codes carry the zeros' signs.  Else e = floor(log2(amax)) - 8, e += 1 if
# amax 2^-e > 464 (464 is the tie that still rounds to 448, so nothing saturates), e clamped to
# [-127, 127], s = e + 127; an element is y = fl32(x 2^-e) rounded to nearest even among the
# e4m3fn values, |y| >= 448 to +-448, the sign of zero kept.
#
# Like BF16 these are structured dtypes NumPy refuses arithmetic on.
E4M3 = np.dtype([("e4m3fn", "u1")])
E8M0 = np.dtype([("e8m0", "u1")])
MX_BLOCK = 32


def is_mxfp8(parameters_update) -> bool:
    """Whether ``parameters_update`` has the MXFP8 form: :data:`E4M3` layers, then one trailing
    :data:`E8M0` array (its length is checked by :func:`mxfp8_check`)."""
    pu = list(parameters_update) if isinstance(parameters_update, (list, tuple)) else None
    return bool(pu) and len(pu) >= 2 and getattr(pu[-1], "dtype", None) == E8M0 and all(
        getattr(a, "dtype", None) == E4M3 for a in pu[:-1])


def has_mxfp8(parameters_update) -> bool:
    """Whether any array of ``parameters_update`` carries :data:`E4M3` or :data:`E8M0`."""
    return any(getattr(a, "dtype", None) in (E4M3, E8M0) for a in parameters_update)


def mxfp8_check(parameters_update) -> int:
    """M of an MXFP8 update; ``ValueError`` when the scale array is missing, is not the one
    trailing 1-D :data:`E8M0` array, or does not hold ``ceil(M / 32)`` bytes."""
    pu = list(parameters_update)
    if not pu or getattr(pu[-1], "dtype", None) != E8M0:
        raise ValueError("MXFP8 update: the trailing wire.E8M0 scale array is missing")
    layers = pu[:-1]
    if not layers or any(getattr(a, "dtype", None) != E4M3 for a in layers):
        raise ValueError("MXFP8 update: every layer before the scale array must have dtype wire.E4M3")
    M = sum(int(np.asarray(a).size) for a in layers)
    s = np.asarray(pu[-1])
    if s.ndim != 1 or s.size != -(-M // MX_BLOCK):
        raise ValueError(f"MXFP8 update: {M} elements need a 1-D scale array of {-(-M // MX_BLOCK)} bytes, "
                         f"got shape {s.shape}")
    return M


def _e4m3_round(y: np.ndarray) -> np.ndarray:
    """fp32 ``y`` (finite) to e4m3fn codes: nearest even, |y| >= 448 to +-448, signed zeros."""
    u = np.ascontiguousarray(y, np.float32).view(np.uint32)
    a = u & np.uint32(0x7FFFFFFF)
    # below 2^-6 the e4m3fn values are the multiples of 2^-9: |y| + 2^14 rounds there (fp32 ulp 2^-9)
    with np.errstate(all="ignore"):
        sub = (a.view(np.float32) + np.float32(16384.0)).view(np.uint32) - np.uint32(0x46800000)
    a_n = np.minimum(a, np.uint32(0x43E00000))  # 448: keeps the shifts below in range
    nrm = (a_n + np.uint32(0x7FFFF) + ((a_n >> np.uint32(20)) & np.uint32(1)) - np.uint32(0x3C000000)) >> np.uint32(20)
    code = np.where(a < np.uint32(0x3C800000), sub, nrm)
    code = np.where(a >= np.uint32(0x43E00000), np.uint32(0x7E), code)
    return (code | ((u >> np.uint32(24)) & np.uint32(0x80))).astype(np.uint8)


def _mx_encode_flat(x: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    M = x.size
    nb = -(-M // MX_BLOCK)
    pad = np.zeros(nb * MX_BLOCK, np.float32)
    pad[:M] = x
    pad = pad.reshape(nb, MX_BLOCK)
    a = (pad.view(np.uint32) & np.uint32(0x7FFFFFFF)).max(axis=1) if nb else np.zeros(0, np.uint32)
    bad = a >= np.uint32(0x7F800000)
    zero = a == 0
    amax = a.view(np.float32).astype(np.float64)
    amax[bad | zero] = 1.0
    e = np.frexp(amax)[1].astype(np.int64) - 9  # floor(log2(amax)) - 8
    e += np.ldexp(amax, -e) > 464.0
    e = np.clip(e, -127, 127)
    e[bad | zero] = 0
    s = (e + 127).astype(np.uint8)
    s[bad] = 255
    inv = np.ldexp(1.0, -e).astype(np.float32)  # 2^-e, exact (2^-127 is an fp32 subnormal)
    with np.errstate(all="ignore"):
        y = pad * inv[:, None]
    codes = _e4m3_round(y)
    codes[bad, :] = 0
    return codes.reshape(-1)[:M].copy(), s


def float32_to_mxfp8(x):
    """``x`` (an array, or a list of layers; cast to fp32) encoded by the rule above:
    ``(codes, scales)`` with ``codes`` of dtype :data:`E4M3` shaped like ``x`` (a list of such
    arrays for a list) and ``scales`` the 1-D :data:`E8M0` array over the raveled concatenation."""
    many = isinstance(x, (list, tuple))
    arrs = [np.asarray(a, dtype=np.float32) for a in (x if many else [x])]
    flat = np.concatenate([a.reshape(-1) for a in arrs]) if arrs else np.zeros(0, np.float32)
    codes, s = _mx_encode_flat(flat)
    out, off = [], 0
    for a in arrs:
        out.append(codes[off : off + a.size].reshape(a.shape).view(E4M3))
        off += a.size
    return (out if many else out[0]), s.view(E8M0)


def mxfp8_to_float32(codes, scales):
    """The exact fp32 values of MXFP8 ``codes`` (an :data:`E4M3` array, or a list of layers) under
    the :data:`E8M0` ``scales`` of their raveled concatenation; the shape(s) of ``codes``."""
    many = isinstance(codes, (list, tuple))
    arrs = [np.asarray(a) for a in (codes if many else [codes])]
    scales = np.asarray(scales)
    if any(a.dtype != E4M3 for a in arrs) or scales.dtype != E8M0:
        raise TypeError("mxfp8_to_float32: expected wire.E4M3 codes and wire.E8M0 scales")
    c = np.concatenate([a["e4m3fn"].reshape(-1) for a in arrs]) if arrs else np.zeros(0, np.uint8)
    s = scales["e8m0"].reshape(-1)
    M = c.size
    if s.size != -(-M // MX_BLOCK):
        raise ValueError(f"mxfp8_to_float32: {M} elements need {-(-M // MX_BLOCK)} scale bytes, got {s.size}")
    E = ((c >> 3) & 15).astype(np.int64)
    m = (c & 7).astype(np.float64)
    mag = np.where(E == 0, m * 2.0 ** -9, np.ldexp(8.0 + m, E - 10))
    mag[(c & 0x7F) == 0x7F] = np.nan
    sc = np.ldexp(1.0, s.astype(np.int64) - 127)
    sc[s == 255] = np.nan
    with np.errstate(all="ignore"):
        v = np.copysign(mag * np.repeat(sc, MX_BLOCK)[:M], np.where(c & 0x80, -1.0, 1.0)).astype(np.float32)
    out, off = [], 0
    for a in arrs:
        out.append(v[off : off + a.size].reshape(a.shape))
        off += a.size
    return out if many else out[0]


class _Bucket:
    """Owner of one flat byte buffer (1-D uint8, C-contiguous, writable)."""

    __slots__ = ("flat", "__weakref__")

    def __init__(self, flat: np.ndarray):
        if flat.dtype != np.uint8 or flat.ndim != 1 or not flat.flags.c_contiguous:
            raise ValueError("a bucket is a 1-D contiguous uint8 buffer")
        self.flat = flat

    def __reduce_ex__(self, protocol):
        if protocol >= 5 and self.flat.flags.writeable:
            return _bucket_from_buffer, (pickle.PickleBuffer(self.flat),)
        return _bucket_from_buffer, (self.flat.tobytes(),)


def _bucket_from_buffer(buf) -> _Bucket:
    """Unpickle: a writable uint8 array over ``buf`` without a copy where that is safe."""
    if isinstance(buf, bytes):
        if len(buf) < _SMALL:
            return _Bucket(np.frombuffer(bytearray(buf), dtype=np.uint8))
        # NumPy's own protocol-4 path: a writable array owning the unpickled bytes object.
        a = np.ndarray.__new__(np.ndarray, (0,), np.uint8)
        a.__setstate__((1, (len(buf),), np.dtype(np.uint8), False, buf))
        return _Bucket(a)
    a = np.frombuffer(buf, dtype=np.uint8)
    if not a.flags.writeable:
        a = a.copy()
    return _Bucket(a)


class BucketArray(np.ndarray):
    """One layer of a flat bucket: a plain ``np.ndarray`` view that pickles by reference to the
    bucket.  Slices and arithmetic results are ordinary arrays (``__array_finalize__`` and
    ``__array_ufunc__`` drop the bucket link)."""

    _bucket: Optional[_Bucket] = None
    _offset: int = 0

    def __array_finalize__(self, obj):
        self._bucket = None
        self._offset = 0

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        inputs = tuple(x.view(np.ndarray) if isinstance(x, BucketArray) else x for x in inputs)
        out = kwargs.get("out")
        if out:
            kwargs["out"] = tuple(x.view(np.ndarray) if isinstance(x, BucketArray) else x for x in out)
        return getattr(ufunc, method)(*inputs, **kwargs)

    def __reduce_ex__(self, protocol):
        if self._bucket is None:
            return self.view(np.ndarray).__reduce_ex__(protocol)
        # a structured dtype's ``str`` is "|V2" and loses its field (wire.BF16): those carry ``descr``
        dt = self.dtype.str if self.dtype.names is None else self.dtype.descr
        return _layer, (self._bucket, self._offset, self.shape, dt)

    def __reduce__(self):
        return self.__reduce_ex__(2)


def _layer(bucket: _Bucket, offset: int, shape: Tuple[int, ...], dtype) -> BucketArray:
    dt = np.dtype([tuple(f) for f in dtype] if isinstance(dtype, list) else dtype)
    n = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
    return _member(bucket, offset, dt, n, tuple(shape))


def _member(bucket: _Bucket, offset: int, dt: np.dtype, n: int, shape) -> BucketArray:
    raw = bucket.flat[offset : offset + n * dt.itemsize]
    v = raw.view(dt).reshape(shape).view(BucketArray)
    v._bucket = bucket
    v._offset = offset
    return v


def bucket_views(flat: np.ndarray, shapes: Sequence[Tuple[int, ...]], dtypes=None) -> List[BucketArray]:
    """Per-layer :class:`BucketArray` views of ``flat`` (layers back to back, in order)."""
    flat = np.ascontiguousarray(flat).reshape(-1)
    base_dt = flat.dtype
    bucket = _Bucket(flat.view(np.uint8))
    out, off = [], 0
    for i, shp in enumerate(shapes):
        dt = np.dtype(dtypes[i]) if dtypes is not None else base_dt
        n = int(np.prod(shp, dtype=np.int64)) if len(shp) else 1
        if off % dt.itemsize:
            raise ValueError("layer offsets must be aligned to the layer's item size")
        out.append(_member(bucket, off, dt, n, tuple(shp)))
        off += n * dt.itemsize
    if off > bucket.flat.nbytes:
        raise ValueError("the layers do not fit in the buffer")
    return out


def pack(arrays: Sequence[np.ndarray]) -> List[BucketArray]:
    """Copy ``arrays`` (any dtypes) into one new flat bucket, each layer aligned to its item size
    (layers of one dtype are therefore back to back, like an engine bucket row)."""
    shapes = [np.shape(a) for a in arrays]
    dtypes = [np.asarray(a).dtype for a in arrays]
    offs, off = [], 0
    for a, dt in zip(arrays, dtypes):
        off = -(-off // dt.itemsize) * dt.itemsize
        offs.append(off)
        off += np.asarray(a).nbytes
    flat = np.empty(off, dtype=np.uint8)  # NumPy allocations are at least 16-B aligned
    bucket = _Bucket(flat)
    out = []
    for a, shp, dt, o in zip(arrays, shapes, dtypes, offs):
        n = int(np.prod(shp, dtype=np.int64)) if len(shp) else 1
        v = _member(bucket, o, dt, n, tuple(shp))
        np.copyto(v.view(np.ndarray), np.asarray(a), casting="no")
        out.append(v)
    return out


def flat_of(arrays: Sequence[np.ndarray]) -> Optional[np.ndarray]:
    """If ``arrays`` are consecutive layers of one bucket, all of one dtype, with no gaps, the 1-D
    array of that dtype spanning exactly them; else None."""
    if not arrays or not all(isinstance(a, BucketArray) and a._bucket is not None for a in arrays):
        return None
    b = arrays[0]._bucket
    dt = arrays[0].dtype
    off = arrays[0]._offset
    start = off
    for a in arrays:
        if a._bucket is not b or a.dtype != dt or a._offset != off:
            return None
        off += a.nbytes
    if start % dt.itemsize:
        return None
    return b.flat[start:off].view(dt)
