"""Client-side bucket producer / consumer with flat-bucket HIP paths.

Same functions, signatures and results as the reference's
``substrafl/algorithms/pytorch/weight_manager.py`` (``model_parameters`` :53-76, ``get_parameters``
:79-100, ``increment_parameters`` :103-137, ``subtract_parameters`` :140-158, ``add_parameters``
:161-179, ``weighted_sum_parameters`` :182-212, ``set_parameters`` :215-238,
``zeros_like_parameters`` :241-265), so an algorithm can switch its import.  When every tensor is
fp32 (or every tensor fp16, or bf16) on a ROCm device the per-layer torch loops become single
launches of libfedagg's flat-bucket kernels, and the tensors they return are views of ONE flat device bucket -- which
:func:`export_numpy` brings home with a single D2H copy (the wire format the aggregator stages
with one contiguous segment per client).  Other dtypes and CPU tensors keep the reference's torch
semantics (they are the client's own device choice, not the aggregation hot path).

Bit-exact with the reference's torch ops: ``weighted_sum_parameters`` is Python ``sum()`` from int 0
over ``param * coeff`` (so ``-0.0`` becomes ``+0.0``, and ``coeff`` is rounded to fp32 as torch does
for a Python scalar); ``increment_parameters`` is ``w += fl32(multiplier) * u``.  On fp16 / bf16
tensors torch computes each op in fp32 and rounds its result once to the tensor's type; a bf16
model takes an fp32 update (the aggregator's average of ``wire.BF16`` buckets) with the add in the
promoted fp32, as torch on ROCm performs it on the reference's per-layer tensors (the update
rounded to bf16 first in each full 16384-element block of a layer; include/fedagg.h states the rules).

A 16-bit model next to fp64 operands -- a Scaffold client from round 2 on, once the aggregator's
fp64 ``avg_parameters_update`` and ``server_control_variate`` have come back -- follows torch's
type promotion on ``libfedagg_promote.so`` (include/fedagg_promote.h states the rules):
``increment_parameters`` of 16-bit parameters by an fp64 update is one
``fedagg_promote_increment`` launch, ``weighted_sum_parameters`` over lists that are each the
model's 16-bit kind or fp64 (at least one of each) one ``fedagg_promote_wsum`` launch into a
fresh fp64 bucket, bit for bit what torch on the device gives for the reference's per-layer
tensors (an fp16 layer's trailing ``numel mod 2048`` elements included, where torch rounds the
product once).  ``FEDAGG_FLAT_PROMOTE=0`` keeps those operand sets on the torch loops.
"""

from __future__ import annotations

import ctypes
from typing import Generator, List, Optional, Sequence

import numpy as np
import torch
from torch._utils import _unflatten_dense_tensors

from .. import _native, _native_promote
from ..wire import BF16, bucket_views, flat_of

_BN = (
    torch.nn.BatchNorm1d,
    torch.nn.BatchNorm2d,
    torch.nn.BatchNorm3d,
    torch.nn.LazyBatchNorm1d,
    torch.nn.LazyBatchNorm2d,
    torch.nn.LazyBatchNorm3d,
)


def is_batchnorm_layer(layer: torch.nn.Module) -> bool:
    return isinstance(layer, _BN)


def batch_norm_param(model: torch.nn.Module) -> Generator[torch.Tensor, None, None]:
    for _, module in model.named_modules():
        if is_batchnorm_layer(module):
            yield module.running_mean
            yield module.running_var


def model_parameters(model: torch.nn.Module, with_batch_norm_parameters: bool):
    """Generator factory: ``model.parameters()`` then (optionally) every BatchNorm layer's running
    mean and variance -- the bucket layer order (weight_manager.py:53-76)."""

    def my_iterator():
        for p in model.parameters():
            yield p
        if with_batch_norm_parameters:
            for p in batch_norm_param(model):
                yield p

    return my_iterator


# ----------------------------------------------------------------------------------------
# flat-bucket helpers
# ----------------------------------------------------------------------------------------
_KIND = {torch.float32: _native.FEDAGG_F32, torch.float64: _native.FEDAGG_F64,
         torch.float16: _native.FEDAGG_F16, torch.bfloat16: _native.FEDAGG_BF16}
_KIND16 = (_native.FEDAGG_F16, _native.FEDAGG_BF16)
# (parameter kind, update kind) pairs of the 16-bit increment (fedagg_flat_increment_kind): a
# 16-bit model takes an update of its own kind, a bf16 model also the engine's fp32 average
_INC16 = {(_native.FEDAGG_F16, _native.FEDAGG_F16), (_native.FEDAGG_BF16, _native.FEDAGG_BF16),
          (_native.FEDAGG_BF16, _native.FEDAGG_F32)}
# host dtypes staged as raw bytes into a device bucket of the torch dtype
_HOST_DTYPE = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
               np.dtype(np.float16): torch.float16, BF16: torch.bfloat16}


def _kind(tensors: Sequence[torch.Tensor], device=None) -> Optional[int]:
    """The libfedagg kind when ``tensors`` are contiguous ROCm tensors of ONE dtype (fp32, fp64,
    fp16 or bf16) on one device (``device`` if given); else None (the op keeps the reference's torch loop)."""
    if not tensors:
        return None
    t0 = tensors[0]
    if not (t0.is_cuda and t0.dtype in _KIND):
        return None
    if device is None:
        idx = t0.get_device()
    else:
        d = torch.device(device)
        if d.type != "cuda":
            return None
        idx = d.index if d.index is not None else torch.cuda.current_device()
    dt = t0.dtype
    for t in tensors:  # get_device() is -1 on the CPU: one int compare covers device and placement
        if t.dtype != dt or t.get_device() != idx or not t.is_contiguous():
            return None
    return _KIND[dt]


def _numel_array(tensors):
    return (ctypes.c_uint64 * max(1, len(tensors)))(*[t.numel() for t in tensors])


def _views(flat: torch.Tensor, like: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    """Per-layer views of ``flat`` shaped like ``like`` (one C++ call: per-layer ``narrow().view()``
    from Python cost ≈10 µs a layer, more than the flat kernels themselves on a 300-layer model)."""
    return list(_unflatten_dense_tensors(flat, list(like)))


def _stream(device) -> int:
    return int(torch.cuda.current_stream(device).cuda_stream)


def flat_bucket(tensors: Sequence[torch.Tensor]) -> Optional[torch.Tensor]:
    """The flat 1-D tensor the given tensors are consecutive views of, else None."""
    if not tensors:
        return None
    base = tensors[0]
    if not base.is_contiguous():
        return None
    storage = base.untyped_storage().data_ptr()
    start = base.storage_offset()
    off = start
    for t in tensors:
        if (t.untyped_storage().data_ptr() != storage or t.storage_offset() != off or not t.is_contiguous()
                or t.dtype != base.dtype):
            return None
        off += t.numel()
    total = off - start
    return torch.as_strided(base, (total,), (1,), start)


def _gather_flat(tensors: Sequence[torch.Tensor]) -> torch.Tensor:
    kind = _kind(tensors)
    flat = torch.empty(sum(t.numel() for t in tensors), dtype=tensors[0].dtype, device=tensors[0].device)
    lib = _native.load()
    _native.check(lib.fedagg_flat_gather(_native.ptr_array([t.data_ptr() for t in tensors]), kind,
                                         _numel_array(tensors), len(tensors), flat.data_ptr(),
                                         _stream(flat.device)), "flat_gather")
    return flat


# ----------------------------------------------------------------------------------------
# reference API
# ----------------------------------------------------------------------------------------
def get_parameters(model: torch.nn.Module, with_batch_norm_parameters: bool) -> List[torch.Tensor]:
    """Copies of the model parameters (weight_manager.py:79-100); on a ROCm device one gather
    launch into one flat bucket, returned as per-layer views."""
    with torch.no_grad():
        params = list(model_parameters(model, with_batch_norm_parameters=with_batch_norm_parameters)())
        if _kind(params) is not None:
            return _views(_gather_flat(params), params)
        return [p.clone() for p in params]


def increment_parameters(
    model: torch.nn.Module,
    updates: List,
    *,
    with_batch_norm_parameters: bool,
    updates_multiplier: float = 1.0,
):
    """``w += updates_multiplier * u`` for every model parameter (weight_manager.py:103-137)."""
    with torch.no_grad():
        params = list(model_parameters(model=model, with_batch_norm_parameters=with_batch_norm_parameters)())
        assert len(params) == len(updates), "Length of model parameters and updates are unequal."
        for w, u in zip(params, updates):
            assert tuple(u.shape) == tuple(w.data.shape), (
                f"The shape of the model weights ({w.data.shape}) and of the update ({u.shape}) "
                "passed in the updates argument are unequal."
            )
        pkind = _kind([p.data for p in params])
        if pkind in _KIND16:
            flat = _device_flat(updates, params[0].device)
            if flat is not None and (pkind, _KIND[flat.dtype]) in _INC16:
                lib = _native.load()
                _native.check(lib.fedagg_flat_increment_kind(_native.ptr_array([p.data.data_ptr() for p in params]),
                                                             pkind, _numel_array(params), len(params),
                                                             flat.data_ptr(), _KIND[flat.dtype],
                                                             float(updates_multiplier), _stream(flat.device)),
                              "flat_increment_kind")
                return
            if flat is not None and flat.dtype == torch.float64 and _native_promote.enabled():
                # torch's promotion: the sum in fp64, back to the parameters' kind through float
                lib = _native_promote.load()
                _native_promote.check(lib.fedagg_promote_increment(
                    _native.ptr_array([p.data.data_ptr() for p in params]), pkind, _numel_array(params), len(params),
                    flat.data_ptr(), float(updates_multiplier), _stream(flat.device)), "flat_promote_increment")
                return
        elif pkind == _native.FEDAGG_F32:
            flat = _device_flat(updates, params[0].device)
            if flat is not None and flat.dtype in (torch.float32, torch.float64):
                lib = _native.load()
                _native.check(lib.fedagg_flat_increment(_native.ptr_array([p.data.data_ptr() for p in params]),
                                                        _numel_array(params), len(params), flat.data_ptr(),
                                                        _KIND[flat.dtype], float(updates_multiplier),
                                                        _stream(flat.device)), "flat_increment")
                return
        for w, u in zip(params, updates):
            if isinstance(u, np.ndarray):
                u = (torch.from_numpy(u.view(np.int16)).view(torch.bfloat16) if u.dtype == BF16
                     else torch.from_numpy(u)).to(w.device)
            w.data += updates_multiplier * u.data


def _device_flat(updates, device) -> Optional[torch.Tensor]:
    """One device bucket (fp32, fp64, fp16 or bf16) holding ``updates`` back to back, None if they
    are not all of one of those dtypes (host layers: float32 / float64 / float16 / ``wire.BF16``)."""
    if all(isinstance(u, torch.Tensor) for u in updates):
        if _kind(updates, device) is None:
            return None
        flat = flat_bucket(updates)
        return flat if flat is not None else _gather_flat(updates)
    if all(isinstance(u, np.ndarray) for u in updates) and updates[0].dtype in _HOST_DTYPE and all(
            u.dtype == updates[0].dtype for u in updates):
        return _stage_host_layers(updates, torch.device(device))
    return None


def _stage_host_layers(arrays: Sequence[np.ndarray], device) -> torch.Tensor:
    """Host layers (one dtype) -> ONE flat device bucket through the native session's pinned ring:
    the layers are packed chunk by chunk into pinned memory by its workers while earlier chunks
    are on the PCIe link (``fedagg_session_stage``, one row of L segments) -- no host-side
    concatenation, no pageable copy.  Wherever the layers live: one unpickled array each (the
    subprocess / docker task inputs), or views of one aggregator output (simulation)."""
    from .. import runtime

    from .. import handoff

    idx = device.index if device.index is not None else torch.cuda.current_device()
    layers = [np.ascontiguousarray(a) for a in arrays]
    n = sum(int(a.size) for a in layers)
    dt = _HOST_DTYPE[layers[0].dtype]  # the caller checked; 16-bit layers travel as their raw bytes
    flat = torch.empty(n, dtype=dt, device=torch.device("cuda", idx))
    if n:
        # the bucket may reuse memory torch's stream still reads: the copy starts after that stream
        torch.cuda.current_stream(flat.device).synchronize()
        with runtime.device_lock(idx):  # the session's ring is shared with the aggregation engine
            s = runtime.session(idx)
            # simulation mode: an aggregator output (or another client's export) still on this GPU
            # is copied device to device (handoff.py); otherwise staged through the pinned ring
            hit = handoff.lookup(list(arrays), idx)
            if hit is not None and hit[1] == n * flat.element_size():
                s.copy_d2d(flat.data_ptr(), hit[0], hit[1])
            else:
                s.stage(flat.data_ptr(), n * flat.element_size(), [layers])
            s.sync()
    return flat


def _host_flat(arrays: Sequence[np.ndarray]) -> Optional[np.ndarray]:
    """The 1-D array the given arrays are consecutive views of (the aggregator returns exactly
    that: per-layer views of one owned array), else None."""
    base = arrays[0].base if arrays[0].base is not None else arrays[0]
    if not isinstance(base, np.ndarray) or base.ndim != 1 or not base.flags.c_contiguous:
        return None
    start = arrays[0].__array_interface__["data"][0]
    b0 = base.__array_interface__["data"][0]
    off = start
    for a in arrays:
        if (a.base is not base and a is not base) or a.__array_interface__["data"][0] != off or not a.flags.c_contiguous:
            return None
        off += a.nbytes
    first = (start - b0) // base.itemsize
    return base[first : first + (off - start) // base.itemsize]


def weighted_sum_parameters(parameters_list: List[List[torch.Tensor]], coefficient_list: List[float]) -> List[torch.Tensor]:
    """``sum(param * coeff ...)`` per layer (weight_manager.py:182-212); fused into one launch."""
    assert all(
        len(parameters_list[0]) == len(parameters) for parameters in parameters_list
    ), "The number of parameters in each List is not the same"
    assert len(parameters_list) == len(coefficient_list), "There must be a coefficient for each List of parameters"
    for parameters_to_sum in zip(*parameters_list):
        assert all(
            parameters_to_sum[0].data.shape == parameter.data.shape for parameter in parameters_to_sum
        ), "The shape of the parameters are unequal."
    kinds = [_kind(lst, parameters_list[0][0].device if parameters_list[0] else None) for lst in parameters_list]
    # a 16-bit list next to a list of another kind follows torch's promotion: the promoted ops below, or torch
    if 1 <= len(parameters_list) <= _native.FEDAGG_FLAT_MAX_LISTS and all(k is not None for k in kinds) and (
            not any(k in _KIND16 for k in kinds) or len(set(kinds)) == 1):
        like = parameters_list[0]
        if kinds[0] in _KIND16:
            out_dtype = like[0].dtype
        else:
            out_dtype = torch.float64 if _native.FEDAGG_F64 in kinds else torch.float32
        with torch.no_grad():
            out = torch.empty(sum(t.numel() for t in like), dtype=out_dtype, device=like[0].device)
            lib = _native.load()
            coeffs = (ctypes.c_double * len(coefficient_list))(*[float(c) for c in coefficient_list])
            _native.check(lib.fedagg_flat_wsum(_native.ptr_array([t.data_ptr() for lst in parameters_list for t in lst]),
                                               (ctypes.c_int * len(kinds))(*kinds), len(parameters_list), coeffs,
                                               _numel_array(like), len(like), out.data_ptr(), _KIND[out_dtype],
                                               _stream(out.device)), "flat_wsum")
        return _views(out, like)
    # lists that are each ONE 16-bit kind or fp64, at least one of each: torch's promotion, result fp64
    if (1 <= len(parameters_list) <= _native.FEDAGG_FLAT_MAX_LISTS and all(k is not None for k in kinds)
            and _native.FEDAGG_F64 in kinds and len(set(kinds) - {_native.FEDAGG_F64}) == 1
            and (set(kinds) & set(_KIND16)) and _native_promote.enabled()):
        like = parameters_list[0]
        with torch.no_grad():
            out = torch.empty(sum(t.numel() for t in like), dtype=torch.float64, device=like[0].device)
            lib = _native_promote.load()
            coeffs = (ctypes.c_double * len(coefficient_list))(*[float(c) for c in coefficient_list])
            _native_promote.check(lib.fedagg_promote_wsum(
                _native.ptr_array([t.data_ptr() for lst in parameters_list for t in lst]),
                (ctypes.c_int * len(kinds))(*kinds), len(parameters_list), coeffs, _numel_array(like), len(like),
                out.data_ptr(), _stream(out.device)), "flat_promote_wsum")
        return _views(out, like)
    weighted_sum = []
    for parameters_to_sum in zip(*parameters_list):
        with torch.no_grad():
            weighted_sum.append(sum(param * coeff for param, coeff in zip(parameters_to_sum, coefficient_list)))
    return weighted_sum


def subtract_parameters(parameters: List[torch.Tensor], parameters_to_subtract: List[torch.Tensor]) -> List[torch.Tensor]:
    return weighted_sum_parameters(parameters_list=[parameters, parameters_to_subtract], coefficient_list=[1, -1])


def add_parameters(parameters: List[torch.Tensor], parameters_to_add: List[torch.Tensor]) -> List[torch.Tensor]:
    return weighted_sum_parameters(parameters_list=[parameters, parameters_to_add], coefficient_list=[1, 1])


def set_parameters(model: torch.nn.Module, parameters: List[torch.Tensor], with_batch_norm_parameters: bool):
    """Rebind every model parameter's data to the given tensors (weight_manager.py:215-238)."""
    with torch.no_grad():
        iter_params = model_parameters(model, with_batch_norm_parameters=with_batch_norm_parameters)
        n_parameters = len(list(iter_params()))
        assert n_parameters == len(parameters), "Length of model parameters and provided parameters are unequal."
        for p, w in zip(iter_params(), parameters):
            p.data = w.data


def zeros_like_parameters(model: torch.nn.Module, with_batch_norm_parameters: bool, device: torch.device):
    with torch.no_grad():
        params = list(model_parameters(model, with_batch_norm_parameters=with_batch_norm_parameters)())
        # one flat bucket for a single-dtype model of a kind the flat ops know (fp16 and bf16 models
        # too: Scaffold's round-1 control variates then export as one 2-byte bucket)
        if params and torch.device(device).type == "cuda" and params[0].dtype in _KIND and all(
                p.dtype == params[0].dtype for p in params):
            flat = torch.zeros(sum(p.numel() for p in params), dtype=params[0].dtype, device=device)
            return _views(flat, params)
        return [torch.zeros_like(p).to(device) for p in params]


def _host_array(t: torch.Tensor) -> np.ndarray:
    """``t.cpu().detach().numpy()``; a bf16 tensor comes home as ``wire.BF16`` (its bit patterns),
    any other dtype NumPy lacks raises as the reference's ``.numpy()`` does."""
    t = t.cpu().detach()
    if t.dtype == torch.bfloat16:
        return t.contiguous().view(torch.int16).numpy().view(BF16)
    return t.numpy()


def export_mxfp8(tensors: Sequence[torch.Tensor], tag: str = "export") -> List[np.ndarray]:
    """The MXFP8 form of ``tensors`` (``wire.py``: L ``wire.E4M3`` layers, then one ``wire.E8M0``
    scale array over the raveled concatenation), quantised on the device by
    ``fedagg_mx_quantize`` from the flat fp32 or bf16 bucket.  Codes and scales share one device
    buffer (the scales right behind the codes), so they leave in ONE D2H copy into one host
    buffer, and the layers returned are :class:`wire.BucketArray` views of it: they pickle as that
    one buffer.  Anything but fp32 or bf16 tensors on a ROCm device is refused
    (``NotImplementedError``): there is no host quantiser behind this and the fp32 average could
    not go back onto an fp16 or fp64 model through the flat kernels."""
    from .. import _native_mx, runtime
    from ..wire import E4M3, E8M0, MX_BLOCK

    tensors = list(tensors)
    kind = _kind(tensors)
    if kind not in (_native.FEDAGG_F32, _native.FEDAGG_BF16):
        dts = sorted({str(t.dtype) for t in tensors})
        raise NotImplementedError(f"wire='mxfp8': the update of an fp32 or bf16 model on a ROCm device is quantised, "
                                  f"got {dts} on {sorted({str(t.device) for t in tensors})}")
    flat = flat_bucket(tensors)
    if flat is None:
        flat = _gather_flat(tensors)
    M = flat.numel()
    n_scales = -(-M // MX_BLOCK)
    dev = torch.empty(M + n_scales, dtype=torch.uint8, device=flat.device)
    _native_mx.quantize(flat.data_ptr(), kind, M, dev.data_ptr(), dev.data_ptr() + M, _stream(flat.device))
    host = runtime.reusable_host_array(M + n_scales, np.dtype(np.uint8), tag)
    torch.cuda.current_stream(flat.device).synchronize()  # the quantiser ran on torch's stream
    with runtime.device_lock(flat.device.index):  # the session's ring is shared with the engine
        runtime.session(flat.device.index).fetch(dev.data_ptr(), host)
    shapes = [tuple(t.shape) for t in tensors]
    return bucket_views(host, shapes + [(n_scales,)], [E4M3] * len(shapes) + [E8M0])


def export_numpy(tensors: Sequence[torch.Tensor], wire: bool = True, tag: str = "export") -> List[np.ndarray]:
    """``[p.cpu().detach().numpy() for p in ...]`` (torch_fed_avg_algo.py:227-230) with ONE D2H copy
    when the tensors are views of one flat bucket.  With ``wire`` the arrays returned are
    :class:`wire.BucketArray` layers of one host buffer -- they pickle as that one buffer, and the
    aggregator stages the client as a single segment; without it they are plain ``np.ndarray``
    views of that buffer, which any process unpickles (no ``substrafl_amd`` import needed).
    ``tag`` names the host buffer recycled across calls (``runtime.reusable_host_array``): exports
    that are alive together (Scaffold's three lists) need one tag each, or every round after the
    first re-faults a fresh buffer for all but one of them."""
    flat = flat_bucket(list(tensors))
    if flat is None or not flat.is_cuda:
        return [_host_array(t) for t in tensors]
    from .. import handoff, runtime

    # one D2H through the native session's pinned ring (chunked, copied out by its worker pool)
    # a bf16 bucket comes home as wire.BF16 (its bit patterns); any other dtype NumPy lacks raises, as .numpy()
    host_dt = BF16 if flat.dtype == torch.bfloat16 else torch.empty(0, dtype=flat.dtype).numpy().dtype
    host = runtime.reusable_host_array(flat.numel(), host_dt, tag)
    torch.cuda.current_stream(flat.device).synchronize()  # the bucket was written on torch's stream
    with runtime.device_lock(flat.device.index):  # the session's ring is shared with the engine
        runtime.session(flat.device.index).fetch(flat.data_ptr(), host)
    if flat.element_size() != 2:  # 16-bit exports are not handed off: the aggregator stages them from the host
        handoff.record_tensor(host, flat)  # simulation mode (opt-in): freezes host, keeps flat for the aggregator
    shapes = [tuple(t.shape) for t in tensors]
    if wire:
        return bucket_views(host, shapes)
    out, off = [], 0
    for shp in shapes:
        n = int(np.prod(shp, dtype=np.int64)) if len(shp) else 1
        out.append(host[off : off + n].reshape(shp))
        off += n
    return out


def to_device(arrays: Sequence[np.ndarray], device) -> List[torch.Tensor]:
    """``[torch.from_numpy(x).to(device) for x in arrays]`` (torch_scaffold_algo.py:397,404-406):
    on a ROCm device, when the arrays share one fp32 or fp64 dtype, ONE host->device copy into a
    flat bucket, returned as per-layer views (so the flat kernels take the bucket as is)."""
    arrays = list(arrays)
    d = torch.device(device)
    if d.type == "cuda" and arrays and all(isinstance(a, np.ndarray) and a.dtype in (np.float32, np.float64)
                                           for a in arrays):
        flat = _device_flat(arrays, d)
        if flat is not None:
            shapes = [a.shape for a in arrays]
            return [v.view(s) for v, s in zip(torch.split(flat, [int(np.prod(s, dtype=np.int64)) for s in shapes]),
                                               shapes)]
    return [torch.from_numpy(x).to(d) for x in arrays]

