"""ctypes binding of ``libfedagg_mxdl.so`` (the C ABI declared in ``include/fedagg_mxdl.h``): the
MXFP8 downlink.  FedAvg over MXFP8 or MXFP4 client rows with the average encoded to MXFP8 in the
same pass, and on the client the fused decode-and-increment of such an average.

Loaded lazily, by the first downlink call (``AggregationEngine.fedavg_mxfp8`` / ``fedavg_mxfp4``
with ``downlink="mxfp8"``, or ``weight_manager.increment_parameters`` handed an MXFP8 update): a
federation without ``downlink`` never touches it.  There is no fallback: a missing library raises
:class:`substrafl_amd._native.NativeLibraryError`.  ``FEDAGG_MXDL_LIB`` names another copy of the
library.
"""

from __future__ import annotations

import ctypes
from typing import Tuple

from ._loader import Library, lib_path
from ._native import P, c_int, c_u64, c_void, ptr_array

LIB_PATH = lib_path("FEDAGG_MXDL_LIB", "libfedagg_mxdl.so")

# Every symbol include/fedagg_mxdl.h declares, with its ctypes signature.
SIGNATURES = {
    "fedagg_mxdl_abi_version": (c_int, []),
    "fedagg_mxdl_last_error": (ctypes.c_char_p, []),
    "fedagg_mxdl_blocking": (c_int, [P(c_int), P(c_int), P(c_int)]),
    "fedagg_mxdl_fedavg": (c_int, [c_int, P(c_void), P(c_void), P(ctypes.c_float), c_int, c_u64, P(c_u64), c_int,
                                   c_void, c_void, c_void]),
    "fedagg_mxdl_increment": (c_int, [P(c_void), P(c_u64), c_int, c_void, c_void, c_u64, ctypes.c_double, c_void]),
    "fedagg_mxdl_decode": (c_int, [c_void, c_void, c_u64, c_void, c_void]),
}

ABI_VERSION = 1
E4M3, E2M1 = 0, 1  # FEDAGG_MXDL_E4M3, FEDAGG_MXDL_E2M1
KMAX = 128  # FEDAGG_MXDL_KMAX

_library = Library(globals(), "fedagg_mxdl_", "The MXFP8 downlink has no fallback.")
load, loaded, check = _library.load, _library.loaded, _library.check  # loaded(): only a downlink call loads it


def blocking() -> Tuple[int, int, int]:
    """``(tile_elems, lane_elems, k_group)``: the sizes at which the kernels change path."""
    t, v, g = c_int(0), c_int(0), c_int(0)
    check(load().fedagg_mxdl_blocking(ctypes.byref(t), ctypes.byref(v), ctypes.byref(g)), "mxdl_blocking")
    return t.value, v.value, g.value


def fedavg(in_kind: int, code_ptrs, scale_ptrs, weights, M: int, pairwise_idx, d_out_codes: int, d_out_scales: int,
           stream: int) -> None:
    """``fedagg_mxdl_fedavg`` over K device rows of ``in_kind`` (lists of device addresses), fp32
    ``weights``, the flat indices of the numel == 1 elements: the average's M MXFP8 code bytes to
    ``d_out_codes`` and its ``ceil(M / 32)`` scale bytes to ``d_out_scales``."""
    K = len(code_ptrs)
    w = (ctypes.c_float * max(1, K))(*[float(v) for v in weights])
    idx = [int(v) for v in (pairwise_idx if pairwise_idx is not None else [])]
    h_idx = (c_u64 * max(1, len(idx)))(*idx)
    rc = load().fedagg_mxdl_fedavg(int(in_kind), ptr_array(code_ptrs), ptr_array(scale_ptrs), w, K, int(M), h_idx,
                                   len(idx), d_out_codes, d_out_scales, stream or None)
    check(rc, "mxdl_fedavg")


def increment(layer_ptrs, numels, d_codes: int, d_scales: int, M: int, multiplier: float, stream: int) -> None:
    """``fedagg_mxdl_increment``: ``w += multiplier * decode(codes, scales)`` over the fp32 device
    tensors at ``layer_ptrs`` with ``numels`` elements each (M in all)."""
    L = len(layer_ptrs)
    n = (c_u64 * max(1, L))(*[int(v) for v in numels])
    check(load().fedagg_mxdl_increment(ptr_array(layer_ptrs), n, L, d_codes, d_scales, int(M), float(multiplier),
                                       stream or None), "mxdl_increment")


def decode(d_codes: int, d_scales: int, M: int, d_out: int, stream: int) -> None:
    """``fedagg_mxdl_decode``: the exact fp32 values of M codes under their scales, to ``d_out``."""
    check(load().fedagg_mxdl_decode(d_codes, d_scales, int(M), d_out, stream or None), "mxdl_decode")
