"""ctypes binding of ``libfedagg_mx4.so`` (the C ABI declared in ``include/fedagg_mx4.h``): FedAvg
over OCP MXFP4 client updates (4-bit ``e2m1`` codes, two to a byte, one ``e8m0`` scale byte per 32
elements) and the device quantiser that produces them, with or without error feedback.

Loaded lazily, by the first MXFP4 call (``AggregationEngine.fedavg_mxfp4``, or the export of an
``accelerate_algo(..., wire="mxfp4")`` client): importing ``substrafl_amd`` and every other
federation, the MXFP8 wire included, never touch it.  There is no fallback: a missing library raises
:class:`substrafl_amd._native.NativeLibraryError`.  ``FEDAGG_MX4_LIB`` names another copy of the
library.
"""

from __future__ import annotations

import ctypes
from typing import Tuple

from ._loader import Library, lib_path
from ._native import P, c_int, c_u64, c_void, ptr_array

LIB_PATH = lib_path("FEDAGG_MX4_LIB", "libfedagg_mx4.so")

# Every symbol include/fedagg_mx4.h declares, with its ctypes signature.
SIGNATURES = {
    "fedagg_mx4_abi_version": (c_int, []),
    "fedagg_mx4_last_error": (ctypes.c_char_p, []),
    "fedagg_mx4_blocking": (c_int, [P(c_int), P(c_int)]),
    "fedagg_mx4_fedavg_e2m1": (c_int, [P(c_void), P(c_void), P(ctypes.c_float), c_int, c_u64, P(c_u64), c_int, c_void,
                                       c_void]),
    "fedagg_mx4_quantize": (c_int, [c_void, c_int, c_u64, c_void, c_void, c_void, c_void]),
}

ABI_VERSION = 1
MX4_BLOCK = 32  # FEDAGG_MX4_BLOCK
MAX_PAIRWISE_K = 256  # FEDAGG_MX4_MAX_PAIRWISE_K

_library = Library(globals(), "fedagg_mx4_", "The MXFP4 wire has no fallback.")
load, loaded, check = _library.load, _library.loaded, _library.check  # loaded(): only an MXFP4 call loads it


def blocking() -> Tuple[int, int]:
    """``(tile_elems, k_group)``: the sizes at which the FedAvg kernel changes path."""
    t, g = c_int(0), c_int(0)
    check(load().fedagg_mx4_blocking(ctypes.byref(t), ctypes.byref(g)), "mx4_blocking")
    return t.value, g.value


def fedavg_e2m1(code_ptrs, scale_ptrs, weights, M: int, pairwise_idx, d_out: int, stream: int) -> None:
    """``fedagg_mx4_fedavg_e2m1`` over K device rows (lists of device addresses), fp32 ``weights``,
    the flat indices of the numel == 1 elements, into the fp32 device buffer ``d_out``."""
    K = len(code_ptrs)
    w = (ctypes.c_float * max(1, K))(*[float(v) for v in weights])
    idx = [int(v) for v in (pairwise_idx if pairwise_idx is not None else [])]
    h_idx = (c_u64 * max(1, len(idx)))(*idx)
    rc = load().fedagg_mx4_fedavg_e2m1(ptr_array(code_ptrs), ptr_array(scale_ptrs), w, K, int(M), h_idx, len(idx),
                                       d_out, stream or None)
    check(rc, "mx4_fedavg_e2m1")


def quantize(d_x: int, kind: int, M: int, d_res, d_codes: int, d_scales: int, stream: int) -> None:
    """``fedagg_mx4_quantize``: M elements of ``kind`` (FEDAGG_F32 / FEDAGG_BF16) at ``d_x`` to
    ``ceil(M / 2)`` code bytes at ``d_codes`` and ``ceil(M / 32)`` scale bytes at ``d_scales``;
    ``d_res`` (0 or None: no error feedback) the M fp32 residuals, overwritten with the new ones."""
    check(load().fedagg_mx4_quantize(d_x, int(kind), int(M), d_res or None, d_codes, d_scales, stream or None),
          "mx4_quantize")
