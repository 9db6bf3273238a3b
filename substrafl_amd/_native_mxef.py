"""ctypes binding of ``libfedagg_mxef.so`` (the C ABI declared in ``include/fedagg_mxef.h``): the
MXFP8 quantiser with error feedback, one fused kernel that adds the client's fp32 residual to the
update, encodes the sum and leaves what the encoding dropped as the new residual.

Loaded lazily, by the first export that carries a residual (an
``accelerate_algo(..., wire="mxfp8", error_feedback=True)`` client, or
``weight_manager.export_mxfp8(..., residual=...)``): every other federation, the plain MXFP8 wire
included, never touches it.  There is no fallback: a missing library raises
:class:`substrafl_amd._native.NativeLibraryError`.  ``FEDAGG_MXEF_LIB`` names another copy of the
library.
"""

from __future__ import annotations

import ctypes
from typing import Tuple

from ._loader import Library, lib_path
from ._native import P, c_int, c_u64, c_void

LIB_PATH = lib_path("FEDAGG_MXEF_LIB", "libfedagg_mxef.so")

# Every symbol include/fedagg_mxef.h declares, with its ctypes signature.
SIGNATURES = {
    "fedagg_mxef_abi_version": (c_int, []),
    "fedagg_mxef_last_error": (ctypes.c_char_p, []),
    "fedagg_mxef_blocking": (c_int, [P(c_int), P(c_int), P(c_u64)]),
    "fedagg_mxef_quantize": (c_int, [c_void, c_int, c_u64, c_void, c_void, c_void, c_void]),
}

ABI_VERSION = 1

_library = Library(globals(), "fedagg_mxef_", "Error feedback on the MXFP8 wire has no fallback.")
load, loaded, check = _library.load, _library.loaded, _library.check  # loaded(): only an export with a residual loads it


def blocking() -> Tuple[int, int, int]:
    """``(lane_elems, tile_elems, second_step_elems)``: the sizes at which the kernel changes path."""
    lane, tile, second = c_int(0), c_int(0), c_u64(0)
    check(load().fedagg_mxef_blocking(ctypes.byref(lane), ctypes.byref(tile), ctypes.byref(second)), "mxef_blocking")
    return lane.value, tile.value, second.value


def quantize_ef(d_x: int, kind: int, M: int, d_res: int, d_codes: int, d_scales: int, stream: int) -> None:
    """``fedagg_mxef_quantize``: M elements of ``kind`` (FEDAGG_F32 / FEDAGG_BF16) at ``d_x`` plus the
    M fp32 residuals at ``d_res`` to M code bytes at ``d_codes`` and ``ceil(M / 32)`` scale bytes at
    ``d_scales``; ``d_res`` is overwritten with the new residual."""
    check(load().fedagg_mxef_quantize(d_x, int(kind), int(M), d_res, d_codes, d_scales, stream or None),
          "mxef_quantize")
