"""ctypes binding of ``libfedagg_mx.so`` (the C ABI declared in ``include/fedagg_mx.h``): FedAvg
over OCP MXFP8 client updates (1-byte ``e4m3fn`` codes, one ``e8m0`` scale byte per 32 elements)
and the device quantiser that produces them.

Loaded lazily, by the first MXFP8 call (``AggregationEngine.fedavg_mxfp8``, or the export of an
``accelerate_algo(..., wire="mxfp8")`` client): importing ``substrafl_amd`` and every fp32, bf16,
fp16 or fp64 federation never touch it.  As with ``libfedagg.so`` there is no fallback: a missing
library raises :class:`substrafl_amd._native.NativeLibraryError`.  ``FEDAGG_MX_LIB`` names another
copy of the library.
"""

from __future__ import annotations

import ctypes
import os
from pathlib import Path
from typing import Optional, Tuple

from ._native import NativeLibraryError

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("FEDAGG_MX_LIB", str(_HERE / "libfedagg_mx.so")))

c_u64 = ctypes.c_uint64
c_int = ctypes.c_int
c_void = ctypes.c_void_p
P = ctypes.POINTER

# Every symbol include/fedagg_mx.h declares, with its ctypes signature.
SIGNATURES = {
    "fedagg_mx_abi_version": (c_int, []),
    "fedagg_mx_last_error": (ctypes.c_char_p, []),
    "fedagg_mx_blocking": (c_int, [P(c_int), P(c_int)]),
    "fedagg_mx_fedavg_e4m3": (c_int, [P(c_void), P(c_void), P(ctypes.c_float), c_int, c_u64, P(c_u64), c_int, c_void,
                                      c_void]),
    "fedagg_mx_quantize": (c_int, [c_void, c_int, c_u64, c_void, c_void, c_void]),
}

ABI_VERSION = 1
MX_BLOCK = 32  # FEDAGG_MX_BLOCK
MAX_PAIRWISE_K = 256  # FEDAGG_MX_MAX_PAIRWISE_K

_lib: Optional[ctypes.CDLL] = None


def loaded() -> bool:
    """Whether this process has loaded the library (only an MXFP8 call does)."""
    return _lib is not None


def load() -> ctypes.CDLL:
    """Load (once) and return the library; raise loudly if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise NativeLibraryError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). The MXFP8 wire has no fallback."
        )
    try:
        lib = ctypes.CDLL(str(LIB_PATH))
    except OSError as e:  # pragma: no cover - depends on the box
        raise NativeLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.fedagg_mx_abi_version() != ABI_VERSION:
        raise NativeLibraryError("libfedagg_mx ABI version mismatch")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().fedagg_mx_last_error().decode(errors="replace")
        raise NativeLibraryError(f"{what} failed ({rc}): {msg}")


def blocking() -> Tuple[int, int]:
    """``(tile_elems, k_group)``: the sizes at which the FedAvg kernel changes path."""
    t, g = c_int(0), c_int(0)
    check(load().fedagg_mx_blocking(ctypes.byref(t), ctypes.byref(g)), "mx_blocking")
    return t.value, g.value


def fedavg_e4m3(code_ptrs, scale_ptrs, weights, M: int, pairwise_idx, d_out: int, stream: int) -> None:
    """``fedagg_mx_fedavg_e4m3`` over K device rows (lists of device addresses), fp32 ``weights``,
    the flat indices of the numel == 1 elements, into the fp32 device buffer ``d_out``."""
    from ._native import ptr_array

    K = len(code_ptrs)
    w = (ctypes.c_float * max(1, K))(*[float(v) for v in weights])
    idx = [int(v) for v in (pairwise_idx if pairwise_idx is not None else [])]
    h_idx = (c_u64 * max(1, len(idx)))(*idx)
    rc = load().fedagg_mx_fedavg_e4m3(ptr_array(code_ptrs), ptr_array(scale_ptrs), w, K, int(M), h_idx, len(idx),
                                      d_out, stream or None)
    check(rc, "mx_fedavg_e4m3")


def quantize(d_x: int, kind: int, M: int, d_codes: int, d_scales: int, stream: int) -> None:
    """``fedagg_mx_quantize``: M elements of ``kind`` (FEDAGG_F32 / FEDAGG_BF16) at ``d_x`` to M code
    bytes at ``d_codes`` and ``ceil(M / 32)`` scale bytes at ``d_scales``."""
    check(load().fedagg_mx_quantize(d_x, int(kind), int(M), d_codes, d_scales, stream or None), "mx_quantize")
