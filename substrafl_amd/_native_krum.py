"""ctypes binding of ``libfedagg_krum.so`` (the C ABI declared in ``include/fedagg_krum.h``): the fp64
Gram matrix of K client rows on the matrix units, the device half of Krum and multi-Krum.

Loaded lazily, by the first Krum call (``AggregationEngine.fedavg_robust`` with ``rule="krum"`` or
``"multi_krum"``, behind ``FedAvg(..., robust=...)``): importing ``substrafl_amd`` and every other
federation never touch it.  There is no fallback: a missing library raises
:class:`substrafl_amd._native.NativeLibraryError`.  ``FEDAGG_KRUM_LIB`` names another copy of the library.
"""

from __future__ import annotations

import ctypes
from typing import Tuple

from ._loader import Library, lib_path
from ._native import P, c_int, c_u64, c_void, ptr_array

LIB_PATH = lib_path("FEDAGG_KRUM_LIB", "libfedagg_krum.so")

# Every symbol include/fedagg_krum.h declares, with its ctypes signature.
SIGNATURES = {
    "fedagg_krum_abi_version": (c_int, []),
    "fedagg_krum_last_error": (ctypes.c_char_p, []),
    "fedagg_krum_blocking": (c_int, [P(c_int), P(c_int), P(c_int)]),
    "fedagg_krum_ws_bytes": (c_int, [c_int, c_u64, P(c_u64)]),
    "fedagg_krum_gram": (c_int, [P(c_void), c_int, c_int, c_u64, c_void, c_u64, c_void, c_void]),
}

ABI_VERSION = 1
MAX_K = 128  # FEDAGG_KRUM_MAX_K

_library = Library(globals(), "fedagg_krum_", "Krum has no fallback.")
load, loaded, check = _library.load, _library.loaded, _library.check  # loaded(): only a Krum call loads it


def blocking() -> Tuple[int, int, int]:
    """``(chunk_elems, vec_f32, vec_bf16)``: the sizes at which the kernel changes path."""
    v = [c_int(0) for _ in range(3)]
    check(load().fedagg_krum_blocking(*[ctypes.byref(c) for c in v]), "krum_blocking")
    return tuple(c.value for c in v)


def ws_bytes(K: int, M: int) -> int:
    """Bytes of workspace ``gram`` needs for K rows of M elements (no HIP call)."""
    n = c_u64(0)
    check(load().fedagg_krum_ws_bytes(int(K), int(M), ctypes.byref(n)), "krum_ws_bytes")
    return int(n.value)


def gram(row_ptrs, kind: int, M: int, d_ws: int, nbytes: int, d_G: int, stream: int) -> None:
    """``fedagg_krum_gram`` over K device rows (a list of device addresses) of ``kind`` (FEDAGG_F32 /
    FEDAGG_BF16): the K x K fp64 matrix of their inner products at ``d_G``, through the ``nbytes`` of
    workspace at ``d_ws``."""
    check(load().fedagg_krum_gram(ptr_array(row_ptrs), int(kind), len(row_ptrs), int(M), d_ws, int(nbytes), d_G,
                                  stream or None), "krum_gram")
