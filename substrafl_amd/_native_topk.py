"""ctypes binding of ``libfedagg_topk.so`` (the C ABI declared in ``include/fedagg_topk.h``): the
top-k sparse wire of FedAvg.  On the client the exact magnitude top-k selection with error feedback
and its ordered compaction, on the aggregator FedAvg over K sparse rows into a dense fp32 average.

Loaded lazily, by the first top-k call (``AggregationEngine.fedavg_topk``, or the export of an
``accelerate_algo(..., wire="topk", error_feedback=True)`` client): importing ``substrafl_amd`` and
every other federation, the MX wires included, never touch it.  There is no fallback: a missing
library raises :class:`substrafl_amd._native.NativeLibraryError`.  ``FEDAGG_TOPK_LIB`` names
another copy of the library.
"""

from __future__ import annotations

import ctypes
from typing import Tuple

from ._loader import Library, lib_path
from ._native import P, c_int, c_u64, c_void, ptr_array

LIB_PATH = lib_path("FEDAGG_TOPK_LIB", "libfedagg_topk.so")

# Every symbol include/fedagg_topk.h declares, with its ctypes signature.
SIGNATURES = {
    "fedagg_topk_abi_version": (c_int, []),
    "fedagg_topk_last_error": (ctypes.c_char_p, []),
    "fedagg_topk_blocking": (c_int, [P(c_int), P(c_int), P(c_int), P(c_int)]),
    "fedagg_topk_workspace": (c_int, [c_u64, c_int, P(ctypes.c_size_t), P(ctypes.c_size_t)]),
    "fedagg_topk_select": (c_int, [c_int, c_void, c_void, c_u64, c_u64, c_void, ctypes.c_size_t, c_void, c_void]),
    "fedagg_topk_compact": (c_int, [c_void, c_u64, c_void, c_void, c_u64, c_void, c_void, c_void]),
    "fedagg_topk_fedavg": (c_int, [P(c_void), P(c_void), P(c_u64), P(ctypes.c_float), c_int, c_u64, P(c_u64), c_int,
                                   c_void, ctypes.c_size_t, c_void, c_void]),
}

ABI_VERSION = 1
KMAX = 128  # FEDAGG_TOPK_KMAX
STATE_WORDS = 8  # FEDAGG_TOPK_STATE_WORDS
STATE_T, STATE_NNZ, STATE_ERROR = 0, 1, 2  # FEDAGG_TOPK_STATE_*
SUB_TILE = 4096  # the sub_tile of fedagg_topk_blocking


def fedavg_ws_bytes(M: int, K: int) -> int:
    """``fedagg_topk_workspace``'s ``fedavg_bytes`` without the library (a budget is checked before
    it loads): one uint32 per client and sub-tile edge, rounded up to 256 bytes."""
    return -(-((-(-int(M) // SUB_TILE) + 1) * int(K) * 4) // 256) * 256


_library = Library(globals(), "fedagg_topk_", "The top-k wire has no fallback.")
load, loaded, check = _library.load, _library.loaded, _library.check  # loaded(): only a top-k call loads it


def blocking() -> Tuple[int, int, int, int]:
    """``(select_tile, sub_tile, k_group, threads)``: the sizes at which the kernels change path."""
    v = [c_int(0) for _ in range(4)]
    check(load().fedagg_topk_blocking(*[ctypes.byref(c) for c in v]), "topk_blocking")
    return tuple(c.value for c in v)


def workspace(M: int, K: int = 0) -> Tuple[int, int]:
    """``(select_bytes, fedavg_bytes)`` of ``d_ws`` for M elements and K rows."""
    a, b = ctypes.c_size_t(0), ctypes.c_size_t(0)
    check(load().fedagg_topk_workspace(int(M), int(K), ctypes.byref(a), ctypes.byref(b)), "topk_workspace")
    return a.value, b.value


def select(kind: int, d_x: int, d_res: int, M: int, k: int, d_ws: int, ws_bytes: int, d_state: int, stream: int) -> None:
    """``fedagg_topk_select``: ``r = fl32(x + res)`` over ``d_res`` in place, the k-th largest
    magnitude and nnz to ``d_state``, the tile offsets to ``d_ws``."""
    check(load().fedagg_topk_select(int(kind), d_x, d_res, int(M), int(k), d_ws, int(ws_bytes), d_state, stream or None),
          "topk_select")


def compact(d_res: int, M: int, d_ws: int, d_state: int, nnz: int, d_idx: int, d_val: int, stream: int) -> None:
    """``fedagg_topk_compact``: the ``nnz`` kept indices and values in index order, and the new
    residual over ``d_res``."""
    check(load().fedagg_topk_compact(d_res, int(M), d_ws, d_state, int(nnz), d_idx or None, d_val or None,
                                     stream or None), "topk_compact")


def fedavg(idx_ptrs, val_ptrs, nnz, weights, M: int, pairwise_idx, d_ws: int, ws_bytes: int, d_out: int,
           stream: int) -> None:
    """``fedagg_topk_fedavg`` over K sparse device rows (lists of device addresses and their
    lengths), fp32 ``weights``, the flat indices of the numel == 1 elements: M fp32 to ``d_out``."""
    K = len(idx_ptrs)
    w = (ctypes.c_float * max(1, K))(*[float(v) for v in weights])
    n = (c_u64 * max(1, K))(*[int(v) for v in nnz])
    idx = [int(v) for v in (pairwise_idx if pairwise_idx is not None else [])]
    h_idx = (c_u64 * max(1, len(idx)))(*idx)
    rc = load().fedagg_topk_fedavg(ptr_array(idx_ptrs), ptr_array(val_ptrs), n, w, K, int(M), h_idx, len(idx), d_ws,
                                   int(ws_bytes), d_out, stream or None)
    check(rc, "topk_fedavg")
