"""ctypes binding of ``libfedagg_dense.so`` (the C ABI declared in ``include/fedagg_dense.h``):
the opt-in dense fp64 solves of NewtonRaphson's Newton system on the GPU (LU, and Cholesky with its
symmetry test), the Cholesky of its clients' Hessian check and FedPCA's Householder LQ.

Loaded lazily, by the first call that asks for the device solve: importing ``substrafl_amd`` and
every default path never touch it.  As with ``libfedagg.so`` there is no fallback: a missing
library raises :class:`substrafl_amd._native.NativeLibraryError`.
"""

from __future__ import annotations

import ctypes

from ._loader import Library, lib_path
from ._native import P, c_int, c_u64, c_void

LIB_PATH = lib_path("FEDAGG_DENSE_LIB", "libfedagg_dense.so")

# Every symbol include/fedagg_dense.h declares, with its ctypes signature.
SIGNATURES = {
    "fedagg_dense_abi_version": (c_int, []),
    "fedagg_dense_last_error": (ctypes.c_char_p, []),
    "fedagg_dense_blocking": (c_int, [P(c_int), P(c_int), P(c_int)]),
    "fedagg_dense_ws_bytes": (c_u64, [c_u64]),
    "fedagg_dense_getrf_f64": (c_int, [c_void, c_u64, c_u64, c_void, c_void, c_void, c_void]),
    "fedagg_dense_getrs_f64": (c_int, [c_void, c_u64, c_u64, c_void, c_void, c_void]),
    "fedagg_dense_solve_f64": (c_int, [c_void, c_u64, c_u64, c_void, c_void, c_void, c_void, c_void]),
    "fedagg_dense_potrf_f64": (c_int, [c_void, c_u64, c_u64, c_void, c_void]),
    "fedagg_dense_lq_blocking": (c_int, [P(c_int), P(c_int), P(c_int), P(c_int)]),
    "fedagg_dense_lq_ws_bytes": (c_u64, [c_u64, c_u64]),
    "fedagg_dense_gelqf_f64": (c_int, [c_void, c_u64, c_u64, c_u64, c_void, c_void, c_void]),
    "fedagg_dense_orglq_f64": (c_int, [c_void, c_u64, c_u64, c_u64, c_void, c_void, c_u64, c_void, c_void]),
    "fedagg_dense_symcopy_f64": (c_int, [c_void, c_u64, c_u64, c_void, c_u64, c_void, c_void]),
    "fedagg_dense_potrs_f64": (c_int, [c_void, c_u64, c_u64, c_void, c_void]),
}

ABI_VERSION = 1

_library = Library(globals(), "fedagg_dense_",
                   "The device solve has no CPU fallback; solve='host' needs no library.")
load, loaded, check = _library.load, _library.loaded, _library.check  # loaded(): the default paths never load it


def call(name: str, *args) -> None:
    """``fedagg_dense_<name>(*args)``, checked.  Device addresses and the stream go in as plain
    ``int``: the ``c_void_p`` argtypes of :data:`SIGNATURES` convert them, ``0`` to NULL."""
    check(getattr(load(), "fedagg_dense_" + name)(*args), "dense_" + name)


def blocking() -> tuple:
    """``(panel, tile_m, tile_n)`` of the kernels (``fedagg_dense_blocking``)."""
    a, b, c = c_int(), c_int(), c_int()
    check(load().fedagg_dense_blocking(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "dense_blocking")
    return a.value, b.value, c.value


def lq_blocking() -> tuple:
    """``(panel, tile_m, tile_n, k_chunk)`` of the LQ kernels (``fedagg_dense_lq_blocking``)."""
    a, b, c, d = c_int(), c_int(), c_int(), c_int()
    check(load().fedagg_dense_lq_blocking(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)),
          "dense_lq_blocking")
    return a.value, b.value, c.value, d.value
