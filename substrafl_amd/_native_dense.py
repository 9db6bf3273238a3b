"""ctypes binding of ``libfedagg_dense.so`` (the C ABI declared in ``include/fedagg_dense.h``):
the opt-in dense fp64 solves of NewtonRaphson's Newton system on the GPU (LU, and Cholesky with its
symmetry test), the Cholesky of its clients' Hessian check and FedPCA's Householder LQ.

Loaded lazily, by the first call that asks for the device solve: importing ``substrafl_amd`` and
every default path never touch it.  As with ``libfedagg.so`` there is no fallback: a missing
library raises :class:`substrafl_amd._native.NativeLibraryError`.
"""

from __future__ import annotations

import ctypes
import os
from pathlib import Path
from typing import Optional

from ._native import NativeLibraryError

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("FEDAGG_DENSE_LIB", str(_HERE / "libfedagg_dense.so")))

c_u64 = ctypes.c_uint64
c_int = ctypes.c_int
c_void = ctypes.c_void_p
P = ctypes.POINTER

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

_lib: Optional[ctypes.CDLL] = None


def loaded() -> bool:
    """Whether this process has loaded the dense library (the default paths never do)."""
    return _lib is not None


def load() -> ctypes.CDLL:
    """Load (once) and return the dense library; raise loudly if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise NativeLibraryError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). The device solve has no CPU fallback; solve='host' needs no library."
        )
    try:
        lib = ctypes.CDLL(str(LIB_PATH))
    except OSError as e:  # pragma: no cover - depends on the box
        raise NativeLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.fedagg_dense_abi_version() != ABI_VERSION:
        raise NativeLibraryError("libfedagg_dense ABI version mismatch")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().fedagg_dense_last_error().decode(errors="replace")
        raise NativeLibraryError(f"{what} failed ({rc}): {msg}")


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
