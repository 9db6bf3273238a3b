"""The one loader behind every ctypes binding of the package (``_native`` and the ``_native_*``
modules of the libraries next to ``libfedagg.so``): find the library, open it, bind the signatures,
check the ABI version, keep the handle, and turn a failed call into :class:`NativeLibraryError`.

A binding module states what differs: its ``LIB_PATH`` (:func:`lib_path`), ``SIGNATURES`` and
``ABI_VERSION``, and one :class:`Library` with its symbol prefix and the hint of its "not found"
message.  The loader reads those three names from the module at every ``load()`` and keeps the
handle in the module's ``_lib``, so they stay what a caller or a test sees and may replace.
"""

from __future__ import annotations

import ctypes
import os
from pathlib import Path
from typing import Callable, Optional

PACKAGE_DIR = Path(__file__).resolve().parent


class NativeLibraryError(RuntimeError):
    """A native library is missing, failed to load, or a call returned an error code."""


def lib_path(env: str, name: str) -> Path:
    """``$env`` when set, else ``name`` in the package directory (where ``build()`` links it)."""
    return Path(os.environ.get(env, str(PACKAGE_DIR / name)))


class Library:
    """``ns`` is the binding module's ``globals()``; ``prefix`` the library's symbol prefix
    (``fedagg_mx_``: ``fedagg_mx_abi_version``, ``fedagg_mx_last_error``, and ``libfedagg_mx`` in the
    ABI message); ``hint`` ends the "not found" message.  ``more_signatures(lib)`` returns further
    signatures to bind, decided by the opened library."""

    def __init__(self, ns: dict, prefix: str, hint: str, more_signatures: Optional[Callable] = None):
        self.ns, self.prefix, self.hint, self.more_signatures = ns, prefix, hint, more_signatures
        ns["_lib"] = None

    def loaded(self) -> bool:
        """Whether this process has loaded the library."""
        return self.ns["_lib"] is not None

    def load(self) -> ctypes.CDLL:
        """Load (once) and return the library; raise loudly if it is not there."""
        ns = self.ns
        if ns["_lib"] is not None:
            return ns["_lib"]
        path = ns["LIB_PATH"]
        if not path.exists():
            raise NativeLibraryError(
                f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                f"(hipcc --offload-arch=gfx950). {self.hint}"
            )
        try:
            lib = ctypes.CDLL(str(path))
        except OSError as e:  # pragma: no cover - depends on the box
            raise NativeLibraryError(f"cannot load {path}: {e}") from e
        sigs = dict(ns["SIGNATURES"])
        if self.more_signatures is not None:
            sigs.update(self.more_signatures(lib))
        for name, (res, args) in sigs.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if getattr(lib, self.prefix + "abi_version")() != ns["ABI_VERSION"]:
            raise NativeLibraryError(f"lib{self.prefix.rstrip('_')} ABI version mismatch")
        ns["_lib"] = lib
        return lib

    def check(self, rc: int, what: str) -> None:
        if rc != 0:
            msg = getattr(self.load(), self.prefix + "last_error")().decode(errors="replace")
            raise NativeLibraryError(f"{what} failed ({rc}): {msg}")
