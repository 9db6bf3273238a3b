"""libfedagg_dense.so (include/fedagg_dense.h): the library exports what the header declares, the
ctypes binding covers exactly that, bad arguments come back as -1 with their own text before any
HIP call, and the C demo compiles against the headers alone (CPU only: no kernel is launched)."""

import ctypes
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

from substrafl_amd import _native, _native_dense

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "fedagg_dense.h"


def declared_functions():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\s*\*?\s*(fedagg_dense_[a-z0-9_]+)\s*\(", text,
                                 flags=re.M)))


def test_library_exports_every_declared_symbol_and_binding_matches():
    names = declared_functions()
    assert {"fedagg_dense_getrf_f64", "fedagg_dense_getrs_f64", "fedagg_dense_solve_f64", "fedagg_dense_blocking",
            "fedagg_dense_ws_bytes", "fedagg_dense_abi_version", "fedagg_dense_last_error"} <= set(names)
    lib = ctypes.CDLL(str(_native_dense.LIB_PATH))
    for name in names:
        assert hasattr(lib, name), name
    assert sorted(_native_dense.SIGNATURES) == names
    # a library of its own: none of fedagg.h's entry points, and the product binding knows nothing of it
    assert not hasattr(lib, "fedagg_abi_version")
    assert not any(k.startswith("fedagg_dense") for k in _native.SIGNATURES)


def test_abi_version_blocking_and_workspace():
    lib = _native_dense.load()
    assert lib.fedagg_dense_abi_version() == _native_dense.ABI_VERSION == 1
    panel, tm, tn = _native_dense.blocking()
    assert panel > 0 and tm > 0 and tn > 0
    assert 5 * max(panel, tm, tn) + 7 <= 800  # the GPU tests derive their sizes from these
    assert lib.fedagg_dense_blocking(None, None, None) == -1
    assert b"NULL output" in lib.fedagg_dense_last_error()
    assert lib.fedagg_dense_ws_bytes(0) == 0
    assert lib.fedagg_dense_ws_bytes(4096) < 4096 * 4096 * 8  # never a second matrix


def test_bad_arguments_are_refused_before_any_hip_call():
    lib = _native_dense.load()
    A, B, I = 0x1000, 0x2000, 0x3000  # never dereferenced: every check comes before the first HIP call
    err = lib.fedagg_dense_last_error
    # n == 0: OK, nothing touched, whatever the pointers
    assert lib.fedagg_dense_getrf_f64(None, 0, 0, None, None, None, None) == 0
    assert lib.fedagg_dense_getrs_f64(None, 0, 0, None, None, None) == 0
    assert lib.fedagg_dense_solve_f64(None, 0, 0, None, None, None, None, None) == 0
    assert lib.fedagg_dense_getrf_f64(None, 4, 4, I, I, None, None) == -1 and b"d_A is NULL" in err()
    assert lib.fedagg_dense_getrf_f64(A, 4, 3, I, I, None, None) == -1 and b"smaller than n" in err()
    assert lib.fedagg_dense_getrf_f64(A, 4, 4, None, I, None, None) == -1 and b"d_ipiv is NULL" in err()
    assert lib.fedagg_dense_getrf_f64(A, 4, 4, I, None, None, None) == -1 and b"d_info is NULL" in err()
    assert lib.fedagg_dense_getrf_f64(A, 2, 1 << 62, I, I, None, None) == -1 and b"overflows" in err()
    assert lib.fedagg_dense_getrf_f64(A, (1 << 20) + 1, 1 << 21, I, I, None, None) == -1 and b"FEDAGG_DENSE_MAX_N" in err()
    assert lib.fedagg_dense_getrs_f64(None, 4, 4, I, B, None) == -1 and b"d_A is NULL" in err()
    assert lib.fedagg_dense_getrs_f64(A, 4, 4, None, B, None) == -1 and b"d_ipiv is NULL" in err()
    assert lib.fedagg_dense_getrs_f64(A, 4, 4, I, None, None) == -1 and b"d_b is NULL" in err()
    assert lib.fedagg_dense_getrs_f64(A, 4, 2, I, B, None) == -1 and b"smaller than n" in err()
    assert lib.fedagg_dense_getrs_f64(A, 3, (1 << 64) - 1, I, B, None) == -1 and b"overflows" in err()
    assert lib.fedagg_dense_solve_f64(A, 4, 4, I, I, None, None, None) == -1 and b"d_b is NULL" in err()
    assert lib.fedagg_dense_solve_f64(A, 4, 4, I, None, B, None, None) == -1 and b"d_info is NULL" in err()
    assert lib.fedagg_dense_solve_f64(A, 4, 1, I, I, B, None, None) == -1 and b"smaller than n" in err()
    with pytest.raises(_native.NativeLibraryError, match="smaller than n"):
        _native_dense.check(-1, "x")


def test_call_takes_plain_ints_for_pointers_and_keeps_the_error_text():
    """``_native_dense.call``: the engine passes device addresses and the stream as ``int``."""
    # what the declared argtypes make of an int, without the library: labs() hands its argument back
    labs = ctypes.CDLL(None).labs
    labs.restype, labs.argtypes = ctypes.c_long, [_native_dense.c_void]
    assert labs(0x7F0012345678) == 0x7F0012345678 and labs(0) == 0
    with pytest.raises(ctypes.ArgumentError):
        labs(1.0)
    for name, (_, args) in _native_dense.SIGNATURES.items():
        if name.endswith("_f64"):  # every entry point the engine reaches through call()
            assert set(args) <= {_native_dense.c_void, _native_dense.c_u64}, name
    # the library's argument checks come before any HIP call: no address below is dereferenced
    L, B = 0x1000, 0x2000
    assert _native_dense.call("potrs_f64", 0, 0, 0, 0, 0) is None  # n == 0
    with pytest.raises(_native.NativeLibraryError, match=r"^dense_potrs_f64 failed \(-1\): d_L is NULL$"):
        _native_dense.call("potrs_f64", 0, 4, 4, B, 0)
    with pytest.raises(_native.NativeLibraryError, match=r"^dense_potrs_f64 failed \(-1\): d_b is NULL$"):
        _native_dense.call("potrs_f64", L, 4, 4, 0, 0)
    with pytest.raises(_native.NativeLibraryError, match=r"^dense_getrf_f64 failed \(-1\): lda = 3 is smaller than n$"):
        _native_dense.call("getrf_f64", L, 4, 3, B, B, 0, 0)
    with pytest.raises(_native.NativeLibraryError, match=r"^dense_symcopy_f64 failed \(-1\): d_flag is NULL$"):
        _native_dense.call("symcopy_f64", L, 4, 4, 0, 4, 0, 0)


def test_missing_dense_library_is_loud_and_names_the_host_solve(monkeypatch, tmp_path):
    monkeypatch.setattr(_native_dense, "_lib", None)
    monkeypatch.setattr(_native_dense, "LIB_PATH", tmp_path / "nope.so")
    with pytest.raises(_native.NativeLibraryError, match="no CPU fallback"):
        _native_dense.load()


def test_importing_the_package_and_the_default_path_do_not_load_it():
    """A fresh interpreter: the package, the integration module and an accelerated NewtonRaphson
    class with the default ``solve`` never load libfedagg_dense.so."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import substrafl_amd, substrafl_amd.integration as I, substrafl_amd.engine\n"
            "import standin_substrafl.strategies as ss\n"
            "cls = I.accelerate(ss.NewtonRaphson)\n"
            "assert cls._fedagg_solve == 'host'\n"
            "assert 'substrafl_amd._native_dense' not in sys.modules\n"
            "assert 'libfedagg_dense' not in open('/proc/self/maps').read()\n" % (str(ROOT), str(ROOT / "tests")))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120)


def test_solve_option_is_validated():
    import standin_substrafl.strategies as ss

    from substrafl_amd.integration import accelerate

    with pytest.raises(ValueError, match="solve"):
        accelerate(ss.NewtonRaphson, solve="gpu")
    assert accelerate(ss.NewtonRaphson, solve="device")._fedagg_solve == "device"
    assert accelerate(ss.FedAvg, solve="device")  # accepted and without effect for the other strategies


def test_c_demo_compiles_against_the_headers(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    exe = tmp_path / "dense_solve_demo"
    libdir = _native_dense.LIB_PATH.parent
    subprocess.run([gcc, "-O2", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "c" / "dense_solve_demo.c"),
                    f"-L{libdir}", "-lfedagg_dense", "-lfedagg", f"-Wl,-rpath,{libdir}",
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert exe.exists()
