"""libfedagg_promote.so (include/fedagg_promote.h): the library exports what the header declares,
the binding's SIGNATURES are the header's prototypes, every refusal the header lists returns
FEDAGG_EINVAL with its own text before any HIP call (so none of this needs a GPU), and nothing but
a 16-bit model next to fp64 operands on a device loads the library."""

import ctypes
import re
import subprocess
import sys
from pathlib import Path

import pytest

from substrafl_amd import _native, _native_promote

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "fedagg_promote.h"
F16, F32, F64, BF16 = _native.FEDAGG_F16, _native.FEDAGG_F32, _native.FEDAGG_F64, _native.FEDAGG_BF16


def _header_names():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\s*\*?\s*(fedagg_promote_[a-z0-9_]+)\s*\(", text,
                                 flags=re.M)))


def test_signatures_are_the_header():
    names = _header_names()
    assert names == sorted(_native_promote.SIGNATURES)
    assert {"fedagg_promote_wsum", "fedagg_promote_increment", "fedagg_promote_tune", "fedagg_promote_abi_version",
            "fedagg_promote_last_error"} == set(names)
    lib = _native_promote.load()
    for n in names:
        assert hasattr(lib, n), n
    # a library of its own: libfedagg.so's binding knows none of it
    assert not any(k.startswith("fedagg_promote") for k in _native.SIGNATURES)


def test_abi_version_and_tune():
    lib = _native_promote.load()
    assert lib.fedagg_promote_abi_version() == _native_promote.ABI_VERSION == 1
    assert "#define FEDAGG_PROMOTE_ABI_VERSION 1" in HEADER.read_text()
    assert lib.fedagg_promote_tune(b"vec", 0) == 0 and lib.fedagg_promote_tune(b"vec", 1) == 0
    assert lib.fedagg_promote_tune(b"vec", 2) == -1 and b"0 or 1" in lib.fedagg_promote_last_error()
    assert lib.fedagg_promote_tune(b"flat_vec", 1) == -1 and b"unknown key" in lib.fedagg_promote_last_error()
    assert lib.fedagg_promote_tune(None, 1) == -1


def _wsum(lib, kinds, ptrs, numel=(64,), nlists=None, L=None, flat=0x10000, coeffs=True):
    nl = len(kinds) if nlists is None else nlists
    L = len(numel) if L is None else L
    return lib.fedagg_promote_wsum(_native.ptr_array(ptrs) if ptrs is not None else None,
                                   (ctypes.c_int * max(1, len(kinds)))(*kinds) if kinds is not None else None, nl,
                                   (ctypes.c_double * max(1, len(kinds or [0])))() if coeffs else None,
                                   (ctypes.c_uint64 * max(1, len(numel)))(*numel) if numel is not None else None, L,
                                   flat, None)


def test_every_refusal_has_its_own_text_and_needs_no_gpu():
    """Fake non-NULL pointers: a refused call has made no HIP call, so nothing is dereferenced."""
    lib = _native_promote.load()
    err = lib.fedagg_promote_last_error
    A, B, C = 0x100000, 0x200000, 0x300000  # 16-B aligned fakes
    texts = []

    def refused(rc, needle):
        assert rc == -1, needle
        msg = err()
        assert needle in msg, (needle, msg)
        texts.append(msg)

    refused(_wsum(lib, [F16, F32], [A, B]), b"is fp32")
    refused(_wsum(lib, [F32, F64], [A, B]), b"is fp32")
    refused(_wsum(lib, [F16, BF16, F64], [A, B, C]), b"F16 next to BF16")
    refused(_wsum(lib, [BF16, F64, F16], [A, B, C]), b"F16 next to BF16")
    refused(_wsum(lib, [F64, F64], [A, B]), b"no 16-bit list")
    refused(_wsum(lib, [F16, F16], [A, B]), b"no fp64 list")
    refused(_wsum(lib, [BF16], [A]), b"no fp64 list")
    refused(_wsum(lib, [F16, 5], [A, B]), b"unsupported kind")
    refused(_wsum(lib, [F16, F64], [A, B], nlists=0), b"nlists outside")
    refused(_wsum(lib, [F16, F64, F64, F64, F64], [A] * 5), b"nlists outside")
    refused(_wsum(lib, None, [A, B], nlists=2), b"kinds is NULL")
    refused(_wsum(lib, [F16, F64], [A, B], L=-1), b"L is negative")
    refused(_wsum(lib, [F16, F64], None), b"d_layers is NULL")
    refused(_wsum(lib, [F16, F64], [A, B], numel=None, L=1), b"numel is NULL")
    refused(_wsum(lib, [F16, F64], [0, B]), b"NULL layer pointer")
    refused(_wsum(lib, [F16, F64], [A, 0]), b"NULL layer pointer")
    refused(_wsum(lib, [F16, F64], [A + 1, B]), b"not 2-B aligned")
    refused(_wsum(lib, [BF16, F64], [A, B + 4]), b"not 8-B aligned")
    refused(_wsum(lib, [F64, F16], [A + 2, B]), b"fp64 layer pointer 0 is not 8-B aligned")
    refused(_wsum(lib, [F16, F64], [A, B], flat=0x10004), b"d_flat is not 8-B aligned")
    refused(_wsum(lib, [F16, F64], [A, B], flat=None), b"d_flat is NULL")

    n1 = (ctypes.c_uint64 * 1)(64)
    for kind in (F32, F64, 5, -1):
        refused(lib.fedagg_promote_increment(_native.ptr_array([A]), kind, n1, 1, B, 1.0, None), b"layer_kind")
    refused(lib.fedagg_promote_increment(_native.ptr_array([A]), F16, n1, -3, B, 1.0, None), b"L is negative")
    refused(lib.fedagg_promote_increment(None, BF16, n1, 1, B, 1.0, None), b"d_layers is NULL")
    refused(lib.fedagg_promote_increment(_native.ptr_array([0]), F16, n1, 1, B, 1.0, None), b"NULL layer pointer")
    refused(lib.fedagg_promote_increment(_native.ptr_array([A + 3]), BF16, n1, 1, B, 1.0, None), b"not 2-B aligned")
    refused(lib.fedagg_promote_increment(_native.ptr_array([A]), F16, n1, 1, B + 2, 1.0, None), b"d_flat is not 8-B")
    refused(lib.fedagg_promote_increment(_native.ptr_array([A]), F16, n1, 1, None, 1.0, None), b"d_flat is NULL")
    assert len(set(texts)) >= 14  # each class of refusal speaks for itself

    # nothing to do is not an error, and launches nothing: NULL pointers with numel 0, L == 0
    z = (ctypes.c_uint64 * 2)(0, 0)
    assert lib.fedagg_promote_wsum(_native.ptr_array([0, 0, 0, 0]), (ctypes.c_int * 2)(F16, F64), 2, None, z, 2, None,
                                   None) == 0
    assert lib.fedagg_promote_wsum(None, (ctypes.c_int * 2)(F64, BF16), 2, None, None, 0, None, None) == 0
    assert lib.fedagg_promote_increment(None, F16, None, 0, None, 1.0, None) == 0


def test_check_raises_with_the_librarys_text():
    lib = _native_promote.load()
    rc = lib.fedagg_promote_increment(None, F32, None, 0, None, 1.0, None)
    with pytest.raises(_native.NativeLibraryError, match="flat_promote_increment failed .*layer_kind"):
        _native_promote.check(rc, "flat_promote_increment")


def test_cpu_tensors_and_fp32_models_never_load_the_library():
    """weight_manager on CPU tensors (16-bit next to fp64 included) and on an fp32 model keeps the
    reference's torch loops and never touches libfedagg_promote.so; a fresh process, so that no
    other test's load counts."""
    code = (
        "import sys; sys.path[:0] = [%r, %r]\n"
        "import torch\n"
        "from substrafl_amd import _native_promote\n"
        "from substrafl_amd.algorithms import weight_manager as wm\n"
        "for dt in (torch.float16, torch.bfloat16, torch.float32):\n"
        "    m = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.BatchNorm1d(3)).to(dt)\n"
        "    p = wm.get_parameters(m, True)\n"
        "    u = [torch.ones_like(t, dtype=torch.float64) for t in p]\n"
        "    wm.increment_parameters(m, u, with_batch_norm_parameters=True, updates_multiplier=0.05)\n"
        "    wm.increment_parameters(m, [t.numpy() for t in u], with_batch_norm_parameters=True)\n"
        "    s = wm.weighted_sum_parameters([p, u], [1, -1])\n"
        "    assert all(t.dtype == torch.float64 for t in s)\n"
        "    assert all(t.dtype == torch.float64 for t in wm.add_parameters(u, p))\n"
        "    assert all(t.dtype == dt for t in wm.subtract_parameters(p, p))\n"
        "assert not _native_promote.loaded()\n"
        "assert 'libfedagg_promote' not in open('/proc/self/maps').read()\n" % (str(ROOT), str(ROOT / "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
