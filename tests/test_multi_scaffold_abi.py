"""``fedagg_multi_scaffold_bucket`` without a GPU: the plain-C demo compiles against the header, and
every bad argument is refused with ``FEDAGG_EINVAL`` before any HIP call -- the library is loaded,
no device is opened, no engine exists (``m`` is NULL throughout; the entry checks it last, so each
case is refused for its own reason and the error text says which)."""

import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from substrafl_amd import _native

ROOT = Path(__file__).resolve().parents[1]
F16, F32, F64, BF16 = _native.FEDAGG_F16, _native.FEDAGG_F32, _native.FEDAGG_F64, _native.FEDAGG_BF16
K, M = 3, 40


def test_the_demo_compiles_against_the_header(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    exe = tmp_path / "scaffold_multi_demo"
    libdir = _native.LIB_PATH.parent
    subprocess.run([gcc, "-O2", "-ffp-contract=off", "-Wall", "-Werror", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "c" / "scaffold_multi_demo.c"), f"-L{libdir}", "-lfedagg",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert exe.exists()


def test_the_binding_is_declared_and_bound():
    lib = _native.load()
    assert "fedagg_multi_scaffold_bucket" in _native.SIGNATURES
    assert len(_native.SIGNATURES["fedagg_multi_scaffold_bucket"][1]) == 18
    assert hasattr(lib, "fedagg_multi_scaffold_bucket")
    header = (ROOT / "include" / "fedagg.h").read_text()
    assert "int fedagg_multi_scaffold_bucket(fedagg_multi* m, int phase, int K" in header


class Call:
    """A valid phase-1 call over host arrays (two uneven segments per row), one argument replaced
    at a time."""

    def __init__(self, row_kind=F32, c_kind=F32, esz=4, c_esz=4):
        self.rows = np.zeros((K, M * esz), np.uint8)
        self.c = np.zeros((K, M * c_esz), np.uint8)
        cut, c_cut = 7 * esz, 7 * c_esz
        self.args = dict(
            m=None, phase=1, K=K, nseg=2,
            h_rows=self._table(self.rows, cut), seg_bytes=(ctypes.c_uint64 * 2)(cut, M * esz - cut),
            row_kind=row_kind, h_w=np.full(K, 1.0 / K).ctypes.data, lr=0.5, Kc=K, c_nseg=2,
            h_c=self._table(self.c, c_cut), c_seg_bytes=(ctypes.c_uint64 * 2)(c_cut, M * c_esz - c_cut),
            c_kind=c_kind, h_idx=(ctypes.c_uint64 * 2)(0, M - 1), P=2,
            h_out=np.zeros(M, np.float64).ctypes.data, mismatches=ctypes.pointer(ctypes.c_uint64(0)))

    @staticmethod
    def _table(a, cut):
        t = (ctypes.c_void_p * (2 * a.shape[0]))()
        for k in range(a.shape[0]):
            t[2 * k], t[2 * k + 1] = a[k].ctypes.data, a[k].ctypes.data + cut
        return t

    def __call__(self, **changed):
        lib = _native.load()
        a = dict(self.args, **changed)
        rc = lib.fedagg_multi_scaffold_bucket(*[a[k] for k in self.args])
        return rc, lib.fedagg_last_error().decode()


def u64(*v):
    return (ctypes.c_uint64 * len(v))(*v)


def test_bad_arguments_are_refused_before_any_hip_call():
    call = Call()
    # with everything else valid, the NULL engine is what is refused
    assert call() == (-1, "fedagg_multi_scaffold_bucket: NULL engine")
    assert call(phase=0, Kc=0, c_nseg=0, h_c=None, c_seg_bytes=None, c_kind=0, mismatches=None) == (
        -1, "fedagg_multi_scaffold_bucket: NULL engine")
    for changed, text in [
        (dict(K=0), "K must be > 0"),
        (dict(K=-2), "K must be > 0"),
        (dict(phase=2), "phase must be 0 or 1"),
        (dict(row_kind=_native.FEDAGG_F64 + 1), "unknown row kind"),  # FEDAGG_I8
        (dict(row_kind=99), "unknown row kind"),
        (dict(c_kind=11), "unknown c kind"),
        (dict(c_kind=F64), "c kind must equal the kind of f32 / f64 rows"),
        (dict(c_kind=F16, c_seg_bytes=u64(14, 66)), "c kind must equal the kind of f32 / f64 rows"),
        (dict(Kc=2), "Kc must be 1 or K"),
        (dict(Kc=0), "Kc must be 1 or K"),
        (dict(seg_bytes=u64(30, 130)), "segment not a whole number of elements"),
        (dict(c_seg_bytes=u64(26, 134)), "c segment not a whole number of elements"),
        (dict(c_seg_bytes=u64(28, 128)), "a c row does not total M elements"),
        (dict(c_nseg=1), "a c row does not total M elements"),
        (dict(h_idx=u64(0, M)), "numel == 1 index out of range"),
        (dict(h_out=None), "NULL h_out"),
        (dict(mismatches=None), "NULL mismatches with Kc == K"),
        (dict(h_w=None), "invalid argument"),
        (dict(h_rows=None), "invalid argument"),
        (dict(h_idx=None), "invalid argument"),
        (dict(P=-1), "invalid argument"),
        (dict(h_c=None), "invalid c argument"),
    ]:
        rc, err = call(**changed)
        assert rc == -1 and err == "fedagg_multi_scaffold_bucket: " + text, (changed, rc, err)
    # NULL mismatches is fine when nothing is compared, and phase 0 reads none of the c arguments
    assert call(Kc=1, mismatches=None)[1].endswith("NULL engine")
    assert call(phase=0, Kc=7, c_kind=99, c_nseg=-1, h_c=None, c_seg_bytes=None, mismatches=None)[1].endswith(
        "NULL engine")


@pytest.mark.parametrize("row_kind,esz,c_kind,c_esz,ok", [
    (F16, 2, F16, 2, True), (F16, 2, BF16, 2, True), (F16, 2, F32, 4, True), (F16, 2, F64, 8, True),
    (BF16, 2, F16, 2, True), (BF16, 2, BF16, 2, True), (BF16, 2, F32, 4, True), (BF16, 2, F64, 8, True),
    (F32, 4, F32, 4, True), (F64, 8, F64, 8, True),
    (F32, 4, F16, 2, False), (F32, 4, BF16, 2, False), (F32, 4, F64, 8, False),
    (F64, 8, F16, 2, False), (F64, 8, BF16, 2, False), (F64, 8, F32, 4, False),
])
def test_the_c_kind_rule(row_kind, esz, c_kind, c_esz, ok):
    """Any of the four kinds next to 16-bit rows; the rows' kind next to f32 / f64 rows."""
    rc, err = Call(row_kind, c_kind, esz, c_esz)()
    assert rc == -1
    assert err.endswith("NULL engine" if ok else "c kind must equal the kind of f32 / f64 rows"), err


def test_the_session_check_takes_the_16_bit_kinds():
    """fedagg_session_stage_check's kind check comes first (no session, no HIP call): fp16 and
    bf16 pass it, an integer kind does not."""
    lib = _native.load()
    mism = ctypes.c_uint64(7)
    assert lib.fedagg_session_stage_check(None, None, 2, 0, None, None, 0, 0, 3, ctypes.byref(mism)) == -1
    assert b"FEDAGG_F16, FEDAGG_BF16, FEDAGG_F32 or FEDAGG_F64" in lib.fedagg_last_error()
    for kind in (F16, BF16, F32, F64):
        assert lib.fedagg_session_stage_check(None, None, 2, 0, None, None, 0, 1, kind, ctypes.byref(mism)) == -1
        assert b"not element-aligned" in lib.fedagg_last_error(), kind
