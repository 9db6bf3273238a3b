"""libfedagg_mxef.so (include/fedagg_mxef.h) without a GPU: the library exports what the header
declares and the binding's SIGNATURES are the header's prototypes, every refusal returns
FEDAGG_EINVAL with its own text before any HIP call, ``error_feedback`` is refused where the MXFP8
wire is not, and a class without it never imports the binding."""

import subprocess
import sys
from pathlib import Path

import abi_header
import pytest

from substrafl_amd import _native, _native_mxef

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "fedagg_mxef.h"
F32, BF16 = _native.FEDAGG_F32, _native.FEDAGG_BF16


def test_signatures_are_the_header_and_the_abi_is_pinned():
    text = HEADER.read_text()
    names = abi_header.declared_functions(HEADER, "fedagg_mxef_")
    assert names == sorted(_native_mxef.SIGNATURES) == ["fedagg_mxef_abi_version", "fedagg_mxef_blocking",
                                                        "fedagg_mxef_last_error", "fedagg_mxef_quantize"]
    lib = _native_mxef.load()
    assert all(hasattr(lib, n) for n in names)
    assert lib.fedagg_mxef_abi_version() == _native_mxef.ABI_VERSION == 1 and "#define FEDAGG_MXEF_ABI_VERSION 1" in text
    lane, tile, second = _native_mxef.blocking()
    assert lane == 8 and tile % 512 == 0 and second % tile == 0  # a quarter block per lane, whole waves per step
    assert lib.fedagg_mxef_blocking(None, None, None) == 0


def test_every_refusal_has_its_own_text_and_needs_no_gpu():
    """Fake non-NULL pointers: a refused call has made no HIP call, so nothing is dereferenced."""
    lib = _native_mxef.load()
    q = lib.fedagg_mxef_quantize
    X, R, C, S = 0x100000, 0x200000, 0x300000, 0x400000
    cases = [((X, 0, 64, R, C, S), b"kind 0 is not FEDAGG_F32 / FEDAGG_BF16"),
             ((X, _native.FEDAGG_F64, 64, R, C, S), b"is not FEDAGG_F32 / FEDAGG_BF16"),
             ((None, F32, 64, R, C, S), b"d_x is NULL"), ((X, F32, 64, None, C, S), b"d_res is NULL"),
             ((X, F32, 64, R, None, S), b"d_codes is NULL"), ((X, BF16, 64, R, C, None), b"d_scales is NULL"),
             ((X + 2, F32, 64, R, C, S), b"d_x is not aligned"), ((X + 1, BF16, 64, R, C, S), b"d_x is not aligned"),
             ((X, F32, 64, R + 2, C, S), b"d_res is not 4-B aligned"),
             ((X, F32, 64, X + 252, C, S), b"d_res overlaps d_x"), ((X, BF16, 64, X - 252, C, S), b"d_res overlaps d_x"),
             ((X, F32, 64, R, R + 252, S), b"d_res overlaps d_codes"), ((X, F32, 64, R, C, R - 1), b"d_res overlaps d_scales"),
             ((X, F32, (1 << 44) + 1, R, C, S), b"M is too large")]
    texts = set()
    for args, needle in cases:
        assert q(*args, None) == -1, needle
        assert needle in lib.fedagg_mxef_last_error(), (needle, lib.fedagg_mxef_last_error())
        texts.add(lib.fedagg_mxef_last_error())
    assert len(texts) >= 12
    assert q(None, F32, 0, None, None, None, None) == 0  # nothing to do is not an error, and launches nothing
    with pytest.raises(_native.NativeLibraryError, match="mxef_quantize failed .*d_x is NULL"):
        _native_mxef.quantize_ef(0, F32, 8, R, C, S, 0)


def test_error_feedback_is_an_option_of_the_mxfp8_wire():
    from standin_substrafl.algorithms.pytorch import TorchFedAvgAlgo, TorchScaffoldAlgo
    from standin_substrafl.algorithms.pytorch.torch_newton_raphson_algo import TorchNewtonRaphsonAlgo

    from substrafl_amd.integration import accelerate_algo

    for cls, wire in ((TorchFedAvgAlgo, False), (TorchFedAvgAlgo, True), (TorchScaffoldAlgo, False),
                      (TorchNewtonRaphsonAlgo, False)):
        with pytest.raises(TypeError, match="error_feedback"):
            accelerate_algo(cls, wire=wire, error_feedback=True)
    with pytest.raises(TypeError):
        accelerate_algo(TorchScaffoldAlgo, wire="mxfp8", error_feedback=True)
    on, off = (accelerate_algo(TorchFedAvgAlgo, wire="mxfp8", error_feedback=ef) for ef in (True, False))
    assert on._fedagg_error_feedback is True and on._fedagg_mx_residual is None
    added = {"_fedagg_error_feedback", "_fedagg_mx_residual", "_get_state_to_save", "_update_from_checkpoint"}
    assert set(vars(on)) - set(vars(off)) == added and not added & set(vars(off))


def test_a_class_without_error_feedback_never_imports_the_binding():
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from standin_substrafl.algorithms.pytorch import TorchFedAvgAlgo\n"
            "from substrafl_amd.integration import accelerate_algo\n"
            "accelerate_algo(TorchFedAvgAlgo, wire='mxfp8')\n"
            "assert 'substrafl_amd._native_mxef' not in sys.modules\n"
            "assert 'libfedagg_mxef' not in open('/proc/self/maps').read()\n" % (str(ROOT), str(ROOT / "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
