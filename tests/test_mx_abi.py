"""libfedagg_mx.so (include/fedagg_mx.h): the library exports what the header declares, the
binding's SIGNATURES are the header's prototypes, every refusal the header lists returns
FEDAGG_EINVAL with its own text before any HIP call (so none of this needs a GPU), the engine and
the client option refuse what the MXFP8 route does not carry before any device work, and an fp32
federation never maps the library."""

import ctypes
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from substrafl_amd import _native, _native_mx, wire

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "fedagg_mx.h"
F16, F32, F64, BF16 = _native.FEDAGG_F16, _native.FEDAGG_F32, _native.FEDAGG_F64, _native.FEDAGG_BF16


def _header_names():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\s*\*?\s*(fedagg_mx_[a-z0-9_]+)\s*\(", text, flags=re.M)))


def test_signatures_are_the_header():
    names = _header_names()
    assert names == sorted(_native_mx.SIGNATURES)
    assert {"fedagg_mx_abi_version", "fedagg_mx_last_error", "fedagg_mx_blocking", "fedagg_mx_fedavg_e4m3",
            "fedagg_mx_quantize"} == set(names)
    lib = _native_mx.load()
    for n in names:
        assert hasattr(lib, n), n
    # a library of its own: libfedagg.so's binding knows none of it
    assert not any(k.startswith("fedagg_mx") for k in _native.SIGNATURES)


def test_abi_version_and_blocking():
    lib = _native_mx.load()
    assert lib.fedagg_mx_abi_version() == _native_mx.ABI_VERSION == 1
    text = HEADER.read_text()
    assert "#define FEDAGG_MX_ABI_VERSION 1" in text
    assert _native_mx.MX_BLOCK == wire.MX_BLOCK == 32 and "#define FEDAGG_MX_BLOCK 32 " in text
    assert f"#define FEDAGG_MX_MAX_PAIRWISE_K {_native_mx.MAX_PAIRWISE_K} " in text
    tile, group = _native_mx.blocking()
    assert tile > 0 and tile % 512 == 0 and group >= 1  # whole 16-element vectors of whole waves
    assert lib.fedagg_mx_blocking(None, None) == 0


def _fedavg(lib, codes, scales, K=None, M=64, w=True, idx=None, P=0, out=0x300000):
    K = len(codes) if K is None and codes is not None else K
    return lib.fedagg_mx_fedavg_e4m3(_native.ptr_array(codes) if codes is not None else None,
                                     _native.ptr_array(scales) if scales is not None else None,
                                     (ctypes.c_float * max(1, K or 1))() if w else None, K, M,
                                     (ctypes.c_uint64 * max(1, len(idx)))(*idx) if idx is not None else None, P, out,
                                     None)


def test_every_refusal_has_its_own_text_and_needs_no_gpu():
    """Fake non-NULL pointers: a refused call has made no HIP call, so nothing is dereferenced."""
    lib = _native_mx.load()
    err = lib.fedagg_mx_last_error
    A, B = 0x100000, 0x200000  # 16-B aligned fakes
    texts = []

    def refused(rc, needle):
        assert rc == -1, needle
        msg = err()
        assert needle in msg, (needle, msg)
        texts.append(msg)

    refused(_fedavg(lib, [A], [B], K=0), b"K must be positive")
    refused(_fedavg(lib, [A], [B], K=-2), b"K must be positive")
    refused(_fedavg(lib, None, [B], K=1), b"d_codes is NULL")
    refused(_fedavg(lib, [A], None, K=1), b"d_scales is NULL")
    refused(_fedavg(lib, [A], [B], w=False), b"h_w is NULL")
    refused(_fedavg(lib, [A], [B], P=-1), b"P is negative")
    refused(_fedavg(lib, [A], [B], P=1), b"h_idx is NULL")
    refused(_fedavg(lib, [A, 0], [B, B]), b"code row 1 is NULL")
    for off in (1, 2, 4, 8):
        refused(_fedavg(lib, [A, A + off], [B, B]), b"code row 1 is not 16-B aligned")
    refused(_fedavg(lib, [A], [0]), b"scale row 0 is NULL")
    refused(_fedavg(lib, [A], [B], out=None), b"d_out is NULL")
    refused(_fedavg(lib, [A], [B], out=0x300002), b"d_out is not 4-B aligned")
    refused(_fedavg(lib, [A], [B], idx=[3, 64], P=2), b"index 1 is out of range")
    refused(_fedavg(lib, [A] * 257, [B] * 257, idx=[0], P=1), b"FEDAGG_MX_MAX_PAIRWISE_K")

    q = lib.fedagg_mx_quantize
    for kind in (F16, F64, 5, -1):
        refused(q(A, kind, 64, B, B + 64, None), b"is not FEDAGG_F32 / FEDAGG_BF16")
    refused(q(None, F32, 64, B, B + 64, None), b"d_x is NULL")
    refused(q(A + 2, F32, 64, B, B + 64, None), b"not aligned to its element size")
    refused(q(A + 1, BF16, 64, B, B + 64, None), b"not aligned to its element size")
    refused(q(A, F32, 64, None, B, None), b"d_codes is NULL")
    refused(q(A, BF16, 64, B, None, None), b"d_scales is NULL")
    assert len(set(texts)) >= 18  # each class of refusal speaks for itself

    # nothing to do is not an error, and launches nothing
    assert _fedavg(lib, [0], [0], M=0, out=None) == 0
    assert q(None, F32, 0, None, None, None) == 0


def test_check_raises_with_the_librarys_text():
    lib = _native_mx.load()
    rc = lib.fedagg_mx_quantize(None, F64, 1, None, None, None)
    with pytest.raises(_native.NativeLibraryError, match="mx_quantize failed .*FEDAGG_F32"):
        _native_mx.check(rc, "mx_quantize")


def _mx_update(shapes, seed):
    rng = np.random.default_rng(seed)
    codes, scales = wire.float32_to_mxfp8([rng.standard_normal(s).astype(np.float32) for s in shapes])
    return list(codes) + [scales]


def test_engine_refuses_before_any_device_work(monkeypatch):
    """None of these reaches the session or the device lock (both are replaced by a function that
    fails the test), so the test needs no GPU."""
    from substrafl_amd import handoff, runtime
    from substrafl_amd.engine import AggregationEngine
    from substrafl_amd.multi_device import MultiDeviceEngine

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(runtime, "session", no_device)
    monkeypatch.setattr(runtime, "device_lock", no_device)
    shapes = [(4, 5), (1,), (7,)]
    mx = [_mx_update(shapes, k) for k in range(3)]
    rng = np.random.default_rng(0)
    plain = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    eng = AggregationEngine(device=0)
    ns = [1, 2, 3]
    for entry in (eng.fedavg_mxfp8, eng.fedavg_routed):
        with pytest.raises(NotImplementedError, match="2 of 3 clients sent MXFP8"):
            entry([mx[0], plain, mx[2]], ns)  # one fp32 client among MXFP8 ones
        with pytest.raises(ValueError, match="scale array is missing"):
            entry([m[:-1] for m in mx], ns)
        with pytest.raises(ValueError, match="scale array is missing"):
            entry([m[:-1] + [m[-1]["e8m0"]] for m in mx], ns)  # plain uint8 scales: the wrong dtype
        with pytest.raises(ValueError, match="need a 1-D scale array of 1 bytes"):
            entry([m[:-1] + [np.zeros(2, wire.E8M0)] for m in mx], ns)
        with pytest.raises(ValueError, match="must have dtype wire.E4M3"):
            entry([[plain[0]] + m[1:] for m in mx], ns)
        with pytest.raises(ValueError, match="shapes differ"):
            entry([mx[0], _mx_update([(5, 4), (1,), (7,)], 9), mx[2]], ns)
        with pytest.raises(NotImplementedError, match="numel == 1 layers up to 256 clients"):
            entry([mx[0]] * 257, [1] * 257)
    monkeypatch.setattr(handoff, "_enabled", True)
    with pytest.raises(NotImplementedError, match="hand-off has no MXFP8 route"):
        eng.fedavg_routed(mx, ns)
    monkeypatch.setattr(handoff, "_enabled", False)

    multi = MultiDeviceEngine.__new__(MultiDeviceEngine)  # device="all": no constructor work needed to refuse
    for entry in (multi.fedavg_routed,):
        with pytest.raises(NotImplementedError, match="MultiDeviceEngine.fedavg_routed.*no MXFP8 path"):
            entry(mx, ns)


def test_client_option_refusals():
    import torch
    from standin_substrafl.algorithms.pytorch import TorchFedAvgAlgo, TorchScaffoldAlgo
    from standin_substrafl.algorithms.pytorch.torch_newton_raphson_algo import TorchNewtonRaphsonAlgo

    from substrafl_amd.algorithms import weight_manager as wm
    from substrafl_amd.integration import accelerate_algo

    for ok in (True, False, "mxfp8"):
        cls = accelerate_algo(TorchFedAvgAlgo, wire=ok)
        assert cls._fedagg_mxfp8 is (ok == "mxfp8") and cls._fedagg_wire is bool(ok)
    for bad in ("bf16", "MXFP8", ""):
        with pytest.raises(ValueError, match="wire must be True, False or 'mxfp8'"):
            accelerate_algo(TorchFedAvgAlgo, wire=bad)
    for cls in (TorchScaffoldAlgo, TorchNewtonRaphsonAlgo):
        with pytest.raises(TypeError, match="wire='mxfp8' is an option of TorchFedAvgAlgo"):
            accelerate_algo(cls, wire="mxfp8")
        accelerate_algo(cls, wire=True)
    # no host quantiser: CPU tensors, fp16 and fp64 are refused before the library is loaded
    for dt in (torch.float32, torch.float16, torch.float64):
        with pytest.raises(NotImplementedError, match="wire='mxfp8'"):
            wm.export_mxfp8([torch.zeros(8, dtype=dt)])


def test_an_fp32_federation_never_maps_the_library():
    """A fresh process: the wire module, the engine and the strategies are imported, fp32 and
    wire.BF16 updates are validated and routed (up to the device, which this test does not need),
    and libfedagg_mx.so is never loaded."""
    code = (
        "import sys; sys.path[:0] = [%r, %r]\n"
        "import numpy as np\n"
        "from substrafl_amd import _native, _native_mx, wire, engine, runtime\n"
        "from substrafl_amd.strategies import FedAvg, Scaffold\n"
        "from substrafl_amd.strategies.fed_avg import weighted_average\n"
        "from substrafl_amd.schemas import FedAvgSharedState\n"
        "_native.load()\n"
        "class Reached(Exception): pass\n"
        "def stop(*a, **k): raise Reached()\n"
        "engine.AggregationEngine.fedavg = stop\n"
        "engine.AggregationEngine._fedavg_bf16_out_of_core = lambda *a, **k: None\n"
        "for dt in (np.float32, wire.BF16):\n"
        "    pu = [np.zeros((3, 2), np.float32).view(np.uint8)[:, :2 * np.dtype(dt).itemsize].copy().view(dt)]\n"
        "    states = [FedAvgSharedState(n_samples=2, parameters_update=pu) for _ in range(2)]\n"
        "    try:\n"
        "        weighted_average(states, 'FedAvgSharedState', 0)\n"
        "        raise SystemExit('the fp32 route was not taken')\n"
        "    except Reached:\n"
        "        pass\n"
        "assert not _native_mx.loaded()\n"
        "assert 'libfedagg_mx' not in open('/proc/self/maps').read()\n"
        "assert 'libfedagg.so' in open('/proc/self/maps').read()\n" % (str(ROOT), str(ROOT / "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def demo_command(exe):
    """The compile line of tests/c/fedavg_mx_demo.c (also used by the GPU test that runs it)."""
    libdir = _native_mx.LIB_PATH.parent
    return ["gcc", "-O2", "-ffp-contract=off", "-Wall", "-Werror", f"-I{ROOT / 'include'}",
            str(ROOT / "tests" / "c" / "fedavg_mx_demo.c"), f"-L{libdir}", "-lfedagg_mx", "-lfedagg", "-lm",
            f"-Wl,-rpath,{libdir}", "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(exe)]


def test_the_demo_compiles_against_the_header(tmp_path):
    import shutil

    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    exe = tmp_path / "fedavg_mx_demo"
    subprocess.run(demo_command(exe), check=True)
    assert exe.exists()
