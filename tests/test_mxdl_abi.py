"""libfedagg_mxdl.so (include/fedagg_mxdl.h) without a GPU: exports, refusals (library, option,
engine, client: all before any device work), and no mapping of the library without ``downlink``."""

import ctypes
import subprocess
import sys
from pathlib import Path

import abi_header
import numpy as np
import pytest

from substrafl_amd import _native, _native_mxdl, wire

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "fedagg_mxdl.h"
A, B, C, D = 0x100000, 0x200000, 0x300000, 0x400000  # 16-B aligned fakes, never dereferenced


def test_signatures_are_the_header():
    names = abi_header.declared_functions(HEADER, "fedagg_mxdl_")
    assert names == sorted(_native_mxdl.SIGNATURES) and len(names) == 6
    lib = _native_mxdl.load()
    assert all(hasattr(lib, n) for n in names)
    assert lib.fedagg_mxdl_abi_version() == _native_mxdl.ABI_VERSION == 1
    text = HEADER.read_text()
    assert f"#define FEDAGG_MXDL_KMAX {_native_mxdl.KMAX} " in text and _native_mxdl.KMAX == 128
    assert "#define FEDAGG_MXDL_E4M3 0 " in text and "#define FEDAGG_MXDL_E2M1 1 " in text
    tile, lane, group = _native_mxdl.blocking()
    assert lane == 16 and tile % (64 * lane) == 0 and group >= 1  # half a scale block per lane, whole waves
    assert lib.fedagg_mxdl_blocking(None, None, None) == 0


def _fedavg(lib, kind=0, codes=(A,), scales=(B,), K=None, M=64, w=True, idx=None, P=0, oc=C, os_=D):
    K = len(codes) if K is None else K
    return lib.fedagg_mxdl_fedavg(kind, _native.ptr_array(list(codes)) if codes else None,
                                  _native.ptr_array(list(scales)) if scales else None,
                                  (ctypes.c_float * max(1, K))() if w else None, K, M,
                                  (ctypes.c_uint64 * len(idx))(*idx) if idx else None, P, oc, os_, None)


def _increment(lib, ptrs=(A,), numel=(64,), L=None, codes=B, scales=C, M=64):
    L = len(ptrs) if L is None else L
    return lib.fedagg_mxdl_increment(_native.ptr_array(list(ptrs)) if ptrs else None,
                                     (ctypes.c_uint64 * len(numel))(*numel) if numel else None, L, codes, scales, M,
                                     1.0, None)


def test_every_refusal_has_its_own_text_and_needs_no_gpu():
    """A refused call has made no HIP call, so the fake pointers are never dereferenced."""
    lib = _native_mxdl.load()
    dec = lib.fedagg_mxdl_decode
    cases = [
        (lambda: _fedavg(lib, kind=2), b"in_kind 2 is not"),
        (lambda: _fedavg(lib, K=0), b"K must be positive"),
        (lambda: _fedavg(lib, codes=[A] * 129, scales=[B] * 129), b"at most FEDAGG_MXDL_KMAX clients"),
        (lambda: _fedavg(lib, codes=None, K=1), b"d_codes is NULL"),
        (lambda: _fedavg(lib, scales=None), b"d_scales is NULL"),
        (lambda: _fedavg(lib, w=False), b"h_w is NULL"),
        (lambda: _fedavg(lib, P=-1), b"P is negative"),
        (lambda: _fedavg(lib, P=1), b"h_idx is NULL"),
        (lambda: _fedavg(lib, M=1 << 45), b"M is too large"),
        (lambda: _fedavg(lib, codes=[A, 0], scales=[B, B]), b"code row 1 is NULL"),
        (lambda: _fedavg(lib, kind=1, codes=[A, A + 8], scales=[B, B]), b"code row 1 is not 16-B aligned"),
        (lambda: _fedavg(lib, scales=[0]), b"scale row 0 is NULL"),
        (lambda: _fedavg(lib, oc=None), b"d_out_codes is NULL"),
        (lambda: _fedavg(lib, os_=None), b"d_out_scales is NULL"),
        (lambda: _fedavg(lib, idx=[3, 64], P=2), b"index 1 is out of range"),
        (lambda: _increment(lib, L=-1), b"L is negative"),
        (lambda: _increment(lib, M=1 << 45), b"increment: M is too large"),
        (lambda: _increment(lib, ptrs=[A, B], numel=[1 << 45, 1]), b"tensor 0 is too large"),
        (lambda: dec(A, B, 1 << 45, C, None), b"decode: M is too large"),
        (lambda: _increment(lib, ptrs=None, L=1), b"d_layers is NULL"),
        (lambda: _increment(lib, numel=None), b"numel is NULL"),
        (lambda: _increment(lib, ptrs=[A, 0], numel=[60, 4]), b"tensor 1 is NULL"),
        (lambda: _increment(lib, ptrs=[A + 2]), b"tensor 0 is not 4-B aligned"),
        (lambda: _increment(lib, numel=[63]), b"hold 63 elements, the update 64"),
        (lambda: _increment(lib, codes=None), b"d_codes is NULL"),
        (lambda: _increment(lib, scales=None), b"d_scales is NULL"),
        (lambda: dec(None, B, 64, C, None), b"d_codes is NULL"),
        (lambda: dec(A, None, 64, C, None), b"d_scales is NULL"),
        (lambda: dec(A, B, 64, None, None), b"d_out is NULL"),
        (lambda: dec(A, B, 64, C + 2, None), b"d_out is not 4-B aligned"),
    ]
    texts = []
    for call, needle in cases:
        rc, msg = call(), lib.fedagg_mxdl_last_error()
        assert rc == -1 and needle in msg, (rc, needle, msg)
        texts.append(msg)
    assert len(set(texts)) == len(texts)  # each refusal speaks for itself
    # nothing to do is not an error, and launches nothing
    assert _fedavg(lib, M=0, oc=None, os_=None) == 0 and _increment(lib, ptrs=[0], numel=[0], M=0) == 0
    assert dec(None, None, 0, None, None) == 0


def test_the_option_where_it_does_not_apply():
    import standin_substrafl.strategies as ss

    from substrafl_amd import strategies
    from substrafl_amd.integration import accelerate

    class _Algo:
        strategies = ["Federated Averaging", "Scaffold", "Federated PCA"]

    assert strategies.FedAvg(algo=_Algo(), downlink="mxfp8").kwargs["downlink"] == "mxfp8"
    assert "downlink" not in strategies.FedAvg(algo=_Algo()).kwargs  # the default changes nothing
    assert accelerate(ss.FedAvg, downlink="mxfp8")._fedagg_downlink == "mxfp8"
    for bad in ("mxfp4", "MXFP8", ""):
        for make in (lambda: strategies.FedAvg(algo=_Algo(), downlink=bad), lambda: accelerate(ss.FedAvg, downlink=bad)):
            with pytest.raises(ValueError, match="downlink must be None or 'mxfp8'"):
                make()
    for name in ("Scaffold", "FedPCA", "NewtonRaphson"):
        with pytest.raises(TypeError, match="downlink"):
            accelerate(getattr(ss, name), downlink="mxfp8")
        if hasattr(strategies, name):
            with pytest.raises(TypeError, match="downlink"):
                getattr(strategies, name)(algo=_Algo(), downlink="mxfp8")


def test_refusals_come_before_any_device_work(monkeypatch):
    """Neither the session, the device lock nor the library's loader is reached (each is replaced by
    a function that fails the test), so the test needs no GPU."""
    import torch

    from substrafl_amd import handoff, runtime
    from substrafl_amd.algorithms import weight_manager as wm
    from substrafl_amd.engine import AggregationEngine
    from substrafl_amd.multi_device import MultiDeviceEngine

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")

    for mod, name in ((runtime, "session"), (runtime, "device_lock"), (_native_mxdl, "load")):
        monkeypatch.setattr(mod, name, no_device)
    rng = np.random.default_rng(0)
    plain = [[rng.standard_normal(s).astype(np.float32) for s in [(4, 5), (1,), (7,)]] for _ in range(3)]
    mx = [[*c, s] for c, s in map(wire.float32_to_mxfp8, plain)]
    eng, multi, ns = AggregationEngine(device=0), MultiDeviceEngine.__new__(MultiDeviceEngine), [1, 2, 3]
    handoff_on = lambda: monkeypatch.setattr(handoff, "_enabled", True)  # noqa: E731
    for call, exc, text in [
        (lambda: eng.fedavg_routed(plain, ns, downlink="mxfp8"), NotImplementedError, "downlink='mxfp8'.*sent none"),
        (lambda: eng.fedavg_mxfp8(mx, ns, downlink="bf16"), ValueError, "downlink must be None or 'mxfp8'"),
        (lambda: eng.fedavg_routed([mx[0], plain[1], mx[2]], ns, downlink="mxfp8"), NotImplementedError, "2 of 3 clients"),
        (lambda: eng.fedavg_routed([mx[0]] * 257, [1] * 257, downlink="mxfp8"), NotImplementedError, "up to 256 clients"),
        (lambda: multi.fedavg_routed(mx, ns, downlink="mxfp8"), NotImplementedError, "no MXFP8 path"),
        (lambda: multi.fedavg_routed(plain, ns, downlink="mxfp8"), NotImplementedError, "no downlink='mxfp8' route"),
        (lambda: (handoff_on(), eng.fedavg_routed(mx, ns, downlink="mxfp8")), NotImplementedError, "hand-off has no MXFP8"),
    ]:
        with pytest.raises(exc, match=text):
            call()
    monkeypatch.setattr(handoff, "_enabled", False)

    # the client: shapes and the scale count are checked, then CPU, fp16 and fp64 models are refused
    def model(dt=torch.float32):
        return torch.nn.Sequential(torch.nn.Linear(5, 4), torch.nn.Linear(7, 1, bias=False)).to(dt)

    c, s = wire.float32_to_mxfp8([np.ones((4, 5), np.float32), np.ones(4, np.float32), np.ones((1, 7), np.float32)])
    upd = [*c, s]
    inc = lambda m, u: wm.increment_parameters(m, u, with_batch_norm_parameters=False)  # noqa: E731
    for dt in (torch.float32, torch.float16, torch.float64):
        with pytest.raises(NotImplementedError, match="downlink='mxfp8'"):
            inc(model(dt), upd)
    for bad, text in [(upd[1:], "2 layers for 3 model parameters"),
                      ([upd[0], upd[1], upd[2].reshape(7, 1), upd[3]], r"\(7, 1\)"),
                      (upd[:-1] + [np.zeros(2, wire.E8M0)], "need a 1-D scale array of 1 bytes"),
                      ([np.ones((4, 5), np.float32)] + upd[1:], "expected wire.E4M3 layers")]:
        with pytest.raises(ValueError, match=text):
            inc(model(), bad)


def test_a_federation_without_downlink_never_maps_the_library():
    """A fresh process: MXFP8 updates are routed up to the device (not needed here) without ``downlink``."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import numpy as np\n"
            "from substrafl_amd import _native, _native_mxdl, wire, engine\n"
            "from substrafl_amd.strategies import FedAvg\n"
            "from substrafl_amd.schemas import FedAvgSharedState\n"
            "_native.load()\n"
            "engine.AggregationEngine._fedavg_mxfp8 = lambda *a, **k: sys.exit(7)\n"
            "class A: strategies = ['Federated Averaging']\n"
            "c, s = wire.float32_to_mxfp8([np.ones((3, 2), np.float32)])\n"
            "states = [FedAvgSharedState(n_samples=2, parameters_update=[*c, s]) for _ in range(2)]\n"
            "mapped = lambda: _native_mxdl.loaded() or 'libfedagg_mxdl' in open('/proc/self/maps').read()\n"
            "import atexit; atexit.register(lambda: mapped() and sys.stderr.write('LOADED'))\n"
            "FedAvg(algo=A(), device=0).avg_shared_states(shared_states=states, _skip=True)\n"
            % (str(ROOT), str(ROOT / "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 7 and "LOADED" not in r.stderr, r.stderr[-2000:]  # 7: the MXFP8 route was reached
