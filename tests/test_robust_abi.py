"""libfedagg_robust.so (include/fedagg_robust.h) and the robust option without a GPU: exports, the
library's refusals (each before any HIP call) and every refusal on the way to it from Python."""

from pathlib import Path

import abi_header
import numpy as np
import pytest

from substrafl_amd import _native, _native_robust, wire

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "fedagg_robust.h"
A, D = 0x100000, 0x400000  # 16-B aligned fakes, never dereferenced
F32, BF16 = _native.FEDAGG_F32, _native.FEDAGG_BF16


def test_signatures_are_the_header():
    names = abi_header.declared_functions(HEADER, "fedagg_robust_")
    assert names == sorted(_native_robust.SIGNATURES) and len(names) == 4
    lib = _native_robust.load()
    assert all(hasattr(lib, n) for n in names)
    assert lib.fedagg_robust_abi_version() == _native_robust.ABI_VERSION == 1
    assert f"#define FEDAGG_ROBUST_MAX_K {_native_robust.MAX_K} " in HEADER.read_text() and _native_robust.MAX_K == 128
    tile, vec_f32, vec_bf16 = _native_robust.blocking()
    assert vec_f32 * 4 == 16 == vec_bf16 * 2 and tile % vec_bf16 == 0 and tile // vec_bf16 % 64 == 0
    assert lib.fedagg_robust_blocking(None, None, None) == 0


def test_refusals_have_their_own_text_and_need_no_gpu():
    """A refused call has made no HIP call, so the fake pointers are never dereferenced."""
    lib = _native_robust.load()

    def mean(rows=(A, A + 64), kind=F32, K=None, t=0, M=64, out=D, table=True):
        K = len(rows) if K is None else K
        return lib.fedagg_robust_mean(_native.ptr_array(list(rows)) if table else None, kind, K, t, M, out, None)

    cases = [
        (lambda: mean(K=0), b"K is outside [1, FEDAGG_ROBUST_MAX_K] (K=0)"),
        (lambda: mean(rows=[A] * 129), b"K is outside [1, FEDAGG_ROBUST_MAX_K] (K=129)"),
        (lambda: mean(t=-1), b"t must satisfy 0 <= 2 t < K (t=-1, K=2)"),
        (lambda: mean(t=1), b"t must satisfy 0 <= 2 t < K (t=1, K=2)"),
        (lambda: mean(kind=9), b"kind 9 is not FEDAGG_F32 / FEDAGG_BF16"),
        (lambda: mean(table=False), b"d_rows is NULL"),
        (lambda: mean(rows=(A, 0)), b"row 1 is NULL"),
        (lambda: mean(rows=(A + 2, A)), b"row 0 is not aligned to its element"),
        (lambda: mean(rows=(A, A + 1), kind=BF16), b"row 1 is not aligned to its element"),
        (lambda: mean(out=None), b"d_out is NULL"),
        (lambda: mean(out=D + 2), b"d_out is not 4-B aligned"),
    ]
    texts = []
    for call, needle in cases:
        rc, msg = call(), lib.fedagg_robust_last_error()
        assert rc == -1 and needle in msg, (rc, needle, msg)
        texts.append(msg)
    assert len(set(texts)) == len(texts)  # each refusal speaks for itself
    assert mean(M=0, out=None) == 0  # nothing to do is not an error, and launches nothing


def test_python_refusals_come_before_any_device_work(monkeypatch):
    """Neither the session, the device lock nor the library's loader is reached."""
    import standin_substrafl.strategies as ss

    from substrafl_amd import runtime, strategies
    from substrafl_amd.engine import AggregationEngine
    from substrafl_amd.integration import accelerate
    from substrafl_amd.multi_device import MultiDeviceEngine

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")

    for mod, name in ((runtime, "session"), (runtime, "device_lock"), (_native_robust, "load")):
        monkeypatch.setattr(mod, name, no_device)
    rng = np.random.default_rng(0)
    plain = [[rng.standard_normal(s).astype(np.float32) for s in [(4, 5), (1,)]] for _ in range(3)]
    cast = lambda dt: [[a.astype(dt) for a in p] for p in plain]  # noqa: E731
    eng, multi = AggregationEngine(device=0), MultiDeviceEngine.__new__(MultiDeviceEngine)
    for updates, text in [
        (cast(np.float16), "all fp32 or all wire.BF16"), (cast(np.float64), "all fp32 or all wire.BF16"),
        (cast(np.int32), "all fp32 or all wire.BF16"),
        ([plain[0], plain[1], [wire.float32_to_bf16(a) for a in plain[2]]], "all fp32 or all wire.BF16"),
        ([list(wire.float32_to_mxfp8(p)) for p in plain], "robust route has no MXFP8 path"),
        ([list(wire.float32_to_mxfp4(p)) for p in plain], "robust route has no MXFP4 path"),
        ([list(wire.float32_to_topk(p, 5)) for p in plain], "robust route has no top-k path"),
        ([plain[0]] * 129, "robust route takes up to 128 clients"),
    ]:
        with pytest.raises(NotImplementedError, match=text):
            eng.fedavg_robust(updates, "median")
    with pytest.raises(NotImplementedError, match="out-of-core route has no robust path"):
        AggregationEngine(device=0, max_bucket_bytes=64).fedavg_robust(plain, "trimmed_mean", 0.1)
    with pytest.raises(NotImplementedError, match="MultiDeviceEngine.*no robust route"):
        multi.fedavg_robust(plain, "median")

    class Algo:
        strategies = ["Federated Averaging", "Scaffold"]

    for make in (lambda **kw: strategies.FedAvg(algo=Algo(), **kw), lambda **kw: accelerate(ss.FedAvg, **kw)):
        with pytest.raises(NotImplementedError, match="robust route has no downlink='mxfp8' path"):
            make(robust="median", downlink="mxfp8")
        for bad in ("mean", "trimmed-mean", True):
            with pytest.raises(ValueError, match="robust must be None, 'trimmed_mean' or 'median'"):
                make(robust=bad)
        for bad in (None, True, "0.1", -0.1, 0.5):
            with pytest.raises(ValueError, match=r"needs trim, a number in \[0, 0.5\)"):
                make(robust="trimmed_mean", trim=bad)
        for kw in ({"robust": "median"}, {}):
            with pytest.raises(TypeError, match="trim is an option of robust='trimmed_mean'"):
                make(trim=0.1, **kw)
    for cls in (ss.Scaffold, ss.FedPCA, ss.NewtonRaphson):
        with pytest.raises(TypeError, match=f"robust is an option of FedAvg, not of {cls.__name__}"):
            accelerate(cls, robust="median")
    with pytest.raises(TypeError, match="robust"):
        strategies.Scaffold(algo=Algo(), robust="median")
    # recorded only when given: a class without the option is attribute for attribute what it was
    assert "robust" not in strategies.FedAvg(algo=Algo()).kwargs and not hasattr(accelerate(ss.FedAvg), "_fedagg_robust")
    given = strategies.FedAvg(algo=Algo(), robust="trimmed_mean", trim=0.25)
    assert given.kwargs["robust"] == "trimmed_mean" and given.kwargs["trim"] == 0.25
    assert accelerate(ss.FedAvg, robust="median")._fedagg_robust == "median"
