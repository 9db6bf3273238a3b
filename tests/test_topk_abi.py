"""libfedagg_topk.so (include/fedagg_topk.h) and the top-k wire without a GPU: exports, the NumPy
rule, refusals (library, option, engine, client: all before any device work), and no mapping of the
library without the option."""

import ctypes
import subprocess
import sys
from pathlib import Path

import abi_header
import numpy as np
import pytest

from substrafl_amd import _native, _native_topk, wire

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "fedagg_topk.h"
A, B, C, D = 0x100000, 0x200000, 0x300000, 0x400000  # 16-B aligned fakes, never dereferenced
F32 = _native.FEDAGG_F32


def test_signatures_are_the_header():
    names = abi_header.declared_functions(HEADER, "fedagg_topk_")
    assert names == sorted(_native_topk.SIGNATURES) and len(names) == 7
    lib = _native_topk.load()
    assert all(hasattr(lib, n) for n in names)
    assert lib.fedagg_topk_abi_version() == _native_topk.ABI_VERSION == 1
    text = HEADER.read_text()
    assert f"#define FEDAGG_TOPK_KMAX {_native_topk.KMAX} " in text and _native_topk.KMAX == 128
    assert f"#define FEDAGG_TOPK_STATE_WORDS {_native_topk.STATE_WORDS} " in text
    tile, sub, group, threads = _native_topk.blocking()
    assert tile % (4 * threads) == 0 and sub % 256 == 0 and group >= 2 and threads % 64 == 0
    assert sub == _native_topk.SUB_TILE and lib.fedagg_topk_blocking(None, None, None, None) == 0
    for M, K in ((1, 1), (sub, 3), (5 * sub + 1, 128)):
        sel, fed = _native_topk.workspace(M, K)
        assert fed == _native_topk.fedavg_ws_bytes(M, K) >= (-(-M // sub) + 1) * K * 4 and sel >= 4 * (4096 + -(-M // tile))


@pytest.mark.parametrize("k", [1, 7, 100])
def test_wire_round_trip_and_the_rule(k):
    rng = np.random.default_rng(k)
    layers = [rng.standard_normal(s).astype(np.float32) for s in [(9, 11), (1,), ()]]
    flat = np.concatenate([a.reshape(-1) for a in layers])
    idx, val, table = wire.float32_to_topk(layers, k)
    assert idx.dtype == wire.TOPK_IDX and val.dtype == wire.TOPK_VAL and idx.size == val.size == k  # no ties here
    assert wire.is_topk([idx, val, table]) and wire.has_topk([idx]) and not wire.has_topk(layers)
    assert wire.topk_check([idx, val, table]) == flat.size == 101
    kept = np.zeros(flat.size, bool)
    kept[idx["topk_idx"]] = True
    assert np.abs(flat[kept]).min() >= np.abs(flat[~kept]).max(initial=0)
    dense = wire.topk_to_float32(idx, val, table)
    assert [d.shape for d in dense] == [a.shape for a in layers]
    got = np.concatenate([d.reshape(-1) for d in dense]).view(np.uint32)
    assert np.array_equal(got, np.where(kept, flat, np.float32(0)).view(np.uint32))
    for arr in (idx, val):
        with pytest.raises(TypeError):  # NumPy refuses arithmetic on the structured dtypes
            arr + arr


def test_ties_zeros_and_non_finite_values():
    z = np.zeros(8, np.float32)
    x = np.array([1, -2, 2, 0, -0.0, 1, 2, -1], np.float32)
    idx, val, res = wire.topk_error_feedback(x, z, 2)  # the threshold falls on a tie: all three 2s go
    assert idx["topk_idx"].tolist() == [1, 2, 6] and val["topk_f32"].tolist() == [-2, 2, 2]
    assert res.tolist() == [1, 0, 0, 0, 0, 1, 0, -1]
    idx, val, res = wire.topk_error_feedback(x, z, 8)  # fewer than k non-zeros: zeros are never sent
    assert idx["topk_idx"].tolist() == [0, 1, 2, 5, 6, 7] and not res.any()
    idx, val, res = wire.topk_error_feedback(z, z, 3)
    assert idx.size == 0 and val.size == 0 and not res.any()
    x = np.array([1, np.nan, np.inf, -np.inf, 3, 0.5], np.float32)
    idx, val, res = wire.topk_error_feedback(x, np.zeros(6, np.float32), 1)  # NaN sorts above Inf
    assert idx["topk_idx"].tolist() == [1] and np.isnan(val["topk_f32"][0])
    assert res.tolist() == [1, 0, 0, 0, 3, 0.5]  # a non-finite residual is dropped, sent or not
    idx, val, res = wire.topk_error_feedback(x, np.float32(0.25) * np.ones(6, np.float32), 4)
    assert idx["topk_idx"].tolist() == [1, 2, 3, 4] and val["topk_f32"][3] == 3.25 and res.tolist() == [1.25, 0, 0, 0, 0, .75]


def test_refusals_have_their_own_text_and_need_no_gpu():
    """A refused call has made no HIP call, so the fake pointers are never dereferenced."""
    lib = _native_topk.load()
    sel, cmp_ = lib.fedagg_topk_select, lib.fedagg_topk_compact
    big = 1 << 20

    def fedavg(idx=(A,), val=(B,), nnz=(4,), K=None, M=64, w=True, pw=None, P=0, ws=C, wsb=big, out=D):
        K = len(idx) if K is None else K
        return lib.fedagg_topk_fedavg(_native.ptr_array(list(idx)) if idx else None,
                                      _native.ptr_array(list(val)) if val else None,
                                      (ctypes.c_uint64 * len(nnz))(*nnz) if nnz else None,
                                      (ctypes.c_float * max(1, K))() if w else None, K, M,
                                      (ctypes.c_uint64 * len(pw))(*pw) if pw else None, P, ws, wsb, out, None)

    cases = [
        (lambda: sel(9, A, B, 64, 1, C, big, D, None), b"in_kind 9 is not"),
        (lambda: sel(F32, A, B, 1 << 32, 1, C, big, D, None), b"select: M must be below 2^32"),
        (lambda: sel(F32, A, B, 64, 0, C, big, D, None), b"k is outside [1, M] (k=0"),
        (lambda: sel(F32, A, B, 64, 65, C, big, D, None), b"k is outside [1, M] (k=65"),
        (lambda: sel(F32, None, B, 64, 1, C, big, D, None), b"select: d_x is NULL"),
        (lambda: sel(F32, A, None, 64, 1, C, big, D, None), b"select: d_res is NULL"),
        (lambda: sel(F32, A, B, 64, 1, None, big, D, None), b"select: d_ws is NULL"),
        (lambda: sel(F32, A, B, 64, 1, C, big, None, None), b"select: d_state is NULL"),
        (lambda: sel(_native.FEDAGG_BF16, A + 1, B, 64, 1, C, big, D, None), b"d_x is not aligned"),
        (lambda: sel(F32, A, B, 64, 1, C + 4, big, D, None), b"select: d_ws is not 16-B aligned"),
        (lambda: sel(F32, A, A + 128, 64, 1, C, big, D, None), b"d_res overlaps d_x"),
        (lambda: sel(F32, A, B, 64, 1, C, 64, D, None), b"ws_bytes is 64, the selection needs"),
        (lambda: cmp_(B, 64, C, D, 65, A, A, None), b"nnz is above M"),
        (lambda: cmp_(None, 64, C, D, 1, A, A, None), b"compact: d_res is NULL"),
        (lambda: cmp_(B, 64, C, None, 1, A, A, None), b"compact: d_state is NULL"),
        (lambda: cmp_(B, 64, C, D, 1, None, A, None), b"d_idx is NULL with nnz > 0"),
        (lambda: cmp_(B, 64, C, D, 1, A, A + 2, None), b"d_val is not 4-B aligned"),
        (lambda: fedavg(K=0), b"K must be positive"),
        (lambda: fedavg(idx=[A] * 129, val=[B] * 129, nnz=[1] * 129), b"at most FEDAGG_TOPK_KMAX clients"),
        (lambda: fedavg(idx=None, K=1), b"fedavg: d_idx is NULL"),
        (lambda: fedavg(nnz=None), b"fedavg: nnz is NULL"),
        (lambda: fedavg(w=False), b"h_w is NULL"),
        (lambda: fedavg(P=1), b"h_pw_idx is NULL"),
        (lambda: fedavg(M=1 << 32), b"fedavg: M must be below 2^32"),
        (lambda: fedavg(nnz=[65]), b"row 0 holds more than M entries"),
        (lambda: fedavg(idx=[A, 0], val=[B, B], nnz=[1, 1]), b"index row 1 is NULL"),
        (lambda: fedavg(val=[B + 2]), b"value row 0 is not 4-B aligned"),
        (lambda: fedavg(ws=None), b"fedavg: d_ws is NULL"),
        (lambda: fedavg(wsb=4), b"ws_bytes is 4, the bounds need"),
        (lambda: fedavg(out=D + 2), b"d_out is not 4-B aligned"),
        (lambda: fedavg(pw=[3, 64], P=2), b"index 1 is out of range"),
        (lambda: lib.fedagg_topk_workspace(1 << 32, 1, None, None), b"workspace: M must be below 2^32"),
        (lambda: lib.fedagg_topk_workspace(64, 129, None, None), b"K is outside [0, FEDAGG_TOPK_KMAX]"),
    ]
    texts = []
    for call, needle in cases:
        rc, msg = call(), lib.fedagg_topk_last_error()
        assert rc == -1 and needle in msg, (rc, needle, msg)
        texts.append(msg)
    assert len(set(texts)) == len(texts)  # each refusal speaks for itself
    # nothing to do is not an error, and launches nothing; an empty row needs no pointers
    assert sel(F32, None, None, 0, 0, None, 0, None, None) == 0 and cmp_(None, 0, None, None, 0, None, None, None) == 0
    assert fedavg(M=0, ws=None, out=None) == 0


def test_refusals_come_before_any_device_work(monkeypatch):
    """Neither the session, the device lock nor the library's loader is reached (each is replaced by
    a function that fails the test), so the test needs no GPU."""
    import torch
    from standin_substrafl.algorithms.pytorch import TorchFedAvgAlgo, TorchScaffoldAlgo
    from standin_substrafl.algorithms.pytorch.torch_newton_raphson_algo import TorchNewtonRaphsonAlgo

    from substrafl_amd import handoff, runtime
    from substrafl_amd.algorithms import weight_manager as wm
    from substrafl_amd.engine import AggregationEngine, reject_mxfp8
    from substrafl_amd.integration import accelerate_algo
    from substrafl_amd.multi_device import MultiDeviceEngine

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")

    for mod, name in ((runtime, "session"), (runtime, "device_lock"), (_native_topk, "load")):
        monkeypatch.setattr(mod, name, no_device)
    rng = np.random.default_rng(0)
    shapes = [(4, 5), (1,), (7,)]
    plain = [[rng.standard_normal(s).astype(np.float32) for s in shapes] for _ in range(3)]
    tk = [list(wire.float32_to_topk(p, 5)) for p in plain]
    other = list(wire.float32_to_topk([a.T for a in plain[0]], 5))
    past = np.array([1, 2, 3, 4, 28], np.uint32).view(wire.TOPK_IDX)
    eng, multi, ns = AggregationEngine(device=0), MultiDeviceEngine.__new__(MultiDeviceEngine), [1, 2, 3]
    small = AggregationEngine(device=0, max_bucket_bytes=64)
    for entry in (eng.fedavg_topk, eng.fedavg_routed, eng.fedavg):
        for call, exc, text in [
            (lambda: entry([tk[0], plain[1], tk[2]], ns), NotImplementedError, "2 of 3 clients sent top-k"),
            (lambda: entry([tk[0]] * 129, [1] * 129), NotImplementedError, "top-k route takes up to 128 clients"),
            (lambda: entry([tk[0], other, tk[2]], ns), ValueError, "shape tables differ"),
            (lambda: entry([[t[0], t[1][:4], t[2]] for t in tk], ns), ValueError, "1-D of one length"),
            (lambda: entry([[t[0][::-1], t[1], t[2]] for t in tk], ns), ValueError, "not strictly ascending"),
            (lambda: entry([[np.repeat(t[0][:1], 5), t[1], t[2]] for t in tk], ns), ValueError, "not strictly ascending"),
            (lambda: entry([[past, t[1], t[2]] for t in tk], ns), ValueError, "index 28 is not below the 28 elements"),
            (lambda: entry([[t[0], t[1]["topk_f32"], t[2]] for t in tk], ns), ValueError, r"expected \[indices"),
        ]:
            with pytest.raises(exc, match=text):
                call()
    with pytest.raises(NotImplementedError, match="downlink='mxfp8'.*sent none"):
        eng.fedavg_routed(tk, ns, downlink="mxfp8")
    with pytest.raises(NotImplementedError, match="out-of-core route has no top-k path"):
        small.fedavg_routed(tk, ns)
    with pytest.raises(NotImplementedError, match="MultiDeviceEngine.fedavg_routed.*no top-k path"):
        multi.fedavg_routed(tk, ns)
    for what in ("Scaffold engine", "client-sharded fedavg"):
        with pytest.raises(NotImplementedError, match=f"{what}: no top-k path"):
            reject_mxfp8(tk, what)
    monkeypatch.setattr(handoff, "_enabled", True)
    with pytest.raises(NotImplementedError, match="hand-off has no top-k route"):
        eng.fedavg_routed(tk, ns)
    monkeypatch.setattr(handoff, "_enabled", False)

    # the client's option
    cls = accelerate_algo(TorchFedAvgAlgo, wire="topk", error_feedback=True)
    assert cls._fedagg_topk is True and cls._fedagg_topk_density == 0.01 and cls._fedagg_mx_residual is None
    assert accelerate_algo(TorchFedAvgAlgo, wire="topk", error_feedback=True, density=1)._fedagg_topk_density == 1.0
    assert not hasattr(accelerate_algo(TorchFedAvgAlgo, wire="mxfp4"), "_fedagg_topk")
    with pytest.raises(ValueError, match="wire='topk' needs error_feedback=True.*discards most of every update"):
        accelerate_algo(TorchFedAvgAlgo, wire="topk")
    for bad in (0, -0.5, 1.5, "0.1", True):
        with pytest.raises(ValueError, match="density must be in \\(0, 1\\]"):
            accelerate_algo(TorchFedAvgAlgo, wire="topk", error_feedback=True, density=bad)
    for w in (False, True, "mxfp8", "mxfp4"):
        with pytest.raises(TypeError, match="density is an option of wire='topk'"):
            accelerate_algo(TorchFedAvgAlgo, wire=w, density=0.1)
    for base in (TorchScaffoldAlgo, TorchNewtonRaphsonAlgo):
        with pytest.raises(TypeError, match="wire='topk' is an option of TorchFedAvgAlgo"):
            accelerate_algo(base, wire="topk", error_feedback=True)
    with pytest.raises(ValueError, match="wire must be True, False or 'mxfp8'.*'topk'"):
        accelerate_algo(TorchFedAvgAlgo, wire="top-k")

    # the client's export: CPU tensors and no fp16 / fp64 path
    for dt in (torch.float32, torch.float16, torch.float64):
        with pytest.raises(NotImplementedError, match="wire='topk'"):
            wm.export_topk([torch.zeros(8, dtype=dt)], 0.5, torch.zeros(8))


def test_a_federation_without_the_option_never_maps_the_library():
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import numpy as np\n"
            "from standin_substrafl.algorithms.pytorch import TorchFedAvgAlgo\n"
            "from substrafl_amd import _native, wire, engine\n"
            "from substrafl_amd.integration import accelerate_algo\n"
            "from substrafl_amd.strategies import FedAvg\n"
            "from substrafl_amd.schemas import FedAvgSharedState\n"
            "_native.load()\n"
            "accelerate_algo(TorchFedAvgAlgo, wire='mxfp4', error_feedback=True)\n"
            "engine.AggregationEngine._fedavg_mxfp4 = lambda *a, **k: sys.exit(7)\n"
            "class A: strategies = ['Federated Averaging']\n"
            "u = list(wire.float32_to_mxfp4([np.ones((3, 2), np.float32)]))\n"
            "states = [FedAvgSharedState(n_samples=2, parameters_update=u) for _ in range(2)]\n"
            "mapped = lambda: 'substrafl_amd._native_topk' in sys.modules or 'libfedagg_topk' in open('/proc/self/maps').read()\n"
            "import atexit; atexit.register(lambda: mapped() and sys.stderr.write('LOADED'))\n"
            "FedAvg(algo=A(), device=0).avg_shared_states(shared_states=states, _skip=True)\n"
            % (str(ROOT), str(ROOT / "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 7 and "LOADED" not in r.stderr, r.stderr[-2000:]  # 7: the MXFP4 route was reached
