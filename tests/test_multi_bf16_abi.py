"""``fedagg_multi_fedavg_bf16`` without a GPU: the plain-C demo compiles against the header, the
binding matches it, and every bad argument is refused with ``FEDAGG_EINVAL`` before any HIP call --
the library is loaded, no device is opened, no engine exists (``m`` is NULL throughout; the entry
checks it last, so each case is refused for its own reason and the error text says which).  And
``weighted_average`` calls ``fedavg_routed`` where the engine has it, ``fedavg`` where it has not."""

import ctypes
import shutil
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from substrafl_amd import _native

ROOT = Path(__file__).resolve().parents[1]
NAME = "fedagg_multi_fedavg_bf16"
K, M = 3, 40


def test_the_demo_compiles_against_the_header(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    exe = tmp_path / "fedavg_multi_bf16_demo"
    libdir = _native.LIB_PATH.parent
    subprocess.run([gcc, "-O2", "-ffp-contract=off", "-Wall", "-Werror", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "c" / "fedavg_multi_bf16_demo.c"), f"-L{libdir}", "-lfedagg",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert exe.exists()


def test_the_binding_is_declared_and_bound():
    lib = _native.load()
    assert NAME in _native.SIGNATURES
    assert len(_native.SIGNATURES[NAME][1]) == 9
    assert hasattr(lib, NAME)
    header = (ROOT / "include" / "fedagg.h").read_text()
    assert "int fedagg_multi_fedavg_bf16(fedagg_multi* m, int K, int nseg, const void* const* h_seg" in header
    assert "const float* h_w, const uint64_t* h_idx, int P, float* h_out);" in header
    assert _native.ABI_VERSION == lib.fedagg_abi_version() == 17 and "#define FEDAGG_ABI_VERSION 17" in header


class Call:
    """A valid call over host arrays (two uneven segments per row), one argument replaced at a time."""

    def __init__(self):
        self.rows = np.zeros((K, M), np.uint16)
        cut = 7 * 2
        t = (ctypes.c_void_p * (2 * K))()
        for k in range(K):
            t[2 * k], t[2 * k + 1] = self.rows[k].ctypes.data, self.rows[k].ctypes.data + cut
        self.w = np.full(K, 1.0 / K, np.float32)
        self.out = np.zeros(M, np.float32)
        self.args = dict(m=None, K=K, nseg=2, h_seg=t, seg_bytes=u64(cut, M * 2 - cut), h_w=self.w.ctypes.data,
                         h_idx=u64(0, M - 1), P=2, h_out=self.out.ctypes.data)

    def __call__(self, **changed):
        lib = _native.load()
        a = dict(self.args, **changed)
        rc = getattr(lib, NAME)(*[a[k] for k in self.args])
        return rc, lib.fedagg_last_error().decode()


def u64(*v):
    return (ctypes.c_uint64 * len(v))(*v)


def test_bad_arguments_are_refused_before_any_hip_call():
    call = Call()
    # with everything else valid, the NULL engine is what is refused
    assert call() == (-1, NAME + ": NULL engine")
    assert call(nseg=0, h_seg=None, seg_bytes=None, h_idx=None, P=0) == (-1, NAME + ": NULL engine")  # M == 0
    for changed, text in [
        (dict(K=0), "K must be > 0"),
        (dict(K=-2), "K must be > 0"),
        (dict(K=0, h_w=None, h_out=None), "K must be > 0"),  # K comes first
        (dict(h_w=None), "invalid argument"),
        (dict(nseg=-1), "invalid argument"),
        (dict(h_seg=None), "invalid argument"),
        (dict(seg_bytes=None), "invalid argument"),
        (dict(P=-1), "invalid argument"),
        (dict(h_idx=None), "invalid argument"),
        (dict(h_w=None, seg_bytes=u64(13, 67)), "invalid argument"),  # before the segment sizes
        (dict(seg_bytes=u64(13, 67)), "segment not a whole number of elements"),
        (dict(seg_bytes=u64(14, 65)), "segment not a whole number of elements"),
        (dict(seg_bytes=u64(13, 67), h_idx=u64(0, M)), "segment not a whole number of elements"),  # before the indices
        (dict(h_idx=u64(0, M)), "numel == 1 index out of range"),
        (dict(h_idx=u64(2**63, 1)), "numel == 1 index out of range"),
        (dict(h_idx=u64(0, M), h_out=None), "numel == 1 index out of range"),  # before h_out
        (dict(nseg=0, h_seg=None, seg_bytes=None, h_idx=u64(0), P=1), "numel == 1 index out of range"),  # M == 0
        (dict(h_out=None), "NULL h_out"),
    ]:
        rc, err = call(**changed)
        assert rc == -1 and err == f"{NAME}: {text}", (changed, rc, err)
    # NULL h_idx is fine with P == 0
    assert call(h_idx=None, P=0)[1].endswith("NULL engine")
    assert not call.out.any(), "a refused call wrote its output"


# ------------------------------------------------------------------------------------- the strategies' switch
class OnlyFedAvg:
    def __init__(self):
        self.calls = []

    def fedavg(self, updates, n_samples, wire=False):
        self.calls.append(("fedavg", len(updates), list(n_samples), wire))
        return ["fedavg"]


class Routed(OnlyFedAvg):
    def fedavg_routed(self, updates, n_samples, wire=False):
        self.calls.append(("fedavg_routed", len(updates), list(n_samples), wire))
        return ["fedavg_routed"]


@pytest.mark.parametrize("fake,name", [(OnlyFedAvg, "fedavg"), (Routed, "fedavg_routed")])
def test_weighted_average_calls_the_routed_name_where_the_engine_has_it(monkeypatch, fake, name):
    from substrafl_amd.strategies import fed_avg

    engine, asked = fake(), []
    monkeypatch.setattr(fed_avg, "engine_for", lambda device: asked.append(device) or engine)
    states = [SimpleNamespace(parameters_update=[np.ones((2, 3), np.float32), np.ones(1, np.float32)], n_samples=n)
              for n in (3, 5)]
    assert fed_avg.weighted_average(states, "FedAvgSharedState", device=(0, 0), wire=False) == [name]
    assert engine.calls == [(name, 2, [3, 5], False)] and asked == [(0, 0)]
