"""``fedagg_dense_gelqf_f64`` / ``fedagg_dense_orglq_f64`` and the FedPCA option built on them, without
a GPU: the header, the binding and the export agree; bad arguments come back as -1 with their own
text before any HIP call; the C demo compiles against the headers alone; the GPU tests' shapes stay
small and their exact family is what LAPACK gives; the ``qr`` option is validated; the engine declines
before it touches a device; and the default classes never map the dense library."""

import ctypes
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from substrafl_amd import _native, _native_dense
from test_dense_abi import declared_functions
from test_dense_lq_gpu import MAX_ELEMENTS, PAD, _exact_case, _shapes

ROOT = Path(__file__).resolve().parents[1]
LQ_SYMBOLS = ("fedagg_dense_lq_blocking", "fedagg_dense_lq_ws_bytes", "fedagg_dense_gelqf_f64", "fedagg_dense_orglq_f64")


def test_header_binding_and_export_agree():
    lib = ctypes.CDLL(str(_native_dense.LIB_PATH))
    for name in LQ_SYMBOLS:
        assert name in declared_functions() and hasattr(lib, name) and name in _native_dense.SIGNATURES, name
    assert len(_native_dense.SIGNATURES["fedagg_dense_gelqf_f64"][1]) == 7  # d_A, n, m, lda, d_tau, d_ws, stream
    assert len(_native_dense.SIGNATURES["fedagg_dense_orglq_f64"][1]) == 9  # ..., d_Q, ldq, d_ws, stream
    assert _native_dense.SIGNATURES["fedagg_dense_lq_ws_bytes"][0] is ctypes.c_uint64
    assert _native_dense.load().fedagg_dense_abi_version() == 1  # added within ABI version 1


def test_blocking_workspace_and_shapes():
    lib = _native_dense.load()
    panel, tm, tn, kc = _native_dense.lq_blocking()
    assert panel > 0 and tm > 0 and tn > 0 and kc > 0 and (panel, tm, tn) == _native_dense.blocking()
    assert lib.fedagg_dense_lq_blocking(None, None, None, None) == -1
    assert b"NULL output" in lib.fedagg_dense_last_error()
    assert lib.fedagg_dense_lq_ws_bytes(0, 0) == 0 and lib.fedagg_dense_lq_ws_bytes(0, 9) == 0
    assert lib.fedagg_dense_lq_ws_bytes(1, 1) > 0
    assert lib.fedagg_dense_lq_ws_bytes(512, 16384) < 512 * 16384 * 8  # less than a second matrix
    shapes = _shapes()
    B = max(panel, tm, tn)
    assert max(n * (m + PAD + 2) for n, m in shapes) < MAX_ELEMENTS  # the largest GPU case, padded
    assert (2 * B + 33, 3 * kc + 7) in shapes and (1, 1) in shapes and all(n <= m for n, m in shapes)


def test_bad_arguments_are_refused_before_any_hip_call():
    lib = _native_dense.load()
    A, T, Q, W = 0x1000, 0x2000, 0x3000, 0x4000  # never dereferenced: every check comes before the first HIP call
    err = lib.fedagg_dense_last_error
    gelqf, orglq = lib.fedagg_dense_gelqf_f64, lib.fedagg_dense_orglq_f64
    big = (1 << 20) + 1
    # n == 0: OK, nothing touched, whatever the pointers
    assert gelqf(None, 0, 5, 5, None, None, None) == 0
    assert orglq(None, 0, 5, 5, None, None, 5, None, None) == 0
    assert gelqf(None, 3, 5, 5, T, W, None) == -1 and b"d_A is NULL" in err()
    assert gelqf(A, 3, 5, 5, None, W, None) == -1 and b"d_tau is NULL" in err()
    assert gelqf(A, 3, 5, 5, T, None, None) == -1 and b"d_ws is NULL" in err()
    assert gelqf(A, 3, 5, 4, T, W, None) == -1 and b"lda = 4 is smaller than m" in err()
    assert gelqf(A, 6, 5, 5, T, W, None) == -1 and b"larger than m" in err()
    assert gelqf(A, big, big, big, T, W, None) == -1 and b"n = 1048577 exceeds FEDAGG_DENSE_MAX_N" in err()
    assert gelqf(A, 3, big, big, T, W, None) == -1 and b"m = 1048577 exceeds FEDAGG_DENSE_MAX_N" in err()
    assert gelqf(A, 2, 5, 1 << 62, T, W, None) == -1 and b"overflows" in err()
    assert orglq(None, 3, 5, 5, T, Q, 5, W, None) == -1 and b"d_A is NULL" in err()
    assert orglq(A, 3, 5, 5, None, Q, 5, W, None) == -1 and b"d_tau is NULL" in err()
    assert orglq(A, 3, 5, 5, T, None, 5, W, None) == -1 and b"d_Q is NULL" in err()
    assert orglq(A, 3, 5, 5, T, Q, 5, None, None) == -1 and b"d_ws is NULL" in err()
    assert orglq(A, 3, 5, 4, T, Q, 5, W, None) == -1 and b"lda = 4 is smaller than m" in err()
    assert orglq(A, 3, 5, 5, T, Q, 4, W, None) == -1 and b"ldq = 4 is smaller than m" in err()
    assert orglq(A, 6, 5, 5, T, Q, 5, W, None) == -1 and b"larger than m" in err()
    assert orglq(A, 3, big, big, T, Q, big, W, None) == -1 and b"FEDAGG_DENSE_MAX_N" in err()
    assert orglq(A, 2, 5, 1 << 62, T, Q, 5, W, None) == -1 and b"n * lda * 8 overflows" in err()
    assert orglq(A, 2, 5, 5, T, Q, 1 << 62, W, None) == -1 and b"n * ldq * 8 overflows" in err()
    with pytest.raises(_native.NativeLibraryError, match="ldq"):
        _native_dense.check(-1, "x")


def test_c_demo_compiles_against_the_headers(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    exe = tmp_path / "dense_lq_demo"
    libdir = _native_dense.LIB_PATH.parent
    subprocess.run([gcc, "-O2", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "c" / "dense_lq_demo.c"),
                    f"-L{libdir}", "-lfedagg_dense", "-lfedagg", "-lm", f"-Wl,-rpath,{libdir}",
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert exe.exists()


def test_exact_family_on_the_host():
    """The family's claims at the GPU tests' own shapes (from the library's ``lq_blocking()``) and
    seeds, without a GPU: tau in {0, 1}, every factor entry a signed power of two (or zero), and
    LAPACK's L Q reproduces A exactly with exactly orthonormal rows."""
    shapes = _shapes()
    for shape, seed in [(s, seed) for s in shapes for seed in (0, 1)] + [((97, 577), 2), ((97, 577), 3)]:
        A, L, tau, Q = _exact_case(*shape, seed)
        assert set(np.unique(tau)) <= {0.0, 1.0}
        for F in (L, Q):
            nz = np.abs(F[F != 0])
            assert np.array_equal(nz, 2.0 ** np.round(np.log2(nz))) and nz.max() <= 4.0 and nz.min() >= 0.5
        assert np.array_equal(L @ Q, A) and np.array_equal(Q @ Q.T, np.eye(shape[0]))
        assert np.array_equal(np.count_nonzero(A, axis=1), np.ones(shape[0])) and np.count_nonzero(A, axis=0).max() <= 1


# ------------------------------------------------------------------ the option
def test_qr_option_is_validated(dummy_algo_class, monkeypatch):
    import standin_substrafl.strategies as ss

    from substrafl_amd.integration import accelerate
    from substrafl_amd.strategies import FedPCA
    from substrafl_amd.strategies.fed_pca import orthonormal_layers, qr_mode

    monkeypatch.delenv("FEDAGG_PCA_QR", raising=False)
    with pytest.raises(ValueError, match="qr"):
        accelerate(ss.FedPCA, qr="gpu")
    with pytest.raises(ValueError, match="qr"):
        FedPCA(algo=dummy_algo_class(), qr="gpu")
    assert accelerate(ss.FedPCA)._fedagg_qr == "host" and accelerate(ss.FedPCA, qr="device")._fedagg_qr == "device"
    assert accelerate(ss.FedAvg, qr="device") and accelerate(ss.NewtonRaphson, qr="device")  # accepted, without effect
    assert not hasattr(accelerate(ss.FedAvg, qr="device"), "_fedagg_qr")
    assert accelerate(ss.FedPCA, solve="device", qr="device")._fedagg_qr == "device"  # solve: still without effect
    plain, opted = FedPCA(algo=dummy_algo_class()), FedPCA(algo=dummy_algo_class(), qr="device")
    assert plain._qr == "host" and "qr" not in plain.kwargs  # the default's recorded arguments are as before
    assert opted._qr == "device" and opted.kwargs["qr"] == "device"  # ... the option travels to the task process
    assert qr_mode("host") == "host" and qr_mode("device") == "device"
    monkeypatch.setenv("FEDAGG_PCA_QR", "device")
    assert qr_mode("host") == "device"
    monkeypatch.setenv("FEDAGG_PCA_QR", "host")
    assert qr_mode("device") == "host"
    monkeypatch.setenv("FEDAGG_PCA_QR", "gpu")
    with pytest.raises(ValueError, match="qr"):
        orthonormal_layers([np.eye(2)], None, "host")


class _Engine:
    """An engine stand-in: ``orthonormal_rows`` answers what ``answer(a)`` says and keeps the calls."""

    def __init__(self, answer):
        self.answer, self.calls, self.last_timing = answer, [], {}

    def orthonormal_rows(self, a):
        self.calls.append(a.shape)
        return self.answer(a)


def test_routes_on_an_engine_stand_in(monkeypatch):
    from substrafl_amd.strategies import fed_pca

    rng = np.random.default_rng(0)
    layers = [rng.standard_normal((3, 8)), rng.standard_normal((8, 3)).astype(np.float32)]
    want = [np.linalg.qr(a.T)[0].T for a in layers]
    marker = np.full((3, 8), 7.0)
    eng = _Engine(lambda a: (marker, "device") if a.shape == (3, 8) else (None, "host: test decline"))
    monkeypatch.setattr(fed_pca, "engine_for", lambda device: eng)
    monkeypatch.delenv("FEDAGG_PCA_QR", raising=False)
    got = fed_pca.orthonormal_layers(layers, None, "host")
    assert eng.calls == [] and all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))
    got = fed_pca.orthonormal_layers(layers, None, "device")
    assert eng.calls == [(3, 8), (8, 3)] and got[0] is marker
    assert got[1].dtype == np.float32 and np.array_equal(got[1], want[1])  # the declined layer: today's line
    assert eng.last_timing == {"qr": "host: test decline", "qr_layers": ["device", "host: test decline"]}
    monkeypatch.setenv("FEDAGG_PCA_QR", "host")
    assert fed_pca.orthonormal_layers(layers, None, "device")[0] is not marker and len(eng.calls) == 2


def test_engine_declines_before_touching_the_device(monkeypatch):
    """Not an ndarray, not 2-D, another dtype, byte-swapped, empty or tall: the real engine's method
    says why and returns before it asks for the library or a session."""
    from substrafl_amd.engine import AggregationEngine

    def untouched(*a, **k):
        raise AssertionError("the engine was touched")

    monkeypatch.setattr(_native_dense, "load", untouched)
    monkeypatch.setattr(AggregationEngine, "session", untouched)
    eng = AggregationEngine.__new__(AggregationEngine)  # no device behind it
    a = np.random.default_rng(1).standard_normal((3, 8))
    cases = {"ndarray": a.tolist(), "2-D": a[0], "dtype int64": a.astype(np.int64), "dtype float16": a.astype(np.float16),
             "byte order": a.astype(a.dtype.newbyteorder()), "empty": a[:0], "n > m": np.ascontiguousarray(a.T),
             "3, 8, 1": a[:, :, None]}
    rows = getattr(AggregationEngine.orthonormal_rows, "__wrapped__", AggregationEngine.orthonormal_rows)
    for word, x in cases.items():
        q, reason = rows(eng, x)
        assert q is None and reason.startswith("host: ") and word in reason, (word, reason)


def test_default_classes_never_map_the_dense_library():
    """A fresh interpreter: ``accelerate(ss.FedPCA)`` and ``strategies.FedPCA`` with the default
    ``qr`` aggregate through an engine stand-in (NumPy's weighted average), give today's line's bits,
    and the process never imports the dense binding or maps libfedagg_dense.so."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import numpy as np\n"
            "import standin_substrafl.strategies as ss\n"
            "from standin_substrafl.strategies import schemas as sch\n"
            "from conftest import DummyAlgo\n"
            "import substrafl_amd.integration as I, substrafl_amd.strategies.fed_avg as FA\n"
            "from substrafl_amd.schemas import FedPCASharedState\n"
            "from substrafl_amd.strategies import FedPCA\n"
            "class E:\n"
            "    calls = 0\n"
            "    def fedavg(self, updates, n_samples, wire=False):\n"
            "        E.calls += 1\n"
            "        n = sum(n_samples)\n"
            "        return [np.sum([u[i] * (k / n) for u, k in zip(updates, n_samples)], axis=0) for i in range(len(updates[0]))]\n"
            "FA.engine_for = lambda device: E()\n"
            "rng = np.random.default_rng(6)\n"
            "layers = [[rng.standard_normal(s).astype(dt) for s, dt in (((4, 30), 'f4'), ((9, 9), 'f8'))] for _ in range(3)]\n"
            "class A: pass\n"
            "for s, cls in ((FedPCA(algo=DummyAlgo()), FedPCASharedState), (I.accelerate(ss.FedPCA)(algo=A()), sch.FedPCASharedState)):\n"
            "    st = [cls(n_samples=n, parameters_update=list(p)) for n, p in zip((3, 9, 4), layers)]\n"
            "    avg = s.avg_shared_states(shared_states=st, _skip=True).avg_parameters_update\n"
            "    got = s.avg_shared_states_with_qr(shared_states=st, _skip=True).avg_parameters_update\n"
            "    for a, g in zip(avg, got):\n"
            "        w = np.linalg.qr(np.asarray(a).T)[0].T\n"
            "        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()\n"
            "assert E.calls == 4\n"
            "assert 'substrafl_amd._native_dense' not in sys.modules\n"
            "assert 'libfedagg_dense' not in open('/proc/self/maps').read()\n" % (str(ROOT), str(ROOT / "tests")))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300)
