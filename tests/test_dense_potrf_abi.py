"""``fedagg_dense_potrf_f64`` and the Hessian check built on it, without a GPU: the header, the
binding and the export agree; bad arguments come back as -1 with their own text before any HIP
call; the C demo compiles against the headers alone; the exact family of the GPU tests is what
LAPACK's Cholesky gives, bit for bit; the decision rule of
``integration.newton_raphson_hessian_check`` on a stubbed engine; and the default client class
never maps the dense library."""

import ctypes
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from substrafl_amd import _native, _native_dense
from substrafl_amd import integration
from substrafl_amd.exceptions import NegativeHessianMatrixError
from test_dense_abi import declared_functions
from test_dense_potrf_gpu import _exact_factor, _gram

ROOT = Path(__file__).resolve().parents[1]
EXACT_SIZES = [1, 2, 3, 17, 31, 32, 33, 63, 64, 65, 129, 327, 577]


def test_header_binding_and_export_agree():
    assert "fedagg_dense_potrf_f64" in declared_functions()
    lib = ctypes.CDLL(str(_native_dense.LIB_PATH))
    assert hasattr(lib, "fedagg_dense_potrf_f64")
    res, args = _native_dense.SIGNATURES["fedagg_dense_potrf_f64"]
    assert res is ctypes.c_int and len(args) == 5  # d_A, n, lda, d_info, stream
    assert _native_dense.load().fedagg_dense_abi_version() == 1  # added within ABI version 1


def test_bad_arguments_are_refused_before_any_hip_call():
    lib = _native_dense.load()
    A, I = 0x1000, 0x3000  # never dereferenced: every check comes before the first HIP call
    err = lib.fedagg_dense_last_error
    assert lib.fedagg_dense_potrf_f64(None, 0, 0, None, None) == 0  # n == 0: OK, nothing touched
    assert lib.fedagg_dense_potrf_f64(None, 4, 4, I, None) == -1 and b"d_A is NULL" in err()
    assert lib.fedagg_dense_potrf_f64(A, 4, 4, None, None) == -1 and b"d_info is NULL" in err()
    assert lib.fedagg_dense_potrf_f64(A, 4, 3, I, None) == -1 and b"smaller than n" in err()
    assert lib.fedagg_dense_potrf_f64(A, (1 << 20) + 1, 1 << 21, I, None) == -1 and b"FEDAGG_DENSE_MAX_N" in err()
    assert lib.fedagg_dense_potrf_f64(A, 2, 1 << 62, I, None) == -1 and b"overflows" in err()
    # the LU entry points report through the same per-thread message
    assert lib.fedagg_dense_getrf_f64(A, 4, 4, None, I, None, None) == -1 and b"d_ipiv is NULL" in err()
    with pytest.raises(_native.NativeLibraryError, match="d_ipiv is NULL"):
        _native_dense.check(-1, "x")


def test_c_demo_compiles_against_the_headers(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    exe = tmp_path / "dense_potrf_demo"
    libdir = _native_dense.LIB_PATH.parent
    subprocess.run([gcc, "-O2", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "c" / "dense_potrf_demo.c"),
                    f"-L{libdir}", "-lfedagg_dense", "-lfedagg", f"-Wl,-rpath,{libdir}",
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(exe)], check=True)
    assert exe.exists()


@pytest.mark.parametrize("n", EXACT_SIZES)
def test_exact_family_on_the_host(n):
    """The family's claim, without a GPU: LAPACK's Cholesky of A = L L^T is L, bit for bit."""
    A, L = _exact_factor(n)
    assert np.all(A == np.round(A)) and np.abs(A).max() < 2.0 ** 40
    assert np.array_equal(np.linalg.cholesky(A), L)
    for p in sorted({0, 31, 32, 33, n - 1}):  # the failed-pivot variant: not positive definite
        if p < n:
            B = A.copy()
            B[p, p] -= L[p, p] ** 2
            with pytest.raises(np.linalg.LinAlgError):
                np.linalg.cholesky(B)


# ------------------------------------------------------------------ the decision rule
class _Engine:
    """An engine stand-in: ``hessian_cholesky_check`` answers ``answer`` and counts its calls."""

    def __init__(self, answer):
        self.answer, self.calls, self.last_timing = answer, 0, {}

    def hessian_cholesky_check(self, H):
        self.calls += 1
        return self.answer


@pytest.fixture
def eig_calls(monkeypatch):
    calls = []
    real = np.linalg.eig

    def counting(a):
        calls.append(a.shape)
        return real(a)

    monkeypatch.setattr(np.linalg, "eig", counting)
    return calls


def _use(monkeypatch, engine):
    monkeypatch.setattr(integration, "engine_for", lambda device: engine)
    monkeypatch.delenv("FEDAGG_NR_CHECK", raising=False)


def _reference_rule(H):
    """torch_newton_raphson_algo.py:346-347: whether the reference raises."""
    return not (np.linalg.eig(H)[0].real >= 0).all()


H_PD = _gram(9, 36, 0.0)
H_INDEFINITE = H_PD - 0.5 * np.linalg.eigvalsh(H_PD).max() * np.eye(9)


def test_device_ok_accepts_without_eigenvalues(monkeypatch, eig_calls):
    eng = _Engine((True, 0, "device"))
    _use(monkeypatch, eng)
    assert integration.newton_raphson_hessian_check(H_INDEFINITE, 0.0) == "device"  # the engine's word is taken
    assert eng.calls == 1 and eig_calls == []
    assert integration.last_hessian_check["route"] == "device" and eng.last_timing["check"] == "device"


@pytest.mark.parametrize("answer,route", [((False, 4, "device"), "host after device info=4"),
                                          ((None, 0, "host: test decline"), "host: test decline")])
def test_failure_or_decline_hands_over_to_the_reference_rule(monkeypatch, eig_calls, answer, route):
    eng = _Engine(answer)
    _use(monkeypatch, eng)
    assert not _reference_rule(H_PD) and _reference_rule(H_INDEFINITE)
    del eig_calls[:]
    assert integration.newton_raphson_hessian_check(H_PD, 0.25) == route  # the host rule accepts
    assert eig_calls == [(9, 9)] and integration.last_hessian_check["route"] == route
    with pytest.raises(NegativeHessianMatrixError) as e:
        integration.newton_raphson_hessian_check(H_INDEFINITE, 0.25)
    eigenvalues = np.linalg.eig(H_INDEFINITE)[0].real
    msg = str(e.value)
    assert msg.startswith("Hessian matrix is not positive semi-definite")
    assert f"Calculated eigenvalues are {eigenvalues.tolist()} and considered l2_coeff is 0.25" in msg
    assert integration.last_hessian_check["route"] == route and eng.calls == 2

    class Mine(Exception):
        pass

    with pytest.raises(Mine, match="Calculated eigenvalues are"):
        integration.newton_raphson_hessian_check(H_INDEFINITE, 0.25, error_cls=Mine)


def test_host_mode_and_environment_override(monkeypatch, eig_calls):
    eng = _Engine((True, 0, "device"))
    _use(monkeypatch, eng)
    assert integration.newton_raphson_hessian_check(H_PD, 0.0, check="host") == "host"
    assert eng.calls == 0 and len(eig_calls) == 1
    with pytest.raises(NegativeHessianMatrixError):
        integration.newton_raphson_hessian_check(H_INDEFINITE, 0.0, check="host")
    monkeypatch.setenv("FEDAGG_NR_CHECK", "device")
    assert integration.newton_raphson_hessian_check(H_PD, 0.0, check="host") == "device" and eng.calls == 1
    monkeypatch.setenv("FEDAGG_NR_CHECK", "host")
    assert integration.newton_raphson_hessian_check(H_PD, 0.0, check="device") == "host" and eng.calls == 1
    monkeypatch.setenv("FEDAGG_NR_CHECK", "gpu")
    with pytest.raises(ValueError, match="check"):
        integration.newton_raphson_hessian_check(H_PD, 0.0)
    monkeypatch.delenv("FEDAGG_NR_CHECK")
    with pytest.raises(ValueError, match="check"):
        integration.newton_raphson_hessian_check(H_PD, 0.0, check="gpu")


def test_engine_declines_before_touching_the_device(monkeypatch, eig_calls):
    """A non-symmetric, fp32, 1-D, non-square, empty or byte-swapped Hessian: the real engine's
    method says why and returns before it asks for the library or a session."""
    from substrafl_amd.engine import AggregationEngine

    def untouched(*a, **k):
        raise AssertionError("the engine was touched")

    monkeypatch.setattr(_native_dense, "load", untouched)
    monkeypatch.setattr(AggregationEngine, "session", untouched)
    eng = AggregationEngine.__new__(AggregationEngine)  # no device behind it
    monkeypatch.setattr(eng, "lock_devices", lambda: [], raising=False)
    skew = H_PD.copy()
    skew[3, 1] = np.nextafter(skew[3, 1], 1.0)
    cases = {"transpose": skew, "float32": H_PD.astype(np.float32), "shape": H_PD[0], "square": H_PD[:, :4],
             "empty": np.zeros((0, 0)), "native": H_PD.astype(H_PD.dtype.newbyteorder())}
    check = getattr(AggregationEngine.hessian_cholesky_check, "__wrapped__", AggregationEngine.hessian_cholesky_check)
    for word, H in cases.items():
        ok, info, reason = check(eng, H)
        assert ok is None and info == 0 and reason.startswith("host: ") and word in reason, (word, reason)
    # and the public rule then decides on the host, with the reason as its route
    _use(monkeypatch, type("E", (), {"hessian_cholesky_check": lambda self, H: check(eng, H), "last_timing": {}})())
    route = integration.newton_raphson_hessian_check(skew, 0.0)
    assert route.startswith("host: ") and "transpose" in route and len(eig_calls) == 1


def test_tiled_symmetry_test_is_array_equal_with_the_transpose():
    from substrafl_amd.engine import equals_transpose

    for n in (1, 2, 63, 64, 65, 130, 327):
        H = _gram(n, 2 * n, 0.0)
        assert equals_transpose(H) and np.array_equal(H, H.T)
        for i, k in {(n - 1, 0), (n // 2, n // 3), (n - 1, n - 1), (0, 0)}:
            for value in ([np.nextafter(H[i, k], 9.0)] if i != k else []) + [np.nan]:
                B = H.copy()
                B[i, k] = value  # one entry below (or on) the diagonal; a NaN differs from itself
                assert equals_transpose(B) == np.array_equal(B, B.T) == False, (n, i, k, value)  # noqa: E712
                assert equals_transpose(np.ascontiguousarray(B.T)) is False


# ------------------------------------------------------------------ the client class
def test_accelerate_algo_takes_the_newton_raphson_client_and_validates_the_option():
    from standin_substrafl.algorithms.pytorch import TorchFedAvgAlgo, TorchScaffoldAlgo
    from standin_substrafl.algorithms.pytorch import torch_newton_raphson_algo as nr

    from substrafl_amd.integration import accelerate_algo

    cls = accelerate_algo(nr.TorchNewtonRaphsonAlgo)
    assert issubclass(cls, nr.TorchNewtonRaphsonAlgo) and cls._fedagg_hessian_check == "host"
    assert cls._local_train is nr.TorchNewtonRaphsonAlgo._local_train and cls.train is not nr.TorchNewtonRaphsonAlgo.train

    class Mine(nr.TorchNewtonRaphsonAlgo):
        pass

    assert accelerate_algo(Mine, hessian_check="device")._fedagg_hessian_check == "device"
    with pytest.raises(ValueError, match="hessian_check"):
        accelerate_algo(nr.TorchNewtonRaphsonAlgo, hessian_check="gpu")
    for other in (TorchFedAvgAlgo, TorchScaffoldAlgo):
        with pytest.raises(TypeError, match="hessian_check"):
            accelerate_algo(other, hessian_check="host")
        assert accelerate_algo(other)  # as before


def test_default_client_class_never_maps_the_dense_library():
    """A fresh interpreter: an accelerated NewtonRaphson client with the default ``hessian_check``
    trains one round on the CPU and the process never loads libfedagg_dense.so."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import numpy as np, torch\n"
            "from standin_substrafl.algorithms.pytorch import torch_newton_raphson_algo as nr\n"
            "from substrafl_amd.integration import accelerate_algo\n"
            "import substrafl_amd.integration as I\n"
            "class DS(torch.utils.data.Dataset):\n"
            "    def __init__(self, d, is_inference=False): self.x, self.y = d\n"
            "    def __len__(self): return len(self.x)\n"
            "    def __getitem__(self, i): return self.x[i], self.y[i]\n"
            "g = torch.Generator().manual_seed(0)\n"
            "d = (torch.randn(12, 3, generator=g), (torch.rand(12, 1, generator=g) > 0.5).float())\n"
            "def make(cls):\n"
            "    torch.manual_seed(1)\n"
            "    m = torch.nn.Sequential(torch.nn.Linear(3, 1), torch.nn.Sigmoid())\n"
            "    return cls(m, torch.nn.BCELoss(), 5, DS, l2_coeff=0.1, disable_gpu=True)\n"
            "cls = accelerate_algo(nr.TorchNewtonRaphsonAlgo)\n"
            "a, b = make(cls), make(nr.TorchNewtonRaphsonAlgo)\n"
            "sa, sb = a.train(shared_state=None, data_from_opener=d, _skip=True), "
            "b.train(shared_state=None, data_from_opener=d, _skip=True)\n"
            "assert a._fedagg_hessian_route == 'host' and I.last_hessian_check['route'] == 'host'\n"
            "assert sa.n_samples == sb.n_samples == 12 and sa.hessian.shape == (4, 4)\n"
            "assert sa.hessian.tobytes() == sb.hessian.tobytes()\n"
            "assert all(x.tobytes() == y.tobytes() for x, y in zip(sa.gradients, sb.gradients))\n"
            "assert 'substrafl_amd._native_dense' not in sys.modules\n"
            "assert 'libfedagg_dense' not in open('/proc/self/maps').read()\n" % (str(ROOT), str(ROOT / "tests")))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300)
