"""``fedagg_dense_symcopy_f64`` / ``fedagg_dense_potrs_f64`` and the ``solve="cholesky"`` option built
on them, without a GPU: the header, the binding and the export agree; bad arguments come back as -1
with their own text before any HIP call; the exact family of the GPU tests is exact on the host in
either summation order; the option is validated and routed (on an engine stand-in); and the default
class never maps the dense library."""

import ctypes
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from substrafl_amd import _native, _native_dense
from substrafl_amd import integration
from test_dense_abi import declared_functions
from test_dense_posv_gpu import _exact_rhs

ROOT = Path(__file__).resolve().parents[1]
POSV_SYMBOLS = ("fedagg_dense_symcopy_f64", "fedagg_dense_potrs_f64")


def test_header_binding_and_export_agree():
    lib = ctypes.CDLL(str(_native_dense.LIB_PATH))
    for name in POSV_SYMBOLS:
        assert name in declared_functions() and hasattr(lib, name) and name in _native_dense.SIGNATURES, name
    assert len(_native_dense.SIGNATURES["fedagg_dense_symcopy_f64"][1]) == 7  # d_A, n, lda, d_L, ldl, d_flag, stream
    assert len(_native_dense.SIGNATURES["fedagg_dense_potrs_f64"][1]) == 5  # d_L, n, ldl, d_b, stream
    assert _native_dense.load().fedagg_dense_abi_version() == _native_dense.ABI_VERSION == 1  # added within version 1


def test_bad_arguments_are_refused_before_any_hip_call():
    lib = _native_dense.load()
    A, L, B, F = 0x1000, 0x3000, 0x5000, 0x7000  # never dereferenced: every check comes before the first HIP call
    err = lib.fedagg_dense_last_error
    symcopy, potrs = lib.fedagg_dense_symcopy_f64, lib.fedagg_dense_potrs_f64
    big = (1 << 20) + 1
    # n == 0: OK, nothing touched, whatever the pointers
    assert symcopy(None, 0, 0, None, 0, None, None) == 0
    assert potrs(None, 0, 0, None, None) == 0
    assert symcopy(None, 4, 4, L, 4, F, None) == -1 and b"d_A is NULL" in err()
    assert symcopy(A, 4, 4, L, 4, None, None) == -1 and b"d_flag is NULL" in err()
    assert symcopy(A, 4, 4, None, 4, None, None) == -1 and b"d_flag is NULL" in err()
    assert symcopy(A, 4, 3, L, 4, F, None) == -1 and b"lda = 3 is smaller than n" in err()
    assert symcopy(A, 4, 4, L, 3, F, None) == -1 and b"ldl = 3 is smaller than n" in err()
    assert symcopy(A, big, big, L, big, F, None) == -1 and b"n = 1048577 exceeds FEDAGG_DENSE_MAX_N" in err()
    assert symcopy(A, 2, 1 << 62, L, 2, F, None) == -1 and b"n * lda * 8 overflows" in err()
    assert symcopy(A, 2, 2, L, 1 << 62, F, None) == -1 and b"n * ldl * 8 overflows" in err()
    # d_L inside the rows of d_A, d_A inside those of d_L, and the first byte behind either
    assert symcopy(A, 4, 4, A, 4, F, None) == -1 and b"d_L overlaps d_A" in err()
    assert symcopy(A, 4, 4, A + 8 * 15, 4, F, None) == -1 and b"d_L overlaps d_A" in err()
    assert symcopy(A + 8 * 15, 4, 4, A, 4, F, None) == -1 and b"d_L overlaps d_A" in err()
    assert potrs(None, 4, 4, B, None) == -1 and b"d_L is NULL" in err()
    assert potrs(L, 4, 4, None, None) == -1 and b"d_b is NULL" in err()
    assert potrs(L, 4, 3, B, None) == -1 and b"ldl = 3 is smaller than n" in err()
    assert potrs(L, big, big, B, None) == -1 and b"n = 1048577 exceeds FEDAGG_DENSE_MAX_N" in err()
    assert potrs(L, 3, (1 << 64) - 1, B, None) == -1 and b"overflows" in err()
    with pytest.raises(_native.NativeLibraryError, match="overflows"):
        _native_dense.check(-1, "x")


def _substitute(L, b, reverse):
    """L L^T x = b by substitution with divisions, the sums ascending or (``reverse``) descending."""
    n = L.shape[0]
    order = (lambda ks: list(ks)[::-1]) if reverse else list
    y = b.copy()
    for i in range(n):
        for k in order(range(i)):
            y[i] -= L[i, k] * y[k]
        y[i] /= L[i, i]
    for i in range(n - 1, -1, -1):
        for k in order(range(i + 1, n)):
            y[i] -= L[k, i] * y[k]
        y[i] /= L[i, i]
    return y


@pytest.mark.parametrize("n", [1, 2, 33, 65, 129])
def test_exact_family_on_the_host(n):
    """The family's claim, without a GPU: b and every partial sum of either substitution are small
    integers, so the substitution returns x by value in either summation order."""
    L, x, b = _exact_rhs(n)
    y = L.T @ x
    assert np.all(b == np.round(b)) and np.abs(y).max() * 4 * n < 2.0 ** 40 and np.abs(x).max() <= 2
    for reverse in (False, True):
        assert np.array_equal(_substitute(L, b, reverse), x), (n, reverse)


# ------------------------------------------------------------------ the option
class _Engine:
    """An engine stand-in: NumPy's sums, and a ``newton_raphson_solve`` that answers ``answer`` and
    keeps the ``method`` it was called with."""

    def __init__(self, answer):
        self.answer, self.methods, self.last_timing = answer, [], {}

    def sequential_sum(self, rows, n_samples):
        n = sum(n_samples)
        return [sum(r[0] * (k / n) for r, k in zip(rows, n_samples))]

    def newton_raphson_solve(self, hessians, gradients, n_samples, method="lu"):
        self.methods.append(method)
        return self.answer


class _Algo:
    pass


def _states():
    from standin_substrafl.strategies import schemas as sch

    H = np.array([[4.0, 1.0], [1.0, 3.0]])
    g = [np.array([1.0, 2.0])]
    return [sch.NewtonRaphsonSharedState(gradients=g, hessian=H, n_samples=2) for _ in range(2)], H, g[0]


def test_solve_option_is_validated_and_routed(monkeypatch):
    import standin_substrafl.strategies as ss

    from substrafl_amd.integration import accelerate, newton_raphson_update

    monkeypatch.delenv("FEDAGG_NR_SOLVE", raising=False)
    with pytest.raises(ValueError, match="'host', 'device' or 'cholesky'"):
        accelerate(ss.NewtonRaphson, solve="gpu")
    assert accelerate(ss.NewtonRaphson, solve="cholesky")._fedagg_solve == "cholesky"
    assert accelerate(ss.NewtonRaphson, solve="device")._fedagg_solve == "device"
    assert accelerate(ss.NewtonRaphson)._fedagg_solve == "host"
    for other in (ss.FedAvg, ss.Scaffold, ss.FedPCA):  # accepted and without effect for the other strategies
        assert not hasattr(accelerate(other, solve="cholesky"), "_fedagg_solve")

    st, H, g = _states()
    x = np.array([7.0, -3.0])
    eng = _Engine((x, 0, "device: cholesky"))
    monkeypatch.setattr(integration, "engine_for", lambda device: eng)
    host = -0.5 * np.linalg.solve(H * 0.5 + H * 0.5, g * 0.5 + g * 0.5)
    assert np.array_equal(newton_raphson_update(st, 0.5, solve="cholesky"), -0.5 * x) and eng.methods == ["cholesky"]
    assert np.array_equal(newton_raphson_update(st, 0.5, solve="device"), -0.5 * x) and eng.methods[-1] == "lu"
    assert np.array_equal(newton_raphson_update(st, 0.5, solve="host"), host) and len(eng.methods) == 2
    NR = accelerate(ss.NewtonRaphson, solve="cholesky")
    res = NR(algo=_Algo(), damping_factor=0.5).compute_averaged_states(shared_states=st, _skip=True)
    assert np.array_equal(np.asarray(res.parameters_update[0]).reshape(-1), -0.5 * x) and eng.methods[-1] == "cholesky"
    # the environment overrides the argument, both ways, and is validated like it
    monkeypatch.setenv("FEDAGG_NR_SOLVE", "cholesky")
    assert np.array_equal(newton_raphson_update(st, 0.5, solve="host"), -0.5 * x) and eng.methods[-1] == "cholesky"
    monkeypatch.setenv("FEDAGG_NR_SOLVE", "host")
    calls = len(eng.methods)
    assert np.array_equal(newton_raphson_update(st, 0.5, solve="cholesky"), host) and len(eng.methods) == calls
    monkeypatch.setenv("FEDAGG_NR_SOLVE", "gpu")
    with pytest.raises(ValueError, match="'host', 'device' or 'cholesky'"):
        newton_raphson_update(st, 0.5, solve="cholesky")
    monkeypatch.delenv("FEDAGG_NR_SOLVE")
    # a decline takes the host solve with the engine's reason; a final info != 0 is NumPy's error
    eng.answer = (None, 0, "host: test decline")
    assert np.array_equal(newton_raphson_update(st, 0.5, solve="cholesky"), host)
    assert eng.last_timing["solve"] == "host: test decline"
    eng.answer = (x, 2, "device: lu after cholesky info=1")
    with pytest.raises(np.linalg.LinAlgError, match="Singular matrix"):
        newton_raphson_update(st, 0.5, solve="cholesky")


def test_engine_validates_the_method_and_declines_before_touching_the_device(monkeypatch):
    from substrafl_amd.engine import AggregationEngine

    def untouched(*a, **k):
        raise AssertionError("the engine was touched")

    monkeypatch.setattr(_native_dense, "load", untouched)
    monkeypatch.setattr(AggregationEngine, "session", untouched)
    eng = AggregationEngine.__new__(AggregationEngine)  # no device behind it
    solve = getattr(AggregationEngine.newton_raphson_solve, "__wrapped__", AggregationEngine.newton_raphson_solve)
    H, g = np.eye(3), np.ones(3)
    with pytest.raises(ValueError, match="method"):
        solve(eng, [[H]], [[g]], [1], method="qr")
    for method in ("lu", "cholesky"):  # the declines are the same ones, with the same words
        cases = {"float32 Hessian": ([[H.astype(np.float32)]], [[g]]), "float16 gradient": ([[H]], [[g.astype(np.float16)]]),
                 "shapes": ([[H[:, :2]]], [[g]]), "empty": ([[H[:0, :0]]], [[g[:0]]])}
        for word, (hs, gs) in cases.items():
            x, info, reason = solve(eng, hs, gs, [1], method=method)
            assert x is None and info == 0 and reason.startswith("host: ") and word in reason, (method, word, reason)


def test_default_class_never_maps_the_dense_library():
    """A fresh interpreter: an accelerated NewtonRaphson class with the default ``solve`` aggregates
    through an engine stand-in (NumPy's sums), gives ``np.linalg.solve``'s bits, and the process
    never imports the dense binding or maps libfedagg_dense.so."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import numpy as np\n"
            "import standin_substrafl.strategies as ss\n"
            "from standin_substrafl.strategies import schemas as sch\n"
            "import substrafl_amd.integration as I\n"
            "class E:\n"
            "    calls = 0\n"
            "    def sequential_sum(self, rows, n_samples):\n"
            "        E.calls += 1\n"
            "        n = sum(n_samples)\n"
            "        return [sum(r[0] * (k / n) for r, k in zip(rows, n_samples))]\n"
            "    def newton_raphson_solve(self, *a, **k):\n"
            "        raise AssertionError('the default took the device solve')\n"
            "I.engine_for = lambda device: E()\n"
            "class A: pass\n"
            "H = np.array([[4.0, 1.0], [1.0, 3.0]]); g = [np.array([1.0, 2.0], np.float32)]\n"
            "st = [sch.NewtonRaphsonSharedState(gradients=g, hessian=H, n_samples=2) for _ in range(2)]\n"
            "cls = I.accelerate(ss.NewtonRaphson)\n"
            "assert cls._fedagg_solve == 'host'\n"
            "r = cls(algo=A(), damping_factor=1.0).compute_averaged_states(shared_states=st, _skip=True)\n"
            "ref = -1.0 * np.linalg.solve(H * 0.5 + H * 0.5, (g[0] * 0.5 + g[0] * 0.5))\n"
            "assert np.asarray(r.parameters_update[0]).reshape(-1).tobytes() == ref.tobytes()\n"
            "assert E.calls == 2\n"
            "assert 'substrafl_amd._native_dense' not in sys.modules\n"
            "assert 'libfedagg_dense' not in open('/proc/self/maps').read()\n" % (str(ROOT), str(ROOT / "tests")))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300)
