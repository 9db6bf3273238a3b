"""The opt-in device solve of NewtonRaphson's Newton system (include/fedagg_dense.h,
substrafl_amd/csrc/dense.hip; ``accelerate(NewtonRaphson, solve="device")``), held to the standard
error bounds of LU with partial pivoting rather than to LAPACK's bits.

u = 2^-53, gamma_n = n u / (1 - n u).  Sizes: {1, 2, 3, 17}, then T - 1, T, T + 1 and 2 T + 1 for
every distinct blocking size T the library reports (``fedagg_dense_blocking``), and 5 max(T) + 7.
Matrix families (seeded ``default_rng``): symmetric diagonally dominant (gen_golden_nr._hessian's
recipe), standard normal, normal with an exactly zero diagonal, normal with the diagonal scaled by
1e-12, normal with rows scaled by 10^[-6, 6]; right-hand sides are fp32 values widened.

One case of that grid is singular by construction: n = 1 with an exactly zero diagonal is the
matrix [0].  There the tests assert what the contract says of a zero pivot (``info == 1``, no
fault) instead of an error bound on a solution that does not exist.
"""

import ctypes
import json
import shutil
import subprocess
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import standin_substrafl.strategies as ss
from standin_substrafl.strategies import schemas as sch

from oracle import newton_raphson_sums

gpu = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
D = ROOT / "tests" / "golden"
ETA_RECORD = ROOT / "profiles" / "dense_solve_eta.json"
U = 2.0 ** -53
FAMILIES = ("spd_dominant", "normal", "zero_diagonal", "tiny_diagonal", "row_scaled")
GUARD = 64  # elements of guard band behind every buffer


def _blocking():
    from substrafl_amd import _native_dense

    return _native_dense.blocking()


def _sizes():
    ts = sorted(set(_blocking()))
    out = {1, 2, 3, 17, 5 * max(ts) + 7}
    for t in ts:
        out |= {t - 1, t, t + 1, 2 * t + 1}
    assert max(out) <= 800
    return sorted(out)


def _gamma(n):
    return n * U / (1.0 - n * U)


def _matrix(family, n, seed=0):
    rng = np.random.default_rng([FAMILIES.index(family), n, seed])
    a = rng.standard_normal((n, n))
    if family == "spd_dominant":
        a = (a + a.T) * 0.5 + np.eye(n) * (n + 1.0)
    elif family == "zero_diagonal":
        a[np.diag_indices(n)] = 0.0
    elif family == "tiny_diagonal":
        a[np.diag_indices(n)] *= 1e-12
    elif family == "row_scaled":
        a *= 10.0 ** rng.uniform(-6, 6, (n, 1))
    g = rng.standard_normal(n).astype(np.float32).astype(np.float64)
    return np.ascontiguousarray(a), g


def _singular_by_construction(family, n):
    return family == "zero_diagonal" and n == 1


class Dev:
    """The library on torch-owned device buffers: every buffer is followed by a guard band."""

    def __init__(self):
        import torch

        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        from substrafl_amd import _native_dense

        self.torch = torch
        self.lib = _native_dense.load()
        self.check = _native_dense.check

    def run(self, A, b=None, lda=None, stream=None, fill_on_stream=False, what="solve"):
        """Factor (and with ``b`` solve) on the device.  Returns a dict: LU (n x n), ipiv, info, x,
        and ``intact``: whether the padding of every row and every guard band kept its bits.
        ``fill_on_stream``: A reaches its buffer by a device copy enqueued on ``stream`` directly
        before the library call (nothing synchronises in between)."""
        torch = self.torch
        n = A.shape[0]
        lda = n if lda is None else lda
        host = np.full((n, lda), np.nan)
        host[:, :n] = A
        guard = np.full(GUARD, -7.25)
        hA = np.concatenate([host.reshape(-1), guard])
        hb = np.concatenate([b if b is not None else np.zeros(n), guard])
        dA_src = torch.from_numpy(hA).cuda()
        db = torch.from_numpy(hb).cuda()
        di = torch.full((n + 1 + GUARD,), -77, dtype=torch.int32, device="cuda")  # ipiv, info, guard
        ws = int(self.lib.fedagg_dense_ws_bytes(n))
        dws = torch.full((ws // 8 + GUARD,), -7.25, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        st = stream if stream is not None else torch.cuda.current_stream()
        if fill_on_stream:
            dA = torch.full_like(dA_src, 3.0)  # what a solve that ran ahead of the copy would factor
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                dA.copy_(dA_src, non_blocking=True)
        else:
            dA = dA_src
        vp = ctypes.c_void_p
        sp = vp(st.cuda_stream)
        p_i, p_info = vp(di.data_ptr()), vp(di.data_ptr() + 4 * n)
        if what == "solve":
            self.check(self.lib.fedagg_dense_solve_f64(vp(dA.data_ptr()), n, lda, p_i, p_info, vp(db.data_ptr()),
                                                       vp(dws.data_ptr()), sp), "solve")
        else:
            self.check(self.lib.fedagg_dense_getrf_f64(vp(dA.data_ptr()), n, lda, p_i, p_info, vp(dws.data_ptr()), sp),
                       "getrf")
            if b is not None:
                self.check(self.lib.fedagg_dense_getrs_f64(vp(dA.data_ptr()), n, lda, p_i, vp(db.data_ptr()), sp), "getrs")
        st.synchronize()
        torch.cuda.synchronize()
        oA, ob, oi, ows = dA.cpu().numpy(), db.cpu().numpy(), di.cpu().numpy(), dws.cpu().numpy()
        full = oA[: n * lda].reshape(n, lda)
        same = lambda a, r: np.array_equal(np.asarray(a).view(np.uint8), np.asarray(r).view(np.uint8))  # noqa: E731
        intact = (same(full[:, n:], host[:, n:]) and same(oA[n * lda:], guard) and same(ob[n:], guard)
                  and same(oi[n + 1:], np.full(GUARD, -77, np.int32)) and same(ows, np.full(ws // 8 + GUARD, -7.25)))
        return {"LU": full[:, :n].copy(), "ipiv": oi[:n].copy(), "info": int(oi[n]), "x": ob[:n].copy(),
                "intact": intact}


@pytest.fixture(scope="module")
def dev():
    return Dev()


def _bits(a):
    a = np.asarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _apply_pivots(A, ipiv):
    PA = A.copy()
    for j, p in enumerate(ipiv):
        if p != j:
            PA[[j, p]] = PA[[p, j]]
    return PA


# ------------------------------------------------------------------ exact residual
def _scaled_ints(a):
    """``(ints, e)`` with ``a[k] == ints[k] * 2**e`` exactly (every double is a dyadic rational)."""
    a = np.asarray(a, np.float64).reshape(-1)
    m, e = np.frexp(a)
    mi = np.ldexp(m, 53).astype(np.int64)  # exact: 53 significant bits
    e = e.astype(np.int64) - 53
    nz = mi != 0
    emin = int(e[nz].min()) if nz.any() else 0
    return [int(v) << int(s - emin) if v else 0 for v, s in zip(mi.tolist(), e.tolist())], emin


def backward_error(H, x, g):
    """eta(x) = ||g - H x||inf / (||H||inf ||x||inf + ||g||inf), the residual computed exactly
    (integers scaled by powers of two, combined as ``fractions.Fraction``) and rounded once."""
    n = H.shape[0]
    hi, he = _scaled_ints(H)
    xi, xe = _scaled_ints(x)
    gi, ge = _scaled_ints(g)
    two = Fraction(2)
    sh, sg = two ** (he + xe), two ** ge
    r = 0.0
    for i in range(n):
        row = hi[i * n:(i + 1) * n]
        r = max(r, float(abs(Fraction(gi[i]) * sg - Fraction(sum(a * b for a, b in zip(row, xi))) * sh)))
    den = np.abs(H).sum(axis=1).max() * np.abs(x).max() + np.abs(g).max()
    return r / den


def test_backward_error_helper_is_exact():
    H = np.array([[1.0, 2.0 ** -60], [3.0, 1e-300]])
    x = np.array([1.0, 2.0 ** 60])
    g = np.array([2.0, 3.0])  # row 0: residual exactly 0 (float64 would round 1 + 1 - 2 fine, but row 1 not)
    r1 = Fraction(3) - Fraction(3) - Fraction(1e-300) * Fraction(2.0 ** 60)
    den = max(1.0 + 2.0 ** -60, 3.0 + 1e-300) * 2.0 ** 60 + 3.0
    assert backward_error(H, x, g) == float(abs(r1)) / den


# ------------------------------------------------------------------ 1. factorisation
@gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_factorisation_bounds(dev, family):
    for n in _sizes():
        A, _ = _matrix(family, n)
        out = dev.run(A, what="getrf")
        LU, ipiv = out["LU"], out["ipiv"]
        assert out["intact"], (family, n)
        assert out["info"] == (1 if _singular_by_construction(family, n) else 0), (family, n, out["info"])
        assert all(j <= int(p) < n for j, p in enumerate(ipiv)), (family, n)
        L = np.tril(LU, -1) + np.eye(n)
        Uf = np.triu(LU)
        assert np.all(np.abs(np.tril(LU, -1)) <= 1.0), (family, n, "a multiplier above 1: no pivoting")
        PA = _apply_pivots(A, ipiv)
        err = np.abs(PA - L @ Uf)
        bound = 3.0 * _gamma(n) * (np.abs(L) @ np.abs(Uf))
        worst = float((err - bound).max())
        assert np.all(err <= bound), (family, n, worst, np.unravel_index(np.argmax(err - bound), err.shape))
        # the pivot is the FIRST row of largest magnitude: replay the elimination on the host
        if n <= 65:
            W = A.copy()
            for j in range(n):
                p = j + int(np.argmax(np.abs(W[j:, j])))  # argmax returns the first maximum
                col = np.abs(W[j:, j])
                # the device's column differs from this replay by rounding only: accept any row that
                # is a maximum to within that rounding, and require the first one on exact ties
                if col.max() > 0 and np.sum(col >= col.max() * (1 - 1e-9)) == 1:
                    assert int(ipiv[j]) == p, (family, n, j)
                q = int(ipiv[j])
                W[[j, q]] = W[[q, j]]
                if W[j, j] != 0:
                    W[j + 1:, j] /= W[j, j]
                    W[j + 1:, j + 1:] -= np.outer(W[j + 1:, j], W[j, j + 1:])


@gpu
def test_first_of_equal_pivots_is_taken(dev):
    """Exact ties in every column: a unit diagonal and one more +-1 further down, 1 to 300 rows
    away (the same wave, another wave, another pass of the same thread).  No row has an entry right
    of its diagonal, so nothing fills in: the first row of largest magnitude is the diagonal at
    every step, no rows move, and the factors are the matrix itself, exactly."""
    n = 5 * max(_blocking()) + 7
    A = np.eye(n)
    for j, d in zip(range(n), [1, 2, 70, 129, 300] * n):
        if j + d < n:
            A[j + d, j] = -1.0 if j % 2 else 1.0
    out = dev.run(A, what="getrf")
    assert out["info"] == 0 and out["intact"]
    assert np.array_equal(out["ipiv"], np.arange(n))
    assert np.array_equal(out["LU"], A)


# ------------------------------------------------------------------ 2. solve
_eta = {}


@gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_solve_backward_error(dev, family):
    for n in _sizes():
        A, g = _matrix(family, n)
        out = dev.run(A, g)
        assert out["intact"], (family, n)
        if _singular_by_construction(family, n):
            assert out["info"] == 1
            _eta[f"{family}/{n}"] = {"n": n, "singular": True}
            continue
        assert out["info"] == 0
        eta_dev = backward_error(A, out["x"], g)
        eta_np = backward_error(A, np.linalg.solve(A, g), g)
        _eta[f"{family}/{n}"] = {"n": n, "eta_device_u": eta_dev / U, "eta_numpy_u": eta_np / U, "gate_u": n}
        print(f"{family} n={n}: eta device {eta_dev / U:.2f} u, numpy {eta_np / U:.2f} u, gate {n} u")
        assert eta_dev <= n * U, (family, n, eta_dev / U)
        # getrf + getrs is the same launch sequence as solve: the same bits
        two = dev.run(A, g, what="getrf+getrs")
        assert np.array_equal(_bits(two["x"]), _bits(out["x"])) and np.array_equal(_bits(two["LU"]), _bits(out["LU"]))


@gpu
def test_eta_record():
    """The record of the backward errors (device and ``np.linalg.solve``) per case; no second gate."""
    want = len(FAMILIES) * len(_sizes())
    if len(_eta) != want:
        return  # the solve cases did not all run in this session: the record is left as it is
    ETA_RECORD.write_text(json.dumps({"unit": "u = 2^-53", "blocking": list(_blocking()), "cases": _eta}, indent=1,
                                     sort_keys=True) + "\n")


# ------------------------------------------------------------------ 3. the reference's own outputs
class _Algo:
    pass


def _states(grads, hess, ns):
    return [sch.NewtonRaphsonSharedState(gradients=g, hessian=h, n_samples=n) for g, h, n in zip(grads, hess, ns)]


@gpu
def test_golden_updates_within_conditioning(dev):
    from substrafl_amd.engine import engine_for
    from substrafl_amd.integration import accelerate
    from substrafl_amd.integration import newton_raphson_sums as engine_sums

    NR = accelerate(ss.NewtonRaphson, solve="device")
    arrays = np.load(D / "golden_newton_raphson.npz", allow_pickle=False)
    meta = json.loads((D / "golden_newton_raphson_meta.json").read_text())
    for c in meta["cases"]:
        key, K, L = c["key"], c["K"], c["layers"]
        grads = [[arrays[f"{key}/k{k}/g{li}"] for li in range(L)] for k in range(K)]
        hess = [arrays[f"{key}/k{k}/h"] for k in range(K)]
        ns = [int(v) for v in arrays[f"{key}/n_samples"]]
        res = NR(algo=_Algo(), damping_factor=c["damping_factor"]).compute_averaged_states(
            shared_states=_states(grads, hess, ns), _skip=True)
        assert engine_for(None).last_timing["solve"] == "device", key
        ref = [arrays[f"{key}/out{i}"] for i in range(c["outputs"])]
        got = res.parameters_update
        assert len(got) == len(ref)
        for gi, ri in zip(got, ref):
            assert np.asarray(gi).dtype == ri.dtype and np.asarray(gi).shape == ri.shape, key
        H, G = engine_sums(_states(grads, hess, ns))
        Hr, Gr = newton_raphson_sums(grads, hess, ns)
        for a, r in ((H, Hr), (G, Gr)):  # the sums, through the refactored device-resident body
            assert a.dtype == r.dtype and np.array_equal(_bits(a), _bits(r)), key
        n = Hr.shape[0]
        gf = np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in got])
        rf = np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in ref])
        rel = np.abs(gf - rf).max() / np.abs(rf).max()
        gate = 4.0 * np.linalg.cond(Hr.astype(np.float64), np.inf) * n * U
        print(f"{key}: n={n} rel {rel:.3e} gate {gate:.3e}")
        assert rel <= gate, (key, rel, gate)


@gpu
def test_environment_override_and_host_fall_through(dev, monkeypatch):
    from substrafl_amd.engine import engine_for
    from substrafl_amd.integration import accelerate, newton_raphson_update

    rng = np.random.default_rng(5)
    P, K = 19, 3
    hess = [_matrix("spd_dominant", P, k)[0] for k in range(K)]
    grads = [[rng.standard_normal(P).astype(np.float32)] for _ in range(K)]
    st = _states(grads, hess, [3, 1, 4])
    host = newton_raphson_update(st, 0.5, solve="host")
    assert engine_for(None).last_timing["solve"] == "host"
    devu = newton_raphson_update(st, 0.5)
    assert engine_for(None).last_timing["solve"] == "device"
    assert devu.dtype == host.dtype and devu.shape == host.shape
    Hr, _ = newton_raphson_sums(grads, hess, [3, 1, 4])
    assert np.abs(devu - host).max() <= 4 * np.linalg.cond(Hr, np.inf) * P * U * np.abs(host).max()
    monkeypatch.setenv("FEDAGG_NR_SOLVE", "device")
    NR = accelerate(ss.NewtonRaphson)  # the default option, overridden by the environment
    res = NR(algo=_Algo(), damping_factor=0.5).compute_averaged_states(shared_states=st, _skip=True)
    assert engine_for(None).last_timing["solve"] == "device"
    assert np.array_equal(_bits(np.asarray(res.parameters_update[0]).reshape(-1)), _bits(devu))
    monkeypatch.setenv("FEDAGG_NR_SOLVE", "host")
    assert np.array_equal(_bits(newton_raphson_update(st, 0.5, solve="device")), _bits(host))
    monkeypatch.delenv("FEDAGG_NR_SOLVE")
    # an fp32 Hessian: NumPy solves it in single precision, so the host does, and says why
    st32 = _states(grads, [h.astype(np.float32) for h in hess], [3, 1, 4])
    u32 = newton_raphson_update(st32, 0.5, solve="device")
    reason = engine_for(None).last_timing["solve"]
    assert reason.startswith("host") and "float32" in reason
    H32, G32 = newton_raphson_sums(grads, [h.astype(np.float32) for h in hess], [3, 1, 4])
    ref32 = -0.5 * np.linalg.solve(H32, G32)
    assert u32.dtype == ref32.dtype and np.array_equal(_bits(u32), _bits(ref32))


# ------------------------------------------------------------------ 4. singular
@gpu
def test_zero_column_reports_its_pivot(dev):
    T = _blocking()
    for n, j in [(1, 0), (3, 1)] + [(t + 1, t) for t in sorted(set(T))] + [(max(T) + 1, 5)]:
        A, g = _matrix("normal", n, seed=9)
        A[:, j] = 0.0
        out = dev.run(A, g)
        assert out["info"] == j + 1, (n, j, out["info"])
        assert out["intact"]


@gpu
def test_singular_system_raises_linalgerror_on_both_routes(dev):
    from substrafl_amd.integration import accelerate

    P = 6
    hess = [_matrix("normal", P, k)[0] for k in range(2)]
    for h in hess:
        h[:, 2] = 0.0
    grads = [[np.ones(P, np.float32)] for _ in range(2)]
    for mode in ("device", "host"):
        NR = accelerate(ss.NewtonRaphson, solve=mode)
        with pytest.raises(np.linalg.LinAlgError, match="Singular matrix"):
            NR(algo=_Algo(), damping_factor=1.0).compute_averaged_states(shared_states=_states(grads, hess, [1, 2]),
                                                                          _skip=True)


# ------------------------------------------------------------------ 5. bounds
@gpu
def test_padding_and_guard_bands_untouched(dev):
    T = _blocking()
    for n in (T[0] + 1, 2 * max(T) + 2):
        A, g = _matrix("normal", n, seed=3)
        tight = dev.run(A, g)
        padded = dev.run(A, g, lda=n + 3)
        assert tight["intact"] and padded["intact"], n
        for k in ("LU", "ipiv", "x"):
            assert np.array_equal(_bits(padded[k]), _bits(tight[k])), (n, k)
        assert padded["info"] == tight["info"] == 0


# ------------------------------------------------------------------ 6. determinism and stream order
@gpu
def test_deterministic_and_ordered_by_the_stream(dev):
    n = 5 * max(_blocking()) + 7
    A, g = _matrix("normal", n, seed=4)
    first = dev.run(A, g)
    again = dev.run(A, g)
    side = dev.run(A, g, stream=dev.torch.cuda.Stream(), fill_on_stream=True)
    for other in (again, side):
        for k in ("LU", "ipiv", "x"):
            assert np.array_equal(_bits(other[k]), _bits(first[k])), k
        assert other["info"] == 0 and other["intact"]


# ------------------------------------------------------------------ 7. the default is unchanged
@gpu
def test_default_is_the_host_solve_and_never_loads_the_dense_library():
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import numpy as np\n"
            "import standin_substrafl.strategies as ss\n"
            "from standin_substrafl.strategies import schemas as sch\n"
            "from substrafl_amd.integration import accelerate\n"
            "from substrafl_amd.engine import engine_for\n"
            "class A: pass\n"
            "H = np.array([[4.0, 1.0], [1.0, 3.0]]); g = [np.array([1.0, 2.0], np.float32)]\n"
            "st = [sch.NewtonRaphsonSharedState(gradients=g, hessian=H, n_samples=2) for _ in range(2)]\n"
            "r = accelerate(ss.NewtonRaphson)(algo=A(), damping_factor=1.0).compute_averaged_states(shared_states=st, _skip=True)\n"
            "ref = -1.0 * np.linalg.solve(H * 0.5 + H * 0.5, (g[0] * 0.5 + g[0] * 0.5))\n"
            "assert np.array_equal(np.asarray(r.parameters_update[0]).reshape(-1), ref)\n"
            "assert engine_for(None).last_timing['solve'] == 'host'\n"
            "assert 'substrafl_amd._native_dense' not in sys.modules\n"
            "assert 'libfedagg_dense' not in open('/proc/self/maps').read()\n" % (str(ROOT), str(ROOT / "tests")))
    subprocess.run([sys.executable or shutil.which("python3"), "-c", code], check=True, timeout=120)
