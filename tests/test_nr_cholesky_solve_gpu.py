"""``accelerate(NewtonRaphson, solve="cholesky")`` on the GPU (integration.newton_raphson_update,
engine.AggregationEngine.newton_raphson_solve with ``method="cholesky"``): a Hessian sum that is
symmetric positive definite is solved from its Cholesky factor and held to Higham's thm 10.4; any other
sum takes the LU of ``solve="device"``, bit for bit, and the route says why.

The bound, |G - H x| <= gamma_{3n+3} |L| |L^T| |x| with the exact residual, is that of
tests/test_dense_posv_gpu.py against the exactly summed system (``oracle.newton_raphson_sums``).  The
device's factor stays in HBM, so |L| is LAPACK's factor of the same sum here: the two agree to a
relative kappa(H) u (kappa below 100 for these Gram matrices), which moves the bound by as little."""

import numpy as np
import pytest

import standin_substrafl.strategies as ss

from oracle import newton_raphson_sums
from test_dense_posv_gpu import _eta, _exact_rhs, _residual
from test_dense_potrf_gpu import _exact_factor, _gram
from test_dense_solve_gpu import U, _Algo, _bits, _gamma, _states

gpu = pytest.mark.gpu

NS = [3, 1, 4]


def _timing():
    from substrafl_amd.engine import engine_for

    return engine_for(None).last_timing


@pytest.fixture(autouse=True)
def _no_override(monkeypatch):
    monkeypatch.delenv("FEDAGG_NR_SOLVE", raising=False)


def _gram_clients(P, shift=0.0):
    rng = np.random.default_rng([P, 11])
    hess = [_gram(P, 4 * P, 0.0, seed=k) - shift * np.eye(P) for k in range(3)]
    grads = [[rng.standard_normal(P)] for _ in range(3)]
    return grads, hess


@gpu
@pytest.mark.parametrize("P", [33, 129, 327])
def test_gram_hessians_take_the_cholesky_route_within_the_bound(P, monkeypatch):
    from substrafl_amd.integration import newton_raphson_update

    grads, hess = _gram_clients(P)
    H, G = newton_raphson_sums(grads, hess, NS)
    assert np.array_equal(H, H.T)
    L = np.linalg.cholesky(H)  # (raises unless positive definite) -- before the patch below

    def refuse(*a, **k):
        raise AssertionError("np.linalg.solve was called on the device route")

    monkeypatch.setattr(np.linalg, "solve", refuse)
    update = newton_raphson_update(_states(grads, hess, NS), 1.0, solve="cholesky")
    tm = _timing()
    assert tm["solve"] == "device: cholesky" and tm["P"] == P
    assert {"symcopy_ms", "factor_ms", "substitute_ms", "sums_ms", "fetch_s", "total_s"} <= set(tm) and "lu_factor_ms" not in tm
    x = -update
    r = _residual(H, x, G)
    bound = _gamma(3 * P + 3) * (np.abs(L) @ (np.abs(L).T @ np.abs(x)))
    eta_u = _eta(H, x, G, r) / U
    print(f"P={P}: |r| / bound {float((r / bound).max()):.4f}, eta {eta_u:.2f} u, gate {P} u")
    assert np.all(r <= bound), (P, float((r / bound).max()))
    assert eta_u <= P, (P, eta_u)


def _both_routes(grads, hess):
    from substrafl_amd.integration import newton_raphson_update

    st = _states(grads, hess, NS)
    lu = newton_raphson_update(st, 0.5, solve="device")
    assert _timing()["solve"] == "device"
    chol = newton_raphson_update(st, 0.5, solve="cholesky")
    return lu, chol, _timing()


@gpu
def test_one_ulp_of_asymmetry_takes_the_lu_bit_for_bit():
    P = 129
    grads, hess = _gram_clients(P)
    # one entry of one client's Hessian, one ulp up: the first one that survives the weighted sum's roundings
    for i, j in [(5, 2), (70, 3), (128, 64), (100, 99), (64, 63), (17, 0), (90, 31), (127, 1)]:
        skew = [h.copy() for h in hess]
        skew[1][i, j] = np.nextafter(skew[1][i, j], np.inf)
        H, _ = newton_raphson_sums(grads, skew, NS)
        if not np.array_equal(H, H.T):
            break
    else:
        raise AssertionError("no candidate entry makes the sum non-symmetric")
    lu, chol, tm = _both_routes(grads, skew)
    assert tm["solve"] == "device: lu, the Hessian sum does not equal its transpose"
    assert {"symcopy_ms", "factor_ms", "substitute_ms", "lu_factor_ms", "lu_substitute_ms"} <= set(tm)
    assert chol.dtype == lu.dtype and np.array_equal(_bits(chol), _bits(lu))


@gpu
def test_indefinite_symmetric_sum_takes_the_lu_bit_for_bit():
    P = 129
    grads, hess = _gram_clients(P, shift=0.2)
    H, _ = newton_raphson_sums(grads, hess, NS)
    ev = np.linalg.eigvalsh(H)
    assert np.array_equal(H, H.T) and ev[0] < -0.01 and ev[-1] > 0.01
    lu, chol, tm = _both_routes(grads, hess)
    assert tm["solve"].startswith("device: lu after cholesky info="), tm["solve"]
    assert 1 <= int(tm["solve"].rsplit("=", 1)[1]) <= P
    assert chol.dtype == lu.dtype and np.array_equal(_bits(chol), _bits(lu))


@gpu
def test_singular_symmetric_sum_raises_linalgerror():
    from substrafl_amd.integration import accelerate

    P = 40
    grads, hess = _gram_clients(P)
    for h in hess:
        h[:, 7] = 0.0
        h[7, :] = 0.0
    NR = accelerate(ss.NewtonRaphson, solve="cholesky")
    with pytest.raises(np.linalg.LinAlgError, match="Singular matrix"):
        NR(algo=_Algo(), damping_factor=1.0).compute_averaged_states(shared_states=_states(grads, hess, NS), _skip=True)
    assert _timing()["solve"] == "device: lu after cholesky info=8"


@gpu
def test_fp32_hessian_takes_the_host_solve_and_the_environment_overrides(monkeypatch):
    from substrafl_amd.integration import newton_raphson_update

    P = 33
    grads, hess = _gram_clients(P)
    st = _states(grads, hess, NS)
    host = newton_raphson_update(st, 0.5, solve="host")
    assert _timing()["solve"] == "host"
    chol = newton_raphson_update(st, 0.5, solve="cholesky")
    assert _timing()["solve"] == "device: cholesky"
    monkeypatch.setenv("FEDAGG_NR_SOLVE", "cholesky")
    assert np.array_equal(_bits(newton_raphson_update(st, 0.5, solve="host")), _bits(chol))
    assert _timing()["solve"] == "device: cholesky"
    monkeypatch.setenv("FEDAGG_NR_SOLVE", "host")
    assert np.array_equal(_bits(newton_raphson_update(st, 0.5, solve="cholesky")), _bits(host))
    assert _timing()["solve"] == "host"
    monkeypatch.delenv("FEDAGG_NR_SOLVE")
    # an fp32 Hessian: NumPy solves it in single precision, so the host does, with today's reason
    h32 = [h.astype(np.float32) for h in hess]
    u32 = newton_raphson_update(_states(grads, h32, NS), 0.5, solve="cholesky")
    reason = _timing()["solve"]
    assert reason.startswith("host") and "float32" in reason
    newton_raphson_update(_states(grads, h32, NS), 0.5, solve="device")
    assert _timing()["solve"] == reason
    H32, G32 = newton_raphson_sums(grads, h32, NS)
    ref32 = -0.5 * np.linalg.solve(H32, G32)
    assert u32.dtype == ref32.dtype and np.array_equal(_bits(u32), _bits(ref32))


@gpu
@pytest.mark.parametrize("gdtype", [np.float64, np.float32], ids=["f64_gradients", "f32_gradients"])
def test_strategy_route_exact(gdtype):
    """``newton_raphson_update`` and the accelerated strategy on a system of the exact family: two
    clients of equal weight with H_0 = A + D, H_1 = A - D (D symmetric, multiples of 1/4) and
    g_0 = g_1 = b, so both sums are exact, the sum is symmetric and the update is -x, exactly.
    fp32 gradients (b fits fp32 exactly) go through the ``fedagg_cast`` widening ahead of the solve."""
    from substrafl_amd.integration import accelerate, newton_raphson_update

    P = 129
    A = _exact_factor(P)[0]
    _, x, b = _exact_rhs(P)
    Dm = np.random.default_rng([P, 1]).integers(-8, 9, (P, P)).astype(np.float64) / 4.0
    Dm = np.tril(Dm) + np.tril(Dm, -1).T
    hess = [A + Dm, A - Dm]
    assert np.array_equal(b.astype(gdtype).astype(np.float64), b)
    shapes = [(P - 77,), (7, 11)]
    split = lambda v: [v[:P - 77].reshape(shapes[0]).copy(), v[P - 77:].reshape(shapes[1]).copy()]  # noqa: E731
    grads = [split(b.astype(gdtype)) for _ in range(2)]
    Hs, Gs = newton_raphson_sums(grads, hess, [1, 1])
    assert np.array_equal(Hs, A) and Gs.dtype == gdtype and np.array_equal(Gs.astype(np.float64), b)
    st = _states(grads, hess, [1, 1])
    update = newton_raphson_update(st, 1.0, solve="cholesky")
    assert _timing()["solve"] == "device: cholesky" and _timing()["P"] == P
    assert update.dtype == np.float64 and np.array_equal(update, -x), np.flatnonzero(update != -x)[:4]
    NR = accelerate(ss.NewtonRaphson, solve="cholesky")
    res = NR(algo=_Algo(), damping_factor=1.0).compute_averaged_states(shared_states=st, _skip=True)
    assert _timing()["solve"] == "device: cholesky"
    got = res.parameters_update
    assert len(got) == 2
    for gi, ri, shp in zip(got, split(-x), shapes):
        assert np.asarray(gi).shape == shp and np.array_equal(np.asarray(gi), ri)


@gpu
def test_accelerated_strategy_equals_newton_raphson_update():
    from substrafl_amd.integration import accelerate, newton_raphson_update

    P = 65
    grads, hess = _gram_clients(P)
    st = _states(grads, hess, NS)
    update = newton_raphson_update(st, 0.5, solve="cholesky")
    NR = accelerate(ss.NewtonRaphson, solve="cholesky")
    res = NR(algo=_Algo(), damping_factor=0.5).compute_averaged_states(shared_states=st, _skip=True)
    assert _timing()["solve"] == "device: cholesky"
    assert np.array_equal(_bits(np.asarray(res.parameters_update[0]).reshape(-1)), _bits(update))
