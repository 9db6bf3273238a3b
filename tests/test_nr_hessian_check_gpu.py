"""The opt-in device Hessian check of NewtonRaphson's clients on the GPU:
``integration.newton_raphson_hessian_check`` (a Cholesky certificate first, the reference's
eigenvalue rule whenever that proves nothing) on Gram Hessians X^T D X / m + l2 I, and the
accelerated client class, ``accelerate_algo(TorchNewtonRaphsonAlgo, hessian_check="device")``,
against the un-accelerated stand-in on a 32-feature logistic regression with bias (P = 33, one
past the panel)."""

import numpy as np
import pytest

from test_dense_potrf_gpu import _gram

gpu = pytest.mark.gpu

SIZES = [33, 129, 327]


@pytest.fixture
def eig_calls(monkeypatch):
    import torch

    # as in a client's process, where the model is on the device before any check runs: torch
    # opens the GPU first, the engine's session after it
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.init()
    calls = []
    real = np.linalg.eig

    def counting(a):
        calls.append(a.shape)
        return real(a)

    monkeypatch.setattr(np.linalg, "eig", counting)
    monkeypatch.delenv("FEDAGG_NR_CHECK", raising=False)
    return calls


def _reference_raises(H):
    """torch_newton_raphson_algo.py:346-347 on ``H``."""
    return not (np.linalg.eig(H)[0].real >= 0).all()


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_positive_definite_hessians_are_accepted_on_the_device(n, eig_calls):
    from substrafl_amd.engine import engine_for
    from substrafl_amd.integration import last_hessian_check, newton_raphson_hessian_check

    for H in (_gram(n, 4 * n, 0.0), _gram(n, n // 2, 1e-3)):
        before = H.copy()
        assert newton_raphson_hessian_check(H, 0.0, check="device") == "device"
        assert eig_calls == [], "the eigenvalues were computed"
        assert last_hessian_check["route"] == "device"
        tm = engine_for(None).last_timing
        assert tm["P"] == n and tm["check"] == "device" and {"stage_s", "factor_ms", "fetch_s", "total_s"} <= set(tm)
        assert H.flags.writeable and np.array_equal(H, before)


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_singular_hessian_goes_to_the_reference_rule(n, eig_calls):
    """m = n / 2 and no l2 term: rank n / 2 exactly.  The Cholesky meets a pivot that is not > 0 and
    proves nothing; the outcome is the reference rule's on the same matrix, whichever that is."""
    from substrafl_amd.engine import engine_for
    from substrafl_amd.exceptions import NegativeHessianMatrixError
    from substrafl_amd.integration import last_hessian_check, newton_raphson_hessian_check

    H = _gram(n, n // 2, 0.0)
    ok, info, reason = engine_for(None).hessian_cholesky_check(H)
    assert ok is False and info != 0 and 1 <= info <= n and reason == "device"
    raises = _reference_raises(H)
    del eig_calls[:]
    if raises:
        with pytest.raises(NegativeHessianMatrixError, match="Calculated eigenvalues are"):
            newton_raphson_hessian_check(H, 0.0, check="device")
    else:
        assert newton_raphson_hessian_check(H, 0.0, check="device") == f"host after device info={info}"
    assert len(eig_calls) == 1
    assert last_hessian_check["route"] == f"host after device info={info}"
    assert last_hessian_check["route"].startswith("host after device")


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_indefinite_hessian_raises_with_the_eigenvalues(n, eig_calls):
    from substrafl_amd.integration import last_hessian_check, newton_raphson_hessian_check

    class Mine(Exception):
        pass

    G = _gram(n, 4 * n, 0.0)
    lam = np.linalg.eigvalsh(G)
    H = G - (lam[0] + 1e-6 * lam[-1]) * np.eye(n)
    assert np.array_equal(H, H.T)
    with pytest.raises(Mine) as e:
        newton_raphson_hessian_check(H, 0.125, check="device", error_cls=Mine)
    assert last_hessian_check["route"].startswith("host after device info=")
    eigenvalues = np.linalg.eig(H)[0].real
    assert f"Calculated eigenvalues are {eigenvalues.tolist()} and considered l2_coeff is 0.125" in str(e.value)


@gpu
def test_environment_override_and_declined_hessians(eig_calls, monkeypatch):
    from substrafl_amd.integration import newton_raphson_hessian_check

    H = _gram(33, 132, 0.0)
    monkeypatch.setenv("FEDAGG_NR_CHECK", "device")
    assert newton_raphson_hessian_check(H, 0.0, check="host") == "device" and eig_calls == []
    monkeypatch.setenv("FEDAGG_NR_CHECK", "host")
    assert newton_raphson_hessian_check(H, 0.0, check="device") == "host" and len(eig_calls) == 1
    monkeypatch.delenv("FEDAGG_NR_CHECK")
    skew = H.copy()
    skew[5, 2] = np.nextafter(skew[5, 2], 1.0)
    assert newton_raphson_hessian_check(skew, 0.0).startswith("host: ")
    assert newton_raphson_hessian_check(H.astype(np.float32), 0.0).startswith("host: ")
    assert len(eig_calls) == 3


# ------------------------------------------------------------------ the client class
FEATURES = 32


def _client_data(seed, m=96):
    import torch

    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, FEATURES, generator=g)
    y = (torch.rand(m, 1, generator=g) < torch.sigmoid(x[:, :1])).float()
    return x, y


def _make(cls, l2_coeff):
    import torch

    class DS(torch.utils.data.Dataset):
        def __init__(self, d, is_inference=False):
            self.x, self.y = d

        def __len__(self):
            return len(self.x)

        def __getitem__(self, i):
            return self.x[i], self.y[i]

    torch.manual_seed(7)
    model = torch.nn.Sequential(torch.nn.Linear(FEATURES, 1), torch.nn.Sigmoid())
    return cls(model, torch.nn.BCELoss(), 40, DS, l2_coeff=l2_coeff)


@gpu
def test_accelerated_client_matches_the_plain_one_bit_for_bit(eig_calls):
    import torch
    from standin_substrafl.algorithms.pytorch import torch_newton_raphson_algo as nr

    from substrafl_amd.integration import accelerate_algo

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    fast_cls = accelerate_algo(nr.TorchNewtonRaphsonAlgo, hessian_check="device")
    for client in range(2):
        data = _client_data(client)
        plain = _make(nr.TorchNewtonRaphsonAlgo, 1e-3).train(shared_state=None, data_from_opener=data, _skip=True)
        assert len(eig_calls) == client + 1  # the plain client's own check
        algo = _make(fast_cls, 1e-3)
        assert next(algo.model.parameters()).is_cuda
        fast = algo.train(shared_state=None, data_from_opener=data, _skip=True)
        assert len(eig_calls) == client + 1, "the accelerated client computed eigenvalues"
        assert algo._fedagg_hessian_route == "device"
        assert fast.n_samples == plain.n_samples == 96
        assert fast.hessian.shape == (FEATURES + 1, FEATURES + 1) and fast.hessian.dtype == np.float64
        assert fast.hessian.tobytes() == plain.hessian.tobytes()
        assert len(fast.gradients) == len(plain.gradients) == 2
        for a, b in zip(fast.gradients, plain.gradients):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@gpu
def test_accelerated_client_applies_the_averaged_update_like_the_plain_one(eig_calls):
    """Round 2: the averaged update (float64 layers, as the aggregator's unflatten returns them)
    goes onto the model before the pass; Hessian and gradients still agree bit for bit."""
    from standin_substrafl.algorithms.pytorch import torch_newton_raphson_algo as nr
    from standin_substrafl.strategies.schemas import NewtonRaphsonAveragedStates

    from substrafl_amd.integration import accelerate_algo

    data = _client_data(3)
    rng = np.random.default_rng(3)
    update = NewtonRaphsonAveragedStates(parameters_update=[rng.standard_normal((1, FEATURES)) * 0.1,
                                                            rng.standard_normal(1) * 0.1])
    outs = []
    for cls in (nr.TorchNewtonRaphsonAlgo, accelerate_algo(nr.TorchNewtonRaphsonAlgo, hessian_check="device")):
        algo = _make(cls, 1e-3)
        algo.train(shared_state=None, data_from_opener=data, _skip=True)
        outs.append(algo.train(shared_state=update, data_from_opener=data, _skip=True))
        outs.append([p.detach().cpu().numpy() for p in algo.model.parameters()])
    (plain, w_plain, fast, w_fast) = outs
    assert fast.hessian.tobytes() == plain.hessian.tobytes()
    for a, b in zip(fast.gradients + w_fast, plain.gradients + w_plain):
        assert a.tobytes() == b.tobytes()


@gpu
def test_indefinite_hessian_raises_the_same_class_from_both_clients(eig_calls):
    from standin_substrafl.algorithms.pytorch import torch_newton_raphson_algo as nr

    from substrafl_amd.integration import accelerate_algo

    data = _client_data(0)
    fast_cls = accelerate_algo(nr.TorchNewtonRaphsonAlgo, hessian_check="device")
    raised = []
    for cls in (nr.TorchNewtonRaphsonAlgo, fast_cls):
        algo = _make(cls, -10.0)  # H - 10 I: every eigenvalue of a logistic Hessian is below 1 here
        with pytest.raises(nr.NegativeHessianMatrixError) as e:
            algo.train(shared_state=None, data_from_opener=data, _skip=True)
        raised.append(type(e.value))
    assert raised[0] is raised[1] is nr.NegativeHessianMatrixError
    assert algo._fedagg_hessian_route is None  # the check raised before the route was kept on the instance
    from substrafl_amd.integration import last_hessian_check

    assert last_hessian_check["route"].startswith("host after device info=")
