"""A Scaffold federation of 16-bit models through the drop-in path:
``accelerate_algo(TorchScaffoldAlgo)`` clients (the stand-in classes of ``tests/standin_substrafl``)
and ``accelerate(Scaffold)``.  Three clients, two rounds, a small MLP with BatchNorm.  Round 1
ships 16-bit deltas, control-variate updates and c; from round 2 on the server's fp64 c comes back
and torch's promotion makes the control-variate bucket and c fp64 next to 16-bit deltas.

* ``model.half()``: the same federation with the stand-in's own classes aggregated by the
  reference's NumPy calls must give the same exports, averages, c and model states, bit for bit.
* ``model.to(torch.bfloat16)``: the reference cannot run it (``.numpy()`` has no bf16), so the
  comparison run restates the sequence: the stand-in's client moves as per-layer torch ops (with
  torch's promotion in round 2), bf16 tensors leaving as their bit patterns, the aggregation as the
  oracle on the exact fp32 upcasts.
"""

import numpy as np
import pytest
import torch

import standin_substrafl.strategies as ss
from standin_substrafl.algorithms.pytorch import TorchScaffoldAlgo
from standin_substrafl.algorithms.pytorch import _weights as w
from standin_substrafl.index_generator import NpIndexGenerator
from standin_substrafl.strategies import schemas as sch

from oracle import scaffold_reference_structure
from substrafl_amd import wire

ROUNDS = 2
CLIENTS = 3
LR = 0.7


def _data(n, seed):
    r = np.random.default_rng(seed)
    x = r.standard_normal((n, 6)).astype(np.float32)
    y = (x @ r.standard_normal((6, 1)) + 0.1 * r.standard_normal((n, 1))).astype(np.float32)
    return x, y


DATA = [_data(200, 1), _data(130, 2), _data(77, 3)]


def _dataset(dtype):
    class XY(torch.utils.data.Dataset):
        def __init__(self, data_from_opener, is_inference=False):
            self.x, self.y = data_from_opener

        def __getitem__(self, i):
            return torch.from_numpy(self.x[i]).to(dtype), torch.from_numpy(self.y[i]).to(dtype)

        def __len__(self):
            return len(self.x)

    return XY


def _algo(dtype, client):
    torch.manual_seed(7)  # every client starts from the same initial weights
    model = torch.nn.Sequential(torch.nn.Linear(6, 24), torch.nn.BatchNorm1d(24), torch.nn.ReLU(),
                                torch.nn.Linear(24, 16), torch.nn.ReLU(), torch.nn.Linear(16, 1)).to(dtype)

    class MyAlgo(TorchScaffoldAlgo):
        def __init__(self):
            super().__init__(model=model, criterion=torch.nn.MSELoss(),
                             optimizer=torch.optim.SGD(model.parameters(), lr=0.02 * (1 + 0.25 * client)),
                             index_generator=NpIndexGenerator(batch_size=32, num_updates=5, seed=11 + client),
                             dataset=_dataset(dtype), with_batch_norm_parameters=True, disable_gpu=False)

    return MyAlgo


def _bits(a):
    a = np.asarray(a).view(np.ndarray)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _state(algo):
    out = []
    for t in algo.model.state_dict().values():
        t = t.detach()
        out.append((t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy().copy())
    return out


def _compare(ref, acc):
    assert [t for t, _ in ref] == [t for t, _ in acc]
    for (tag, r), (_, a) in zip(ref, acc):
        assert len(r) == len(a), tag
        for x, y in zip(r, a):
            x, y = np.asarray(x), np.asarray(y)
            assert x.dtype == y.dtype and x.shape == y.shape, (tag, x.dtype, y.dtype, x.shape, y.shape)
            assert np.array_equal(_bits(x), _bits(y)), tag


def _host(ts):
    return [t.detach().view(torch.int16).cpu().numpy().view(wire.BF16) if t.dtype == torch.bfloat16
            else t.cpu().detach().numpy() for t in ts]


def _bf16_reference_train(algo, data, shared_state):
    """The stand-in's ``TorchScaffoldAlgo.train`` restated for a bf16 model: the same per-layer
    torch ops, bf16 tensors leaving as their bit patterns."""
    bn = algo._with_batch_norm_parameters
    ds = algo._dataset(data, is_inference=False)
    gen = algo._index_generator
    if shared_state is None:
        gen.n_samples = len(ds)
        algo._client_control_variate = w.zeros(algo.model, bn, algo._device)
        algo._server_control_variate = w.zeros(algo.model, bn, algo._device)
    else:
        w.add_into(algo._model, [torch.from_numpy(a).to(algo._device) for a in shared_state.avg_parameters_update], bn)
        algo._server_control_variate = [torch.from_numpy(a).to(algo._device)
                                        for a in shared_state.server_control_variate]
    gen.reset_counter()
    start = w.snapshot(algo._model, bn)
    algo._delta_variate = w.combine([algo._client_control_variate, algo._server_control_variate], [1, -1])
    algo._model.train()
    algo._local_train(ds)
    gen.check_num_updates()
    assert algo._scaffold_parameters_update_num_call == gen._num_updates
    algo._reset_scaffold_parameters_update()
    algo._model.eval()
    delta = w.combine([w.snapshot(algo._model, bn), start], [1, -1])
    cv_update = w.combine([algo._server_control_variate, delta], [-1.0, -1.0 / (algo._current_lr * gen.num_updates)])
    algo._client_control_variate = w.combine([algo._client_control_variate, cv_update], [1, 1])
    w.rebind(algo._model, start, bn)
    return sch.ScaffoldSharedState(parameters_update=_host(delta), control_variate_update=_host(cv_update),
                                   server_control_variate=_host(algo._server_control_variate), n_samples=len(ds))


def _up(a):
    return wire.bf16_to_float32(a) if wire.is_bf16(a) else np.asarray(a)


def _run(dtype, accelerated):
    from substrafl_amd.integration import accelerate, accelerate_algo

    algos = []
    for k in range(CLIENTS):
        cls = _algo(dtype, k)
        algos.append((accelerate_algo(cls) if accelerated else cls)())
    strategy = accelerate(ss.Scaffold)(algo=algos[0], aggregation_lr=LR) if accelerated else None
    trace, avg, kinds = [], None, []
    for _ in range(ROUNDS):
        if accelerated or dtype == torch.float16:
            states = [a.train(data_from_opener=d, shared_state=avg, _skip=True) for a, d in zip(algos, DATA)]
        else:
            states = [_bf16_reference_train(a, d, avg) for a, d in zip(algos, DATA)]
        for a, s in zip(algos, states):
            trace += [("delta", list(s.parameters_update)), ("cv", list(s.control_variate_update)),
                      ("c", list(s.server_control_variate)), ("model", _state(a)), ("n", [np.int64(s.n_samples)])]
        if accelerated:
            from substrafl_amd.engine import engine_for

            avg = strategy.avg_shared_states(shared_states=states, _skip=True)
            kinds.append(engine_for(None).last_timing.get("bucket_kinds"))
        else:  # the reference's own NumPy calls (scaffold.py:204-337), bf16 on its exact fp32 upcasts
            up = lambda rows: [[_up(a) for a in row] for row in rows]  # noqa: E731
            new_c, upd = scaffold_reference_structure(up([s.parameters_update for s in states]),
                                                      up([s.control_variate_update for s in states]),
                                                      [_up(a) for a in states[0].server_control_variate],
                                                      [s.n_samples for s in states], LR)
            avg = sch.ScaffoldAveragedStates(server_control_variate=new_c, avg_parameters_update=upd)
        trace += [("avg", list(avg.avg_parameters_update)), ("new_c", list(avg.server_control_variate))]
    return trace, kinds


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from substrafl_amd import _native

    _native.load()
    torch.backends.cudnn.enabled = False  # the native BatchNorm kernels: deterministic training
    yield
    torch.backends.cudnn.enabled = True


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_scaffold_16_bit_federation_bit_identical(gpu, dtype):
    ref, _ = _run(dtype, accelerated=False)
    acc, kinds = _run(dtype, accelerated=True)
    _compare(ref, acc)
    k16 = "f16" if dtype == torch.float16 else "bf16"
    # round 1: three 16-bit lists; round 2: the fp64 c came back and promoted the control variates
    assert kinds == [(k16, k16, k16), (k16, "f64", "f64")]
    host16 = np.dtype(np.float16) if dtype == torch.float16 else wire.BF16
    assert all(np.asarray(a).dtype == host16 for tag, layers in acc if tag == "delta" for a in layers)
    assert all(np.asarray(a).dtype == np.float64 for tag, layers in acc if tag in ("avg", "new_c") for a in layers)
    assert np.isfinite(np.concatenate([np.asarray(a).reshape(-1) for tag, layers in acc
                                       if tag in ("avg", "new_c") for a in layers])).all()  # a real training run
