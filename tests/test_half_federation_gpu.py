"""A federation of 16-bit models through the drop-in path: ``accelerate_algo(TorchFedAvgAlgo)``
clients (the stand-in classes of ``tests/standin_substrafl``, as ``tests/test_accelerate_algo.py``)
and ``accelerate(FedAvg)``.  Three clients, two rounds, a small MLP with BatchNorm whose running
statistics travel in the bucket.

* ``model.half()``: the same federation with the stand-in's own classes (per-layer torch ops, one
  pickled fp16 array per layer) aggregated by the reference's NumPy calls must give the same
  exports, averages and model states, bit for bit.
* ``model.to(torch.bfloat16)``: the reference cannot run it (``.numpy()`` has no bf16), so the
  comparison run restates the sequence: the client moves as torch ops on the device, the
  aggregation as the oracle on the exact fp32 upcasts, the update applied as
  ``w.data += 1.0 * torch.from_numpy(u).to(device)``.
"""

import numpy as np
import pytest
import torch

import standin_substrafl.strategies as ss
from standin_substrafl.algorithms.pytorch import TorchFedAvgAlgo
from standin_substrafl.algorithms.pytorch import _weights as w
from standin_substrafl.index_generator import NpIndexGenerator
from standin_substrafl.strategies import schemas as sch

from oracle import fedavg_explicit, fedavg_reference_structure
from substrafl_amd import wire

ROUNDS = 2
CLIENTS = 3


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


def _algo(base, dtype, client):
    torch.manual_seed(7)  # every client starts from the same initial weights
    model = torch.nn.Sequential(torch.nn.Linear(6, 24), torch.nn.BatchNorm1d(24), torch.nn.ReLU(),
                                torch.nn.Linear(24, 16), torch.nn.ReLU(), torch.nn.Linear(16, 1)).to(dtype)

    class MyAlgo(base):
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


def _bf16_reference_train(algo, data, avg):
    """TorchFedAvgAlgo.train (torch_fed_avg_algo.py:154-230) restated in per-layer torch ops for
    a bf16 model; the update leaves as its bit patterns."""
    ds = algo._dataset(data, is_inference=False)
    gen = algo._index_generator
    if avg is None:
        gen.n_samples = len(ds)
    else:
        with torch.no_grad():
            for p, u in zip(w.layers(algo._model, True), avg):
                p.data += 1.0 * torch.from_numpy(u).to(algo._device)
    gen.reset_counter()
    start = w.snapshot(algo._model, True)
    algo._model.train()
    algo._local_train(ds)
    gen.check_num_updates()
    algo._model.eval()
    delta = w.combine([w.snapshot(algo._model, True), start], [1, -1])
    w.rebind(algo._model, start, True)
    update = [t.detach().view(torch.int16).cpu().numpy().view(wire.BF16) for t in delta]
    return sch.FedAvgSharedState(n_samples=len(ds), parameters_update=update)


def _run(dtype, accelerated, use_wire=False):
    from substrafl_amd.integration import accelerate, accelerate_algo

    algos = []
    for k in range(CLIENTS):
        cls = _algo(TorchFedAvgAlgo, dtype, k)
        algos.append((accelerate_algo(cls, wire=use_wire) if accelerated else cls)())
    strategy = accelerate(ss.FedAvg)(algo=algos[0]) if accelerated else None
    trace, avg, states = [], None, None
    for _ in range(ROUNDS):
        if accelerated or dtype == torch.float16:
            states = [a.train(data_from_opener=d, shared_state=avg, _skip=True) for a, d in zip(algos, DATA)]
        else:
            states = [_bf16_reference_train(a, d, None if avg is None else list(avg.avg_parameters_update))
                      for a, d in zip(algos, DATA)]
        for a, s in zip(algos, states):
            trace += [("update", list(s.parameters_update)), ("model", _state(a)), ("n", [np.int64(s.n_samples)])]
        updates = [list(s.parameters_update) for s in states]
        ns = [s.n_samples for s in states]
        if accelerated:
            avg = strategy.avg_shared_states(shared_states=states, _skip=True)
        elif dtype == torch.float16:  # the reference's own NumPy calls (fed_avg.py:217-222)
            avg = sch.FedAvgAveragedState(avg_parameters_update=fedavg_reference_structure(updates, ns))
        else:  # the DESIGN §2 contract for bf16 buckets: the reference on the exact fp32 upcasts
            ups = [[wire.bf16_to_float32(a) for a in row] for row in updates]
            avg = sch.FedAvgAveragedState(avg_parameters_update=fedavg_explicit(ups, ns))
        trace.append(("avg", list(avg.avg_parameters_update)))
    return trace, algos, states


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from substrafl_amd import _native

    _native.load()
    torch.backends.cudnn.enabled = False  # the native BatchNorm kernels: deterministic training
    yield
    torch.backends.cudnn.enabled = True


@pytest.fixture(scope="module")
def reference_runs(gpu):
    """The comparison federation per dtype, run once and shared by the wire / plain cases."""
    return {dtype: _run(dtype, accelerated=False)[0] for dtype in (torch.float16, torch.bfloat16)}


@pytest.mark.gpu
@pytest.mark.parametrize("use_wire", [False, True], ids=["plain", "wire"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_half_federation_bit_identical(gpu, reference_runs, dtype, use_wire):
    from substrafl_amd.algorithms.weight_manager import flat_bucket, model_parameters

    acc, algos, states = _run(dtype, accelerated=True, use_wire=use_wire)
    _compare(reference_runs[dtype], acc)
    host_dtype = np.dtype(np.float16) if dtype == torch.float16 else wire.BF16
    avg_dtype = np.float16 if dtype == torch.float16 else np.float32  # bf16 buckets average into fp32
    assert all(a.dtype == host_dtype for s in states for a in s.parameters_update)
    assert all(np.asarray(a).dtype == avg_dtype for tag, layers in acc if tag == "avg" for a in layers)
    # the flat path ran: the weights are views of the one snapshot bucket set back after train,
    # and a wire export is one segment per client
    assert flat_bucket([p.data for p in model_parameters(algos[0].model, True)()]) is not None
    assert (wire.flat_of(list(states[1].parameters_update)) is not None) == use_wire
    assert np.isfinite(np.concatenate([np.asarray(a, dtype=np.float32).reshape(-1) for tag, layers in acc
                                       if tag == "avg" for a in layers])).all()  # a real training run
