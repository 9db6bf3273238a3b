"""``wire.BF16`` layers through the drop-in host path (``engine.fedavg``,
``strategies.FedAvg.avg_shared_states``): the rows are staged as raw 2-byte elements, the bf16
kernels average them, and the result is float32 -- the oracle's explicit-order FedAvg on the exact
fp32 upcasts, bit for bit (where the oracle gives NaN only NaN-ness is compared)."""

import numpy as np
import pytest

from oracle.aggregation import fedavg_explicit
from substrafl_amd import wire

SHAPES = [(3, 5), (1,), (), (257,), (4099,)]  # numel == 1 and 0-d: the pairwise path; vector remainders


def _clients(K, shapes, seed, nonfinite=0.0):
    """K clients' bf16 layers (as wire.BF16 arrays), their exact fp32 upcasts, uneven n_samples."""
    rng = np.random.default_rng(seed)
    pus, ups = [], []
    for _ in range(K):
        row = []
        for s in shapes:
            x = np.asarray(rng.standard_normal(s), dtype=np.float32) * np.float32(10.0 ** int(rng.integers(-3, 4)))
            b = wire.float32_to_bf16(x)
            if nonfinite:
                u = np.asarray(b).view(np.uint16).copy()
                pick = np.asarray(rng.random(u.shape) < nonfinite)
                special = np.asarray(rng.choice(np.array([0x7F80, 0xFF80, 0x7FC0, 0xFFC1], np.uint16), u.shape))
                u = np.where(pick, special, u).astype(np.uint16)
                b = u.view(wire.BF16)
            row.append(b)
        pus.append(row)
        ups.append([wire.bf16_to_float32(a) for a in row])
    ns = [int(v) for v in rng.integers(1, 5000, K)]
    return pus, ups, ns


def _as_buckets(pus):
    return [wire.pack(row) for row in pus]


def _assert_same(got, ref):
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        g, r = np.asarray(g), np.asarray(r)
        assert g.dtype == np.float32 and r.dtype == np.float32 and g.shape == r.shape
        nan = np.isnan(r)
        assert np.array_equal(np.isnan(g), nan)
        assert np.array_equal(g.view(np.uint32)[~nan], r.view(np.uint32)[~nan])


@pytest.fixture(scope="module")
def cases():
    """The inputs and the oracle's result per client count, computed once and left unchanged."""
    out = {}
    for K in (1, 2, 3, 9, 130):
        pus, ups, ns = _clients(K, SHAPES, K)
        out[K] = (pus, ns, fedavg_explicit(ups, ns))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["plain", "bucket"])
@pytest.mark.parametrize("K", [1, 2, 3, 9, 130])  # 130 crosses the 128-client chunk
def test_engine_fedavg_bf16_bit_exact(cases, K, form):
    from substrafl_amd.engine import AggregationEngine

    pus, ns, ref = cases[K]
    rows = _as_buckets(pus) if form == "bucket" else pus
    if form == "bucket":
        assert all(wire.flat_of(r) is not None for r in rows)  # one segment per client
    eng = AggregationEngine(device=0)
    got = eng.fedavg(rows, ns)
    assert eng.last_timing["layout"] == "rows"
    _assert_same(got, ref)
    got = eng.fedavg(rows, ns, wire=True)
    _assert_same(got, ref)


@pytest.mark.gpu
def test_engine_fedavg_bf16_nonfinite_inputs():
    from substrafl_amd.engine import AggregationEngine

    pus, ups, ns = _clients(3, SHAPES, 77, nonfinite=0.3)
    _assert_same(AggregationEngine(device=0).fedavg(_as_buckets(pus), ns), fedavg_explicit(ups, ns))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["plain", "bucket"])
def test_engine_fedavg_bf16_tile_interleaved(form):
    from substrafl_amd.engine import AggregationEngine

    shapes = [(3, 5), (1,), (2 * 32768 + 12345,), (257,)]
    pus, ups, ns = _clients(5, shapes, 5)
    eng = AggregationEngine(device=0)
    eng.tiled = True  # the layout is recommended only for many clients over many tiles; forced here
    got = eng.fedavg(_as_buckets(pus) if form == "bucket" else pus, ns)
    assert eng.last_timing["layout"] == "tiles"
    _assert_same(got, fedavg_explicit(ups, ns))


@pytest.mark.gpu
def test_engine_fedavg_bf16_next_to_other_dtype_groups():
    """bf16 layers and fp32 / fp64 layers in one call: each keeps its own group and result dtype."""
    from substrafl_amd.engine import AggregationEngine

    rng = np.random.default_rng(11)
    pus, ups, ns = _clients(4, [(33,), (5, 7)], 11)
    f32 = [rng.standard_normal((19,)).astype(np.float32) for _ in range(4)]
    f64 = [rng.standard_normal((6,)) for _ in range(4)]
    got = AggregationEngine(device=0).fedavg([[p[0], a, p[1], b] for p, a, b in zip(pus, f32, f64)], ns)
    ref = fedavg_explicit([[u[0], a, u[1]] for u, a in zip(ups, f32)], ns)
    _assert_same([got[0], got[1], got[2]], ref)
    ref64 = fedavg_explicit([[b] for b in f64], ns)[0]
    assert got[3].dtype == np.float64 and np.array_equal(got[3].view(np.uint64), ref64.view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["plain", "bucket"])
def test_strategy_fedavg_bf16(dummy_algo_class, form):
    from substrafl_amd.schemas import FedAvgSharedState
    from substrafl_amd.strategies import FedAvg

    shapes = [s for s in SHAPES if s != ()]  # a 0-d average is a scalar, which the schema rejects
    pus, ups, ns = _clients(3, shapes, 21)
    rows = _as_buckets(pus) if form == "bucket" else pus
    states = [FedAvgSharedState(n_samples=n, parameters_update=p) for n, p in zip(ns, rows)]
    got = FedAvg(algo=dummy_algo_class(), device=0).avg_shared_states(shared_states=states, _skip=True)
    _assert_same(got.avg_parameters_update, fedavg_explicit(ups, ns))
    assert wire.flat_of(list(got.avg_parameters_update)) is not None  # the average is one fp32 bucket


@pytest.mark.gpu
def test_bf16_errors(dummy_algo_class):
    from substrafl_amd.engine import AggregationEngine
    from substrafl_amd.exceptions import EmptySharedStatesError
    from substrafl_amd.multi_device import MultiDeviceEngine
    from substrafl_amd.schemas import FedAvgSharedState
    from substrafl_amd.strategies import FedAvg

    pus, ups, ns = _clients(3, [(4, 3), (10,)], 31)
    eng = AggregationEngine(device=0)
    mixed = [pus[0], ups[1], pus[2]]  # layer 0 (and 1) bf16 for two clients, fp32 for one
    with pytest.raises(NotImplementedError, match="layer 0"):
        eng.fedavg(mixed, ns)
    with pytest.raises(NotImplementedError, match="bf16"):
        eng.scaffold(pus, pus, pus, ns, 1.0)
    with pytest.raises(NotImplementedError, match="bf16"):
        eng.scaffold(ups, ups, pus, ns, 1.0)
    with pytest.raises(NotImplementedError, match="bf16"):
        eng.sequential_sum(pus, ns)
    multi = MultiDeviceEngine((0, 0))
    with pytest.raises(NotImplementedError, match="bf16"):
        multi.fedavg(pus, ns)
    with pytest.raises(NotImplementedError, match="bf16"):
        multi.sequential_sum(pus, ns)
    with pytest.raises(NotImplementedError, match="bf16"):
        multi.scaffold(pus, pus, pus, ns, 1.0)
    # the host checks come first, as for every dtype
    strat = FedAvg(algo=dummy_algo_class(), device=0)
    with pytest.raises(EmptySharedStatesError):
        strat.avg_shared_states(shared_states=[], _skip=True)
    zero = [FedAvgSharedState(n_samples=0, parameters_update=p) for p in pus]
    with pytest.raises(ZeroDivisionError):
        strat.avg_shared_states(shared_states=zero, _skip=True)
    assert eng.fedavg([[], []], [1, 2]) == []
    # and the engine still averages bf16 after the refused calls
    _assert_same(eng.fedavg(pus, ns), fedavg_explicit(ups, ns))
