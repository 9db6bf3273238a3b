"""Every engine route against what the REFERENCE itself computed on the non-fp32 paths
(tests/golden/golden_dtypes.npz and golden_plumbing_half.npz, made by the generators beside them).
No oracle in between: each output is compared with the recorded reference output under
``golden_dtypes_cases.same`` (same dtype, shape and bits; NaN exactly where the reference has NaN).

Routes, each over every case whose kinds it accepts (a documented refusal is asserted, never
skipped): the drop-in strategies; ``AggregationEngine.fedavg`` on rows, tiles, out of core and over
``wire.pack``-ed inputs; ``AggregationEngine.scaffold`` and ``scaffold_per_bucket``; ``wire.BF16``
inputs; ``MultiDeviceEngine`` over three shards of one GPU; the one-call C entry
``NativeMultiFedAvg``; the replay of the reference's fp16 simulations.

The shapes are the fixtures' (nothing is scaled up).  A route loops over the cases, so two
consecutive launches never compute the same values; the sessions' output buffers are filled with
0xFF before every call and every result array is filled with 0xFF once it has been compared (the
host buffers are recycled), so an element that a kernel or a fetch does not write cannot show an
earlier right answer.  (The C entry's sessions are its own: there the device side rests on the
consecutive cases differing.)  A route goes on after a red case and names all of them at its end.
The counts per route, the file's time and the HBM it held are printed when the module ends
(``pytest -s``)."""

import time

import numpy as np
import pytest

import golden_dtypes_cases as G
from substrafl_amd import wire

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]

N_FEDAVG, N_FLOAT, N_SCAFFOLD_OK, N_SCAFFOLD_ERR = 84, 51, 45, 2  # N_FLOAT: FedAvg cases of one float dtype
FLOAT_NAMES = ({"float16"}, {"float32"}, {"float64"})
SIXTEEN_BIT = (["f16", "f16", "f16"], ["f16", "f64", "f64"], ["f16", "f16", "f32"])
SMALL_BUDGET = 64  # bytes: below one row of any case, so sub-ranges are the 512-element minimum
ROUTES, _FREE = {}, []  # cases per route; free HBM after each test
_OUT_SLOTS, _POISON_BYTES = (1, 6), 1 << 18  # the sessions' FedAvg / Scaffold output buffers; > any case's output


class Route:
    """One test's bookkeeping: cases per route (counted here, reported when the module ends) and
    the cases that came out red, all of them."""

    def __init__(self):
        self.n, self.red = {}, []

    def count(self, route):
        self.n[route] = self.n.get(route, 0) + 1

    def same(self, got, ref, what):
        try:
            G.same(got, ref, what)
        except AssertionError as e:
            self.red.append(str(e)[:300])
        for a in got:  # compared: spoil the recycled host buffer behind it
            np.asarray(a).view(np.ndarray).reshape(-1).view(np.uint8).fill(0xFF)

    def done(self, **expected):
        ROUTES.update(self.n)
        assert not self.red, f"{len(self.red)} red:\n" + "\n".join(self.red)
        assert self.n == expected, self.n


def _poison(sessions):
    for s in sessions:
        for slot in _OUT_SLOTS:
            s.memset(s.buffer(slot, _POISON_BYTES), 0xFF, _POISON_BYTES)
        s.sync()


@pytest.fixture(scope="module")
def engine():
    """The engine the strategies use.  Ends with the report."""
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from substrafl_amd import runtime
    from substrafl_amd.engine import engine_for

    t0, (free0, total) = time.perf_counter(), runtime.device_memory(0)
    _FREE.append(free0)
    yield engine_for(None)
    _, meta = G.dtypes_fixture()
    print(f"\ngolden dtypes on the GPU: NumPy {np.__version__} here, {meta['numpy']} made the fixtures; "
          f"{time.perf_counter() - t0:.1f} s; HBM in use at most {(total - min(_FREE)) / 2**20:.0f} MiB "
          f"({(free0 - min(_FREE)) / 2**20:.0f} MiB more than before the file); cases per route:")
    for k, v in ROUTES.items():
        print(f"  {k}: {v}")


@pytest.fixture(scope="module")
def own_engine(engine):
    """An engine of this file's own for the tests that turn its knobs (layout, bucket budget)."""
    from substrafl_amd.engine import AggregationEngine

    return AggregationEngine(device=0)


@pytest.fixture(autouse=True)
def _sample_memory(engine):
    from substrafl_amd import runtime

    yield
    _FREE.append(runtime.device_memory(0)[0])


def _single_float(case) -> bool:
    return set(case["dtypes"]) in FLOAT_NAMES


def test_fixtures_keep_the_nan_cap():
    """Re-asserted from the arrays: finite cases are finite, and no non-finite case or fp16 call is
    mostly NaN (it would compare NaN with NaN and little else)."""
    outs = [(c, out) for c, _, _, out in G.fedavg_cases()]
    outs += [(c, o[0] + o[1]) for c, *_, o in G.scaffold_cases() if o is not None]
    assert len(outs) == N_FEDAVG + N_SCAFFOLD_OK
    n = 0
    for case, out in outs:
        if case["finite"]:
            assert all(np.isfinite(a).all() for a in out), case["key"]
        else:
            assert G.nan_share(out) <= 0.25, (case["key"], G.nan_share(out))
            n += 1
    assert n == 12 + 2 + 6 + 2  # non-finite FedAvg, fp16 overflow, non-finite Scaffold, c holding a NaN
    calls = list(G.half_calls())
    assert len(calls) == 8
    for name, call, ns, pu, extra, out in calls:
        assert G.nan_share(out["avg"] + out.get("c", [])) <= 0.25, call["key"]


# ------------------------------------------------------------------------------------- strategies
def test_strategies_fedavg(engine, dummy_algo_class):
    from substrafl_amd.schemas import FedAvgSharedState
    from substrafl_amd.strategies import FedAvg

    r = Route()
    fa = FedAvg(algo=dummy_algo_class())
    for case, ns, clients, out in G.fedavg_cases():
        _poison([engine.session()])
        res = fa.avg_shared_states([FedAvgSharedState(n_samples=n, parameters_update=c) for n, c in zip(ns, clients)],
                                   _skip=True)
        r.same(res.avg_parameters_update, out, case["key"])
        r.count("strategies.FedAvg")
    r.done(**{"strategies.FedAvg": N_FEDAVG})


def _strategy_scaffold(algo_class, ns, pu, cv, cs, lr):
    from substrafl_amd.schemas import ScaffoldSharedState
    from substrafl_amd.strategies import Scaffold

    states = [ScaffoldSharedState(parameters_update=pu[k], control_variate_update=cv[k], n_samples=ns[k],
                                  server_control_variate=cs[k]) for k in range(len(ns))]
    return Scaffold(algo=algo_class(), aggregation_lr=lr).avg_shared_states(states, _skip=True)


def test_strategies_scaffold(engine, dummy_algo_class):
    _, meta = G.dtypes_fixture()
    r, errors = Route(), {}
    for case, ns, pu, cv, cs, lr, out in G.scaffold_cases():
        _poison([engine.session()])
        if out is None:
            with pytest.raises(AssertionError, match="all server_control_variate in the shared_states are not equal") as e:
                _strategy_scaffold(dummy_algo_class, ns, pu, cv, cs, lr)
            errors[case["key"]] = e.type.__name__
            r.count("strategies.Scaffold (refused as the reference refuses)")
            continue
        res = _strategy_scaffold(dummy_algo_class, ns, pu, cv, cs, lr)
        if case["triple"] in SIXTEEN_BIT:  # kinds per bucket: the 2-byte rows went to the GPU as they are
            assert list(engine.last_timing["bucket_kinds"]) == case["triple"], case["key"]
        r.same(res.avg_parameters_update, out[0], (case["key"], "avg"))
        r.same(res.server_control_variate, out[1], (case["key"], "new c"))
        r.count("strategies.Scaffold")
    assert errors == meta["errors"]
    r.done(**{"strategies.Scaffold": N_SCAFFOLD_OK,
              "strategies.Scaffold (refused as the reference refuses)": N_SCAFFOLD_ERR})


# ------------------------------------------------------------------------------------- AggregationEngine.fedavg
@pytest.mark.parametrize("route", ["rows", "tiles", "out-of-core", "packed"])
def test_engine_fedavg(own_engine, route):
    engine = own_engine
    tiled, budget = engine.tiled, engine.max_bucket_bytes
    r, n_ooc = Route(), 0
    try:
        engine.tiled = route == "tiles"
        if route == "out-of-core":
            engine.max_bucket_bytes = SMALL_BUDGET
        for case, ns, clients, out in G.fedavg_cases():
            ns = [int(n) for n in ns]
            rows = [wire.pack(c) for c in clients] if route == "packed" else clients
            sessions = [engine.session()] + (engine._ooc.sessions() if engine._ooc is not None else [])
            _poison(sessions)
            r.same(engine.fedavg(rows, ns), out, (case["key"], route))
            staging = engine.last_timing["staging"]
            if route == "out-of-core":  # a call over one float dtype streams in ranges; others are cast in core
                assert (staging == "out-of-core") == _single_float(case), (case["key"], staging)
                if case["kind"] == "edge":
                    assert sum(len(x) for x in engine.last_timing["out_of_core"]["ranges"]) > 1
                n_ooc += staging == "out-of-core"
            elif route != "packed" and _single_float(case):
                want = "host-tiles" if route == "tiles" and case["dtypes"] == ["float32"] else "host-rows"
                assert staging == want, (case["key"], staging)
            r.count(f"AggregationEngine.fedavg {route}")
    finally:
        engine.tiled, engine.max_bucket_bytes = tiled, budget
    r.done(**{f"AggregationEngine.fedavg {route}": N_FEDAVG})
    if route == "out-of-core":
        assert n_ooc == sum(_single_float(c) for c, *_ in G.fedavg_cases()) == N_FLOAT


# ------------------------------------------------------------------------------------- AggregationEngine.scaffold
def test_engine_scaffold_and_per_bucket(engine):
    r = Route()
    for case, ns, pu, cv, cs, lr, out in G.scaffold_cases():
        _poison([engine.session()])
        mism, new_c, avg = engine.scaffold(pu, cv, cs, ns, lr)
        first = ([a.copy() for a in avg], [a.copy() for a in new_c])
        if out is None:
            assert mism > 0, case["key"]
            r.count("AggregationEngine.scaffold (mismatch counted)")
        else:
            assert mism == 0, case["key"]
            r.same(avg, out[0], (case["key"], "scaffold", "avg"))
            r.same(new_c, out[1], (case["key"], "scaffold", "new c"))
            r.count("AggregationEngine.scaffold")
        if case["triple"] not in SIXTEEN_BIT:
            continue
        _poison([engine.session()])
        mism2, new_c2, avg2 = engine.scaffold_per_bucket(pu, cv, cs, ns, lr)
        assert list(engine.last_timing["bucket_kinds"]) == case["triple"]
        assert (mism2 > 0) == (out is None), case["key"]
        if out is not None:
            G.same(avg2, first[0], (case["key"], "per bucket against scaffold"))
            G.same(new_c2, first[1], (case["key"], "per bucket against scaffold"))
            r.same(avg2, out[0], (case["key"], "per bucket", "avg"))
            r.same(new_c2, out[1], (case["key"], "per bucket", "new c"))
            r.count("AggregationEngine.scaffold_per_bucket")
    # per bucket: the three 16-bit tables, the (f16, f64, f64) edge, fp16 non-finite, fp16 c equal by value
    r.done(**{"AggregationEngine.scaffold": N_SCAFFOLD_OK, "AggregationEngine.scaffold (mismatch counted)": N_SCAFFOLD_ERR,
              "AggregationEngine.scaffold_per_bucket": 3 * 7 + 1 + 2 + 1})


# ------------------------------------------------------------------------------------- bf16
def test_bf16_inputs(own_engine):
    """The bf16-representable float32 cases as ``wire.BF16`` rows (the conversion is exact for them):
    the float32 average is the reference's on the upcasts.  Routes without a bf16 path refuse."""
    from substrafl_amd.multi_device import MultiDeviceEngine, NativeMultiFedAvg

    engine = own_engine
    tiled, budget = engine.tiled, engine.max_bucket_bytes
    r = Route()
    try:
        for case, ns, clients, out in G.fedavg_cases(kinds=("bf16",)):
            rows = [[wire.float32_to_bf16(a) for a in c] for c in clients]
            for row, c in zip(rows, clients):
                for b, a in zip(row, c):
                    assert b.dtype == wire.BF16 and np.array_equal(G.bits(wire.bf16_to_float32(b)), G.bits(a))
            for route in ("rows", "tiles", "packed"):
                engine.tiled = route == "tiles"
                _poison([engine.session()])
                r.same(engine.fedavg([wire.pack(x) for x in rows] if route == "packed" else rows, ns), out,
                       (case["key"], "bf16", route))
                r.count(f"AggregationEngine.fedavg wire.BF16 {route}")
            engine.max_bucket_bytes = SMALL_BUDGET
            with pytest.raises(NotImplementedError):
                engine.fedavg(rows, ns)
            engine.max_bucket_bytes = budget
            with pytest.raises(NotImplementedError):
                engine.scaffold(rows, rows, [rows[0]] * len(rows), ns, 0.7)
            with pytest.raises(NotImplementedError):
                MultiDeviceEngine([0, 0, 0], max_shard_bytes=SMALL_BUDGET).fedavg(rows, ns)
            nat = NativeMultiFedAvg([0, 0, 0], max_shard_bytes=SMALL_BUDGET)
            try:
                with pytest.raises(NotImplementedError):
                    nat.fedavg(rows, ns)
            finally:
                nat.close()
            r.count("wire.BF16 refused (out of core, scaffold, multi-device, native multi)")
    finally:
        engine.tiled, engine.max_bucket_bytes = tiled, budget
    r.done(**{"AggregationEngine.fedavg wire.BF16 rows": 2, "AggregationEngine.fedavg wire.BF16 tiles": 2,
              "AggregationEngine.fedavg wire.BF16 packed": 2,
              "wire.BF16 refused (out of core, scaffold, multi-device, native multi)": 2})


# ------------------------------------------------------------------------------------- multi-device
def _shards_busy(ranges) -> bool:
    """At least two shards have work and one runs more than one sub-range."""
    return sum(1 for x in ranges if x) >= 2 and max(len(x) for x in ranges) > 1


def test_multi_device_fedavg(engine):
    from substrafl_amd.multi_device import MultiDeviceEngine

    md = MultiDeviceEngine([0, 0, 0], max_shard_bytes=SMALL_BUDGET)
    r, busy = Route(), 0
    for case, ns, clients, out in G.fedavg_cases():
        ns = [int(n) for n in ns]
        _poison(md.sessions())
        md.last_timing = {}
        r.same(md.fedavg(clients, ns), out, (case["key"], "multi-device"))
        sharded = "ranges" in md.last_timing  # one float dtype: sharded; else the first device casts
        assert sharded == _single_float(case), case["key"]
        if case["kind"] == "edge":
            assert _shards_busy(md.last_timing["ranges"]), md.last_timing["ranges"]
            busy += 1
        r.count("MultiDeviceEngine.fedavg" + ("" if sharded else " (first device: casts / dtype groups)"))
    assert busy == 4
    r.done(**{"MultiDeviceEngine.fedavg": N_FLOAT,
              "MultiDeviceEngine.fedavg (first device: casts / dtype groups)": N_FEDAVG - N_FLOAT})


def test_multi_device_scaffold(engine):
    from substrafl_amd.multi_device import MultiDeviceEngine

    md = MultiDeviceEngine([0, 0, 0], max_shard_bytes=SMALL_BUDGET)
    r, busy = Route(), 0
    for case, ns, pu, cv, cs, lr, out in G.scaffold_cases():
        _poison(md.sessions())
        md.last_timing = {}
        mism, new_c, avg = md.scaffold(pu, cv, cs, ns, lr)
        sharded = "ranges" in md.last_timing
        assert sharded == (case["triple"] in (["f32"] * 3, ["f64"] * 3)), case["key"]
        if out is None:
            assert mism > 0, case["key"]
            continue
        assert mism == 0, case["key"]
        r.same(avg, out[0], (case["key"], "multi-device", "avg"))
        r.same(new_c, out[1], (case["key"], "multi-device", "new c"))
        if case["kind"] == "edge" and sharded:  # the fp64 edge: shards with lo > 0, several sub-ranges
            assert _shards_busy(md.last_timing["ranges"]), md.last_timing["ranges"]
            busy += 1
        r.count("MultiDeviceEngine.scaffold" + ("" if sharded else " (first device: 16-bit kinds)"))
    assert busy == 1
    # sharded: the f32 and f64 tables, the fp64 edge, f32 / f64 non-finite, fp64 c equal by value
    r.done(**{"MultiDeviceEngine.scaffold": 2 * 7 + 1 + 4 + 1,
              "MultiDeviceEngine.scaffold (first device: 16-bit kinds)": N_SCAFFOLD_OK - (2 * 7 + 1 + 4 + 1)})


def test_native_multi_fedavg(engine):
    from substrafl_amd.multi_device import NativeMultiFedAvg

    nat = NativeMultiFedAvg([0, 0, 0], max_shard_bytes=SMALL_BUDGET)
    r, busy = Route(), 0
    try:
        for case, ns, clients, out in G.fedavg_cases():
            ns = [int(n) for n in ns]
            if not _single_float(case):  # integers, bool, mixed dtypes: the C entry takes one float dtype
                with pytest.raises(NotImplementedError):
                    nat.fedavg(clients, ns)
                r.count("NativeMultiFedAvg (refused: not one float dtype)")
                continue
            r.same(nat.fedavg(clients, ns), out, (case["key"], "native multi"))
            if case["kind"] == "edge":
                info = nat.shard_info()
                assert sum(1 for i in info if i["hi"] > i["lo"]) >= 2 and max(i["ranges"] for i in info) > 1, info
                busy += 1
            r.count("NativeMultiFedAvg")
    finally:
        nat.close()
    assert busy == 4
    r.done(**{"NativeMultiFedAvg": N_FLOAT, "NativeMultiFedAvg (refused: not one float dtype)": N_FEDAVG - N_FLOAT})


# ------------------------------------------------------------------------------------- the fp16 simulations
def test_replays_every_fp16_aggregation(engine, dummy_algo_class):
    from substrafl_amd.schemas import FedAvgSharedState
    from substrafl_amd.strategies import FedAvg

    r, kinds = Route(), []
    for name, call, ns, pu, extra, out in G.half_calls():
        _poison([engine.session()])
        if call["kind"] == "fedavg":
            res = FedAvg(algo=dummy_algo_class()).avg_shared_states(
                [FedAvgSharedState(n_samples=n, parameters_update=p) for n, p in zip(ns, pu)], _skip=True)
            r.same(res.avg_parameters_update, out["avg"], call["key"])
        else:
            res = _strategy_scaffold(dummy_algo_class, ns, pu, extra["cv"], extra["c"], call["aggregation_lr"])
            kinds.append(tuple(engine.last_timing["bucket_kinds"]))
            r.same(res.avg_parameters_update, out["avg"], call["key"])
            r.same(res.server_control_variate, out["c"], call["key"])
        r.count("fp16 simulations replayed through the strategies")
    # round 1 ships fp16 control variates, later rounds the float64 the aggregation returned
    assert kinds == [("f16", "f16", "f16"), ("f16", "f64", "f64"), ("f16", "f64", "f64")]
    r.done(**{"fp16 simulations replayed through the strategies": 8})
