"""Scaffold over fp16 and bf16 buckets through ``Scaffold(...).avg_shared_states``: kinds per
bucket, 2-byte rows staged raw, bit for bit against the reference's own NumPy calls.

Reference: ``oracle.scaffold_reference_structure`` on the inputs (fp16: NumPy multiplies them by
float64 weights itself) or on their exact ``wire.bf16_to_float32`` upcasts (bf16, which NumPy
lacks).  ``last_timing["bucket_kinds"]`` names what was staged.

0-d layers: ``np.sum`` of 0-d arrays is a NumPy scalar, which ``ScaffoldAveragedStates`` (a list of
arrays) refuses in the reference as here, so they are checked one level down, at
``AggregationEngine.scaffold_per_bucket``, which returns the scalars the reference's sums give."""

import numpy as np
import pytest

from oracle import scaffold_reference_structure
from substrafl_amd import wire

pytestmark = pytest.mark.gpu

SHAPES = [(33, 9), (1,), (1, 1), (2049,), (1,), (7,)]
NP = {"f16": np.float16, "f32": np.float32, "f64": np.float64}


@pytest.fixture(scope="module")
def engine():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from substrafl_amd.engine import engine_for

    return engine_for(None)


def layer(kind: str, shape, rng) -> np.ndarray:
    x = np.asarray(rng.standard_normal(shape) * 3, np.float32)
    return wire.float32_to_bf16(x) if kind == "bf16" else x.astype(NP[kind])


def upcast(a):
    return wire.bf16_to_float32(a) if wire.is_bf16(a) else np.asarray(a)


def same(got, ref):
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert g.dtype == np.float64 == r.dtype and g.shape == r.shape
        assert np.array_equal(np.asarray(g).view(np.uint64), np.asarray(r).view(np.uint64))


def clients(dts, K, seed, packed=False):
    rng = np.random.default_rng(seed)
    d_k, cv_k, c_k = dts
    mk = (lambda arrs: wire.pack(arrs)) if packed else (lambda arrs: arrs)
    pus = [mk([layer(d_k, s, rng) for s in SHAPES]) for _ in range(K)]
    cvs = [mk([layer(cv_k, s, rng) for s in SHAPES]) for _ in range(K)]
    c = mk([layer(c_k, s, rng) for s in SHAPES])
    ns = [int(v) for v in rng.integers(1, 5000, K)]
    return pus, cvs, c, ns


def run(algo_class, pus, cvs, cs, ns, lr=0.7):
    from substrafl_amd.schemas import ScaffoldSharedState
    from substrafl_amd.strategies import Scaffold

    states = [ScaffoldSharedState(parameters_update=pus[k], control_variate_update=cvs[k], n_samples=ns[k],
                                  server_control_variate=cs[k]) for k in range(len(ns))]
    return Scaffold(algo=algo_class(), aggregation_lr=lr).avg_shared_states(shared_states=states, _skip=True)


def reference(pus, cvs, c, ns, lr=0.7):
    up = lambda rows: [[upcast(a) for a in row] for row in rows]  # noqa: E731
    return scaffold_reference_structure(up(pus), up(cvs), [upcast(a) for a in c], ns, lr)


TRIPLES = [("f16", "f16", "f16"), ("bf16", "bf16", "bf16"), ("f16", "f64", "f64"), ("bf16", "f64", "f64"),
           ("bf16", "bf16", "f64"), ("f16", "f32", "f32"), ("f32", "f16", "f16")]


@pytest.mark.parametrize("K", [3, 17, 70])
@pytest.mark.parametrize("dts", TRIPLES, ids="-".join)
def test_bucket_kinds(engine, dummy_algo_class, dts, K):
    pus, cvs, c, ns = clients(dts, K, seed=K * 7 + TRIPLES.index(dts))
    res = run(dummy_algo_class, pus, cvs, [c] * K, ns)
    assert engine.last_timing["bucket_kinds"] == dts
    ref_c, ref_avg = reference(pus, cvs, c, ns)
    same(res.server_control_variate, ref_c)
    same(res.avg_parameters_update, ref_avg)


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_zero_d_layers_at_the_engine(engine, kind):
    rng = np.random.default_rng(2)
    K, shapes = 9, [(), (5,), (), (1,)]
    pus = [[layer(kind, s, rng) for s in shapes] for _ in range(K)]
    cvs = [[layer(kind, s, rng) for s in shapes] for _ in range(K)]
    c = [layer(kind, s, rng) for s in shapes]
    ns = [int(v) for v in rng.integers(1, 5000, K)]
    mism, new_c, avg = engine.scaffold_per_bucket(pus, cvs, [c] * K, ns, 0.7)
    assert mism == 0 and engine.last_timing["bucket_kinds"] == (kind, kind, kind)
    ref_c, ref_avg = reference(pus, cvs, c, ns)
    same(new_c, ref_c)
    same(avg, ref_avg)


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_flat_wire_buckets_as_inputs(engine, dummy_algo_class, kind):
    pus, cvs, c, ns = clients((kind, kind, kind), 5, seed=3, packed=True)
    assert wire.flat_of(pus[0]) is not None
    res = run(dummy_algo_class, pus, cvs, [c] * 5, ns)
    assert engine.last_timing["bucket_kinds"] == (kind, kind, kind)
    ref_c, ref_avg = reference(pus, cvs, c, ns)
    same(res.server_control_variate, ref_c)
    same(res.avg_parameters_update, ref_avg)


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_c_check_on_16_bit_c(engine, dummy_algo_class, kind):
    K = 4
    pus, cvs, c, ns = clients((kind, kind, kind), K, seed=11)
    ref_c, _ = reference(pus, cvs, c, ns)
    bits = lambda a: a.view(np.uint16)  # noqa: E731
    nan = 0x7E00 if kind == "f16" else 0x7FC0

    same(run(dummy_algo_class, pus, cvs, [c] * K, ns).server_control_variate, ref_c)
    assert engine.last_timing["c_check"] == "identity"

    copies = [c] + [[a.copy() for a in c] for _ in range(K - 1)]
    same(run(dummy_algo_class, pus, cvs, copies, ns).server_control_variate, ref_c)
    assert engine.last_timing["c_check"] == "host-bytes"

    # copies that differ only in the sign of a zero, or hold the same NaN in one place, are equal
    c0 = [a.copy() for a in c]
    bits(c0[0])[0, 0] = 0x0000
    bits(c0[3])[5] = nan
    other = [a.copy() for a in c0]
    bits(other[0])[0, 0] = 0x8000
    bits(other[3])[5] = nan | 1  # another payload: still NaN == NaN
    run(dummy_algo_class, pus, cvs, [c0, other, c0, other], ns)
    assert engine.last_timing["c_check"] == "host-values"

    # one differing element: the reference's message
    wrong = [a.copy() for a in c]
    bits(wrong[3])[7] ^= 0x0100
    with pytest.raises(AssertionError, match="all server_control_variate in the shared_states are not equal"):
        run(dummy_algo_class, pus, cvs, [c, c, wrong, c], ns)


def test_bf16_mixed_into_a_bucket_is_refused(engine, dummy_algo_class):
    pus, cvs, c, ns = clients(("bf16", "bf16", "bf16"), 3, seed=5)
    pus[1][0] = upcast(pus[1][0])  # one fp32 layer among bf16 ones
    with pytest.raises(NotImplementedError):
        run(dummy_algo_class, pus, cvs, [c] * 3, ns)


def test_ingest_prestages_two_byte_rows(engine, dummy_algo_class, tmp_path):
    """K fp16 Scaffold states loaded by ``ingest``: the 2-byte rows are staged once, while loading,
    and the aggregation call finds them; the result is that of a call without ingest."""
    from substrafl_amd.remote import PickleSerializer
    from substrafl_amd.schemas import ScaffoldSharedState
    from substrafl_amd.strategies import Scaffold

    K = 5
    pus, cvs, c, ns = clients(("f16", "f16", "f16"), K, seed=8)
    paths = []
    for k in range(K):
        paths.append(tmp_path / f"s{k}")
        PickleSerializer.save(ScaffoldSharedState(parameters_update=pus[k], control_variate_update=cvs[k],
                                                  n_samples=ns[k], server_control_variate=c), paths[-1])
    sc = Scaffold(algo=dummy_algo_class(), aggregation_lr=0.7)
    states = sc.ingest_shared_states("avg_shared_states", paths, PickleSerializer.load)
    assert engine.last_ingest["prestaged_clients"] == K
    res = sc.avg_shared_states(states, _skip=True)
    assert engine.last_timing.get("prestaged") is True
    assert engine.last_timing["bucket_kinds"] == ("f16", "f16", "f16")
    ref_c, ref_avg = reference(pus, cvs, c, ns)
    same(res.server_control_variate, ref_c)
    same(res.avg_parameters_update, ref_avg)
    res2 = sc.avg_shared_states(states, _skip=True)  # staged by the call itself
    assert not engine.last_timing.get("prestaged")
    same(res2.avg_parameters_update, ref_avg)
