"""The opt-in device orthonormalisation of FedPCA's averaged state (fed_pca.py:289-299) through both
strategy classes -- ``strategies.FedPCA(qr="device")`` and ``accelerate(ss.FedPCA, qr="device")`` --
and :meth:`engine.AggregationEngine.orthonormal_rows` behind them.

The host route (``np.linalg.qr(a.T)[0].T``, LAPACK in fp64 whatever the state's dtype) is the
reference.  With u = 2^-53, eps and o as in tests/test_dense_lq_gpu.py and the caps that module
holds the kernels to, eps_cap = max(4 eps_ref, 8 u sqrt(n)) and o_cap likewise, the distance bound is
D = 2 (sqrt(2) kappa_2 (eps_cap + eps_ref) + o_dev + o_ref).  The engine does not return L, so the
device's own eps is not available here and its cap stands in; o_dev is measured on the returned Q
where that is the fp64 Q (fp64 states), and is o_cap where only its fp32 rounding comes back:
  * fp64 states: ||Q_dev - Q_host||_F <= D, and o_dev itself within both gates of the kernel tests;
  * fp32 states: elementwise |Q_dev - Q_host| <= D + 2^-23 |Q_host| with D of the widened matrix
    (both routes round an fp64 Q to fp32), same dtype and shape; the number of elements that are
    not bit-identical is printed and has no threshold;
  * layers the engine declines (n > m, 1-D, byte-swapped, integer) take the host line, the reason
    is in ``last_timing["qr"]`` and the result is the host route's, bit for bit -- an error
    included: a 1-D layer raises NumPy's LinAlgError on either route.  An integer layer of the
    clients is a float64 layer of the average (the engine averages integers in fp64), so through the
    strategy classes it goes to the device; the integer array itself is declined by the engine.
"""

import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import standin_substrafl.strategies as ss
from standin_substrafl.strategies import schemas as sch
from test_dense_lq_gpu import U, _reference

gpu = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
D = ROOT / "tests" / "golden"
NS = [17, 5, 230]
WIDE_SHAPES = [(1, 7), (4, 30), (33, 130), (65, 600)]


class _Algo:
    pass


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _layers(shapes, dtype, seed):
    rng = np.random.default_rng([seed, len(shapes)])
    return [[rng.standard_normal(s).astype(dtype) for s in shapes] for _ in NS]


def _make(kind, qr=None, dummy_algo_class=None):
    """``(strategy, state class)`` of one of the two strategy classes; ``qr`` None: the default."""
    kw = {} if qr is None else {"qr": qr}
    if kind == "mirror":
        from substrafl_amd.schemas import FedPCASharedState
        from substrafl_amd.strategies import FedPCA

        return FedPCA(algo=dummy_algo_class(), **kw), FedPCASharedState
    from substrafl_amd.integration import accelerate

    return accelerate(ss.FedPCA, **kw)(algo=_Algo()), sch.FedPCASharedState


def _run(strategy, state_cls, layers, method="avg_shared_states_with_qr"):
    states = [state_cls(n_samples=n, parameters_update=list(p)) for n, p in zip(NS, layers)]
    return [np.asarray(a) for a in getattr(strategy, method)(shared_states=states, _skip=True).avg_parameters_update]


def _timing():
    from substrafl_amd.engine import engine_for

    return engine_for(None).last_timing


def _distance_bound(A64, Q_dev=None):
    """``(D, kappa_2)`` of the module docstring; ``Q_dev``: the device's fp64 Q, whose measured loss
    of orthogonality then takes o_cap's place (and is held to both gates itself)."""
    n, m = A64.shape
    ref = _reference(A64)
    cap = lambda v: max(4.0 * v, 8.0 * U * np.sqrt(n))  # noqa: E731
    o_dev = cap(ref["o"])
    if Q_dev is not None:
        o_dev = float(np.linalg.norm(Q_dev @ Q_dev.T - np.eye(n)))
        assert o_dev <= cap(ref["o"]) and o_dev <= m * n * U * np.sqrt(n), (A64.shape, o_dev, ref["o"])
    return 2.0 * (np.sqrt(2.0) * ref["kappa"] * (cap(ref["eps"]) + ref["eps"]) + o_dev + ref["o"]), ref["kappa"]


KINDS = ["mirror", "accelerate"]


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_fp64_states_within_the_closeness_bound(kind, dummy_algo_class):
    layers = _layers(WIDE_SHAPES, np.float64, 1)
    dev_s, cls = _make(kind, "device", dummy_algo_class)
    host_s, _ = _make(kind, "host", dummy_algo_class)
    avg = _run(host_s, cls, layers, "avg_shared_states")
    host = _run(host_s, cls, layers)
    got = _run(dev_s, cls, layers)
    tm = _timing()
    assert tm["qr"] == "device" and tm["qr_layers"] == ["device"] * len(WIDE_SHAPES), tm
    assert (tm["n"], tm["m"]) == WIDE_SHAPES[-1]
    assert {"stage_s", "factor_ms", "fetch_s", "total_s"} <= set(tm)
    for a, h, g in zip(avg, host, got):
        assert np.array_equal(_bits(h), _bits(np.linalg.qr(a.T)[0].T))  # the host route is today's line
        assert g.dtype == h.dtype == np.float64 and g.shape == h.shape and g.flags.c_contiguous
        bound, kappa = _distance_bound(a, g)
        assert kappa <= 1e3, kappa
        dist = float(np.linalg.norm(g - h))
        print(f"{kind} {a.shape} f64: kappa {kappa:.3g}  |Q_dev - Q_host|_F {dist:.3e}  bound {bound:.3e}")
        assert dist <= bound, (a.shape, dist, bound)


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_fp32_states_elementwise(kind, dummy_algo_class):
    layers = _layers(WIDE_SHAPES, np.float32, 2)
    dev_s, cls = _make(kind, "device", dummy_algo_class)
    host_s, _ = _make(kind, "host", dummy_algo_class)
    avg = _run(host_s, cls, layers, "avg_shared_states")
    host = _run(host_s, cls, layers)
    got = _run(dev_s, cls, layers)
    assert _timing()["qr_layers"] == ["device"] * len(WIDE_SHAPES)
    for a, h, g in zip(avg, host, got):
        assert a.dtype == np.float32
        assert g.dtype == h.dtype == np.float32 and g.shape == h.shape == a.shape and g.flags.c_contiguous
        bound, kappa = _distance_bound(a.astype(np.float64))
        h64, g64 = h.astype(np.float64), g.astype(np.float64)
        differ = int(np.count_nonzero(_bits(g) != _bits(h)))
        print(f"{kind} {a.shape} f32: kappa {kappa:.3g}  max |Q_dev - Q_host| {np.abs(g64 - h64).max():.3e}  "
              f"D {bound:.3e}  not bit-identical: {differ} of {g.size}")
        assert np.all(np.abs(g64 - h64) <= bound + 2.0 ** -23 * np.abs(h64)), a.shape


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_golden_fedpca_layers(kind, dummy_algo_class):
    """The reference's own FedPCA vectors (float32, 4 x 30 and 3 x 17): the default route gives the
    reference's bits; both layers meet the engine's conditions, so the device route takes them and
    is held to the fp32 bound against the reference's output."""
    import json

    arrays = np.load(D / "golden_aggregation.npz", allow_pickle=False)
    cases = [c for c in json.loads((D / "golden_meta.json").read_text())["cases"] if c["strategy"] == "fedpca"]
    assert cases
    for case in cases:
        key, K, L = case["key"], case["K"], case["layers"]
        ns = [int(v) for v in arrays[f"{key}/n_samples"]]
        want = [arrays[f"{key}/qr{li}"] for li in range(L)]
        for qr in (None, "device"):
            s, cls = _make(kind, qr, dummy_algo_class)
            states = [cls(n_samples=ns[k], parameters_update=[arrays[f"{key}/x{li}"][k] for li in range(L)])
                      for k in range(K)]
            got = [np.asarray(a) for a in s.avg_shared_states_with_qr(shared_states=states, _skip=True).avg_parameters_update]
            avg = [np.asarray(a) for a in s.avg_shared_states(shared_states=states, _skip=True).avg_parameters_update]
            for a, g, w in zip(avg, got, want):
                assert g.dtype == w.dtype and g.shape == w.shape
                if qr is None:
                    assert np.array_equal(_bits(g), _bits(w))
                    continue
                bound, _ = _distance_bound(a.astype(np.float64))
                g64, w64 = g.astype(np.float64), w.astype(np.float64)
                print(f"{kind} {key} {a.shape}: not bit-identical to the reference: "
                      f"{int(np.count_nonzero(_bits(g) != _bits(w)))} of {g.size}")
                assert np.all(np.abs(g64 - w64) <= bound + 2.0 ** -23 * np.abs(w64))


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_declined_layers_take_the_host_route(kind, dummy_algo_class):
    """Tall layers (n > m) through the strategies: the engine declines, says why, and the result is
    the host route's, bit for bit; a wide layer in the same state still goes to the device."""
    for dtype in (np.float32, np.float64):
        layers = _layers([(30, 4), (17, 16), (4, 30)], dtype, 3)
        dev_s, cls = _make(kind, "device", dummy_algo_class)
        host_s, _ = _make(kind, "host", dummy_algo_class)
        host = _run(host_s, cls, layers)
        got = _run(dev_s, cls, layers)
        routes = _timing()["qr_layers"]
        assert routes[2] == "device" and all(r.startswith("host: ") and "n > m" in r for r in routes[:2]), routes
        for h, g in zip(host[:2], got[:2]):
            assert g.dtype == h.dtype and np.array_equal(_bits(g), _bits(h))
        tall_only = [[p[0]] for p in layers]
        got = _run(dev_s, cls, tall_only)
        assert _timing()["qr"].startswith("host: ") and np.array_equal(_bits(got[0]), _bits(host[0]))


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_one_dimensional_and_integer_layers_through_the_strategies(kind, dummy_algo_class):
    """A 1-D layer: the engine declines it and the host line raises NumPy's error, as on the host
    route.  Integer layers: their average is float64 (the reference multiplies by a float), so the
    averaged layer meets the engine's conditions and is held to the fp64 bound."""
    dev_s, cls = _make(kind, "device", dummy_algo_class)
    host_s, _ = _make(kind, "host", dummy_algo_class)
    flat = _layers([(7,)], np.float64, 7)
    for s in (host_s, dev_s):
        with pytest.raises(np.linalg.LinAlgError):
            _run(s, cls, flat)
    assert _timing()["qr"].startswith("host: ") and "2-D" in _timing()["qr"], _timing()
    rng = np.random.default_rng(8)
    ints = [[rng.integers(-9, 10, (3, 8))] for _ in NS]
    (avg,) = _run(host_s, cls, ints, "avg_shared_states")
    (host,), (got,) = _run(host_s, cls, ints), _run(dev_s, cls, ints)
    assert avg.dtype == host.dtype == got.dtype == np.float64 and _timing()["qr_layers"] == ["device"]
    assert np.array_equal(_bits(host), _bits(np.linalg.qr(avg.T)[0].T))
    bound, _ = _distance_bound(avg, got)
    assert float(np.linalg.norm(got - host)) <= bound


@gpu
def test_engine_declines_and_the_host_line_decides():
    """A 1-D layer, an integer layer, a byte-swapped one and a list: declined with the reason, and
    ``orthonormal_layers`` then gives exactly what the host line gives -- its error included."""
    from substrafl_amd.engine import engine_for
    from substrafl_amd.strategies.fed_pca import orthonormal_layers

    eng = engine_for(None)
    rng = np.random.default_rng(4)
    wide = rng.standard_normal((3, 8))
    cases = {"2-D": rng.standard_normal(7), "dtype": rng.integers(-4, 5, (3, 8)), "byte order": wide.astype(">f8"),
             "ndarray": wide.tolist(), "empty": np.zeros((0, 4)), "n > m": wide.T.copy(), "float16": wide.astype(np.float16)}
    for word, a in cases.items():
        q, reason = eng.orthonormal_rows(a)
        assert q is None and reason.startswith("host: ") and word in reason, (word, reason)
    for word in ("dtype", "byte order", "n > m"):
        a = cases[word]
        (got,) = orthonormal_layers([a], None, "device")
        want = np.linalg.qr(a.T)[0].T
        assert got.dtype == want.dtype and np.array_equal(got, want) and eng.last_timing["qr"].startswith("host: ")
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.qr(cases["2-D"].T)
    with pytest.raises(np.linalg.LinAlgError):
        orthonormal_layers([cases["2-D"]], None, "device")
    before = wide.copy()
    q, reason = eng.orthonormal_rows(wide)
    assert reason == "device" and q.shape == (3, 8) and eng.last_timing["qr"] == "device"
    assert np.array_equal(_bits(wide), _bits(before))  # the host array is only read


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_environment_overrides_both_ways(kind, dummy_algo_class, monkeypatch):
    layers = _layers([(4, 30)], np.float64, 5)
    host_s, cls = _make(kind, None, dummy_algo_class)
    dev_s, _ = _make(kind, "device", dummy_algo_class)
    monkeypatch.delenv("FEDAGG_PCA_QR", raising=False)
    host = _run(host_s, cls, layers)
    assert "qr" not in _timing()  # the default route does not go near the LQ
    dev = _run(dev_s, cls, layers)
    assert _timing()["qr"] == "device"
    monkeypatch.setenv("FEDAGG_PCA_QR", "device")
    got = _run(host_s, cls, layers)
    assert _timing()["qr"] == "device" and np.array_equal(_bits(got[0]), _bits(dev[0]))
    monkeypatch.setenv("FEDAGG_PCA_QR", "host")
    got = _run(dev_s, cls, layers)
    assert "qr" not in _timing() and np.array_equal(_bits(got[0]), _bits(host[0]))
    monkeypatch.setenv("FEDAGG_PCA_QR", "gpu")
    with pytest.raises(ValueError, match="qr"):
        _run(dev_s, cls, layers)


@gpu
def test_default_route_is_the_host_line_and_never_loads_the_dense_library():
    """A fresh process on the GPU: both classes with the default ``qr`` give ``np.linalg.qr(a.T)[0].T``
    of the average, and the dense library is never imported or mapped."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import numpy as np\n"
            "import standin_substrafl.strategies as ss\n"
            "from standin_substrafl.strategies import schemas as sch\n"
            "from conftest import DummyAlgo\n"
            "from substrafl_amd.integration import accelerate\n"
            "from substrafl_amd.schemas import FedPCASharedState\n"
            "from substrafl_amd.strategies import FedPCA\n"
            "rng = np.random.default_rng(6)\n"
            "layers = [[rng.standard_normal(s).astype(dt) for s, dt in (((4, 30), 'f4'), ((33, 70), 'f8'))] for _ in range(3)]\n"
            "class A: pass\n"
            "for s, cls in ((FedPCA(algo=DummyAlgo()), FedPCASharedState), (accelerate(ss.FedPCA)(algo=A()), sch.FedPCASharedState)):\n"
            "    st = [cls(n_samples=n, parameters_update=list(p)) for n, p in zip((3, 9, 4), layers)]\n"
            "    avg = s.avg_shared_states(shared_states=st, _skip=True).avg_parameters_update\n"
            "    got = s.avg_shared_states_with_qr(shared_states=st, _skip=True).avg_parameters_update\n"
            "    for a, g in zip(avg, got):\n"
            "        w = np.linalg.qr(np.asarray(a).T)[0].T\n"
            "        assert g.dtype == w.dtype and np.array_equal(g, w) and g.tobytes() == w.tobytes()\n"
            "assert 'substrafl_amd._native_dense' not in sys.modules\n"
            "assert 'libfedagg_dense' not in open('/proc/self/maps').read()\n" % (str(ROOT), str(ROOT / "tests")))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300)
