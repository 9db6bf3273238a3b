"""libfedagg_krum.so (include/fedagg_krum.h) and the Krum rules without a GPU: exports, the library's
refusals (each before any HIP call), krum_select against a brute-force loop, and every refusal on the
way to the device from Python."""

from pathlib import Path

import abi_header
import numpy as np
import pytest

from substrafl_amd import _native, _native_krum
from substrafl_amd.engine import krum_select

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "fedagg_krum.h"
A, W, D = 0x100000, 0x200000, 0x400000  # 16-B aligned fakes, never dereferenced
F32, BF16 = _native.FEDAGG_F32, _native.FEDAGG_BF16


def test_signatures_are_the_header():
    names = abi_header.declared_functions(HEADER, "fedagg_krum_")
    assert names == sorted(_native_krum.SIGNATURES) and len(names) == 5
    lib = _native_krum.load()
    assert all(hasattr(lib, n) for n in names)
    assert lib.fedagg_krum_abi_version() == _native_krum.ABI_VERSION == 1
    assert f"#define FEDAGG_KRUM_MAX_K {_native_krum.MAX_K} " in HEADER.read_text() and _native_krum.MAX_K == 128
    chunk, vec_f32, vec_bf16 = _native_krum.blocking()
    assert vec_f32 * 4 == 16 == vec_bf16 * 2 and chunk % (4 * vec_bf16) == 0
    assert lib.fedagg_krum_blocking(None, None, None) == 0
    # one partial triangle of 2 KB tiles per workgroup, more workgroups for more elements, none for none
    sizes = [_native_krum.ws_bytes(128, M) for M in (0, 1, chunk * 1000, 1 << 30, 1 << 44)]
    assert sizes[0] == 0 and sizes == sorted(sizes) and sizes[1] == 36 * 2048 and sizes[3] == sizes[4] <= 1 << 26


def test_refusals_have_their_own_text_and_need_no_gpu():
    """A refused call has made no HIP call, so the fake pointers are never dereferenced."""
    lib = _native_krum.load()

    def gram(rows=(A, A + 64), kind=F32, K=None, M=64, ws=W, ws_bytes=1 << 20, G=D, table=True):
        K = len(rows) if K is None else K
        return lib.fedagg_krum_gram(_native.ptr_array(list(rows)) if table else None, kind, K, M, ws, ws_bytes, G, None)

    cases = [
        (lambda: gram(K=0), b"K is outside [1, FEDAGG_KRUM_MAX_K] (K=0)"),
        (lambda: gram(rows=[A] * 129), b"K is outside [1, FEDAGG_KRUM_MAX_K] (K=129)"),
        (lambda: gram(M=(1 << 44) + 1), b"M is above 2^44"),
        (lambda: gram(kind=9), b"kind 9 is not FEDAGG_F32 / FEDAGG_BF16"),
        (lambda: gram(table=False), b"d_rows is NULL"),
        (lambda: gram(rows=(A, 0)), b"row 1 is NULL"),
        (lambda: gram(rows=(A + 2, A)), b"row 0 is not aligned to its element"),
        (lambda: gram(rows=(A, A + 1), kind=BF16), b"row 1 is not aligned to its element"),
        (lambda: gram(G=None), b"d_G is NULL"),
        (lambda: gram(G=D + 4), b"d_G is not 8-B aligned"),
        (lambda: gram(ws=None), b"d_ws is NULL"),
        (lambda: gram(ws=W + 8), b"d_ws is not 16-B aligned"),
        (lambda: gram(ws_bytes=8191), b"ws_bytes = 8191 is below fedagg_krum_ws_bytes = 8192"),
        (lambda: lib.fedagg_krum_ws_bytes(129, 64, None), b"krum ws_bytes: K is outside"),
        (lambda: lib.fedagg_krum_ws_bytes(2, 64, None), b"bytes is NULL"),
    ]
    texts = []
    for call, needle in cases:
        rc, msg = call(), lib.fedagg_krum_last_error()
        assert rc == -1 and needle in msg, (rc, needle, msg)
        texts.append(msg)
    assert len(set(texts)) == len(texts)  # each refusal speaks for itself


def brute_force(X, f, m):
    """Krum from direct fp64 distances, the way the paper states it; NaN or Inf clients at +inf."""
    K = len(X)
    scores = []
    for i in range(K):
        d = []
        for j in range(K):
            if j != i:
                ok = np.isfinite(X[i]).all() and np.isfinite(X[j]).all()
                d.append(float(((X[i] - X[j]) ** 2).sum()) if ok else np.inf)
        scores.append(sum(sorted(d)[:K - f - 2]))
    order = sorted(range(K), key=lambda i: (scores[i], i))[:m]
    return sorted(order), scores


@pytest.mark.parametrize("K,f,m,bad", [(3, 0, 1, ()), (5, 1, 1, (2,)), (7, 2, 5, (0, 6)), (9, 2, 7, (4,)),
                                       (9, 3, 1, (1, 2, 3)), (8, 1, 7, ())])
def test_krum_select_is_the_brute_force_selection(K, f, m, bad):
    rng = np.random.default_rng(K * 10 + f)
    X = rng.integers(-4, 5, (K, 12)).astype(np.float64)  # small integers: G and every distance are exact
    X[-1] = X[0]  # an exact tie of two scores: the lower index wins
    for k in bad:
        X[k, k % 12] = (np.nan, np.inf)[k % 2]
    with np.errstate(all="ignore"):
        G = X @ X.T
    want, scores = brute_force(X, f, m)
    got = krum_select(G, f, m)
    assert got.tolist() == want and not set(got) & set(bad)
    if not bad:
        assert scores[0] == scores[-1] and (0 in got or K - 1 not in got)


def test_krum_select_refuses_too_many_non_finite_clients():
    X = np.arange(35.0).reshape(7, 5)
    X[[0, 3, 5, 6]] = np.nan  # the three others have two finite distances each and K - f - 2 = 3 to add
    with np.errstate(all="ignore"):
        G = X @ X.T
    with pytest.raises(ValueError, match="more than byzantine=2 clients sent non-finite updates"):
        krum_select(G, 2, 1)
    for f, m in ((3, 1), (-1, 1), (1, 0), (1, 8)):  # K < f + 3, a negative f, a select outside [1, K]
        with pytest.raises(ValueError):
            krum_select(np.eye(7) if f != 3 else np.eye(5), f, m)


def test_python_refusals_come_before_any_device_work(monkeypatch):
    """Neither the session, the device lock nor the library's loader is reached."""
    import standin_substrafl.strategies as ss

    from substrafl_amd import runtime, strategies
    from substrafl_amd.engine import ROBUST_RULES, AggregationEngine
    from substrafl_amd.integration import accelerate
    from substrafl_amd.multi_device import MultiDeviceEngine

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")

    for mod, name in ((runtime, "session"), (runtime, "device_lock"), (_native_krum, "load")):
        monkeypatch.setattr(mod, name, no_device)
    assert ROBUST_RULES[2:] == ("krum", "multi_krum")
    rng = np.random.default_rng(0)
    plain = [[rng.standard_normal(s).astype(np.float32) for s in [(4, 5), (1,)]] for _ in range(7)]
    eng, multi = AggregationEngine(device=0), MultiDeviceEngine.__new__(MultiDeviceEngine)
    for kw, text in [({"byzantine": 3}, r"needs at least 2 f \+ 3 = 9 clients, not 7"),
                     ({"byzantine": 1, "select": 7}, r"select in \[1, K - f\] = \[1, 6\] \(K=7, byzantine=1\), not 7")]:
        with pytest.raises(ValueError, match=text):
            eng.fedavg_robust(plain, "multi_krum", **kw)
    with pytest.raises(NotImplementedError, match="all fp32 or all wire.BF16"):
        eng.fedavg_robust([[a.astype(np.float64) for a in p] for p in plain], "krum", byzantine=1)
    with pytest.raises(NotImplementedError, match="robust route takes up to 128 clients"):
        eng.fedavg_robust([plain[0]] * 129, "krum", byzantine=1)
    with pytest.raises(NotImplementedError, match="out-of-core route has no robust path"):
        AggregationEngine(device=0, max_bucket_bytes=64).fedavg_robust(plain, "krum", byzantine=1)
    with pytest.raises(NotImplementedError, match="MultiDeviceEngine.*no robust route"):
        multi.fedavg_robust(plain, "krum", byzantine=1)

    class Algo:
        strategies = ["Federated Averaging", "Scaffold"]

    for make in (lambda **kw: strategies.FedAvg(algo=Algo(), **kw), lambda **kw: accelerate(ss.FedAvg, **kw)):
        with pytest.raises(ValueError, match="robust must be None, 'trimmed_mean' or 'median', or 'krum' or 'multi_krum'"):
            make(robust="bulyan")
        for rule in ("krum", "multi_krum"):
            for bad in (None, True, 1.0, "1", -1):
                with pytest.raises(ValueError, match=f"robust='{rule}' needs byzantine, an int >= 0"):
                    make(robust=rule, byzantine=bad)
            with pytest.raises(TypeError, match="trim is an option of robust='trimmed_mean'"):
                make(robust=rule, byzantine=1, trim=0.1)
            with pytest.raises(NotImplementedError, match="robust route has no downlink='mxfp8' path"):
                make(robust=rule, byzantine=1, downlink="mxfp8")
        for bad in (0, True, 2.0):
            with pytest.raises(ValueError, match="takes select, an int >= 1"):
                make(robust="multi_krum", byzantine=1, select=bad)
        for kw in ({"robust": "median"}, {"robust": "trimmed_mean", "trim": 0.1}, {}):
            with pytest.raises(TypeError, match="byzantine is an option of robust='krum' and robust='multi_krum'"):
                make(byzantine=1, **kw)
        for kw in ({"robust": "krum", "byzantine": 1}, {"robust": "median"}, {}):
            with pytest.raises(TypeError, match="select is an option of robust='multi_krum'"):
                make(select=2, **kw)
    with pytest.raises(TypeError, match="robust is an option of FedAvg, not of Scaffold"):
        accelerate(ss.Scaffold, robust="krum", byzantine=1)
    # recorded only when given
    assert "byzantine" not in strategies.FedAvg(algo=Algo(), robust="median").kwargs
    given = strategies.FedAvg(algo=Algo(), robust="multi_krum", byzantine=2, select=3)
    assert (given.kwargs["robust"], given.kwargs["byzantine"], given.kwargs["select"]) == ("multi_krum", 2, 3)
    assert "select" not in strategies.FedAvg(algo=Algo(), robust="krum", byzantine=0).kwargs
    cls = accelerate(ss.FedAvg, robust="krum", byzantine=2)
    assert (cls._fedagg_robust, cls._fedagg_byzantine) == ("krum", 2) and not hasattr(accelerate(ss.FedAvg), "_fedagg_byzantine")
