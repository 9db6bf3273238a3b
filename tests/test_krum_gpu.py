"""libfedagg_krum.so on the GPU: the fp64 Gram matrix of the client rows against exact integer
arithmetic and against a long-double reference with a derived bound, at every block count and at the
sizes where the kernel changes path; Krum and multi-Krum end to end against a brute-force selection."""

from __future__ import annotations

import numpy as np
import pytest
import torch  # before the native libraries: one HIP runtime in the process

from substrafl_amd import _native, _native_krum, wire

pytestmark = pytest.mark.gpu
CHUNK, VEC_F32, VEC_BF16 = _native_krum.blocking()  # no HIP call
KINDS = {"f32": (_native.FEDAGG_F32, VEC_F32), "bf16": (_native.FEDAGG_BF16, VEC_BF16)}
KS = (1, 2, 15, 16, 17, 33, 64, 65, 127, 128)
SEVERAL = 8 * CHUNK * 3 + 5  # past one workgroup's smallest share: three workgroups and a tail
GUARD = 64  # doubles of NaN around d_G and d_ws


def sizes(vec):
    return (1, vec - 1, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 47, SEVERAL)


def to_rows(x: np.ndarray, name: str) -> np.ndarray:
    """[K, M] fp32 values as the rows' storage: fp32 itself, or bf16 bits (the values are bf16 already)."""
    return x if name == "f32" else (x.view(np.uint32) >> 16).astype(np.uint16)


def gram(rows: np.ndarray, kind: int, off: int = 0) -> np.ndarray:
    """The library over the [K, M] rows; ``off``: elements by which every row is moved off its 16-B
    alignment.  NaN guard bands lie around d_G and the workspace and must stay NaN; a NaN element lies
    before (``off``) and after every row, so a read outside a row shows in the matrix."""
    K, M = rows.shape
    nan = np.full(1, -1, np.int32).view(rows.dtype)[:1]
    dev = [torch.from_numpy(np.concatenate([nan.repeat(off), rows[k], nan]).view(np.uint8)).cuda() for k in range(K)]
    nws = _native_krum.ws_bytes(K, M)
    ws = torch.full((2 * GUARD + nws // 8,), float("nan"), dtype=torch.float64, device="cuda")
    G = torch.full((2 * GUARD + K * K,), float("nan"), dtype=torch.float64, device="cuda")
    _native_krum.gram([d.data_ptr() + off * rows.itemsize for d in dev], kind, M, ws.data_ptr() + 8 * GUARD, nws,
                      G.data_ptr() + 8 * GUARD, int(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    G, ws = G.cpu().numpy(), ws.cpu().numpy()
    for band in (G[:GUARD], G[GUARD + K * K:], ws[:GUARD], ws[GUARD + nws // 8:]):
        assert np.isnan(band).all()  # nothing outside the matrix and the workspace
    return G[GUARD: GUARD + K * K].reshape(K, K)


@pytest.mark.parametrize("name", list(KINDS))
@pytest.mark.parametrize("K", KS)
def test_small_integers_give_the_exact_matrix(K, name):
    """|x| <= 8: every partial sum is an integer below 2^53, so any order gives the exact matrix."""
    kind, vec = KINDS[name]
    rng = np.random.default_rng(100 * K + len(name))
    for M in sizes(vec):
        xi = rng.integers(-8, 9, (K, M))
        want = (xi @ xi.T).astype(np.float64)
        got = gram(to_rows(xi.astype(np.float32), name), kind)
        assert np.array_equal(got, want), (name, K, M, np.argwhere(got != want)[:4])
        if M in (CHUNK + 1, SEVERAL):  # the element-by-element path: the same matrix
            assert np.array_equal(gram(to_rows(xi.astype(np.float32), name), kind, off=1), want), (name, K, M, "misaligned")
    assert np.array_equal(gram(to_rows(np.zeros((K, 0), np.float32), name), kind), np.zeros((K, K)))  # the empty sum


@pytest.mark.parametrize("name", list(KINDS))
@pytest.mark.parametrize("K", (5, 33, 128))
def test_wide_range_rows_stay_within_the_summation_bound(K, name):
    """|G^ - G| <= gamma_M |X||X|^T, gamma_M = M u / (1 - M u), u = 2^-53: the products are exact, so
    the bound holds for any order of the additions.  The reference is a long-double product."""
    kind, vec = KINDS[name]
    rng = np.random.default_rng(K)
    for M in (2 * CHUNK + 47, SEVERAL):
        x = (rng.standard_normal((K, M)) * 2.0 ** rng.integers(-20, 21, (K, M))).astype(np.float32)
        x = (x.view(np.uint32) & 0xFFFF0000).view(np.float32) if name == "bf16" else x  # bf16 values exactly
        rows = to_rows(x, name)
        xl = x.astype(np.longdouble)
        ref, mag = xl @ xl.T, np.abs(xl) @ np.abs(xl).T
        u = np.longdouble(2.0) ** -53
        bound = M * u / (1 - M * u) * mag
        got = gram(rows, kind)
        err = np.abs(got.astype(np.longdouble) - ref)
        print(f"{name} K={K} M={M}: worst error / bound = {float((err / bound).max()):.3f}")
        assert (err <= bound).all() and np.array_equal(got, got.T)
        assert np.array_equal(gram(rows, kind), got)  # a second call: the same bits
        assert np.array_equal(gram(rows, kind, off=1), got)  # and the misaligned path: the same bits


class Algo:
    strategies = ["Federated Averaging"]


def brute_force_scores(pus, f):
    """Krum's scores from direct long-double distances; a non-finite client at +inf from everyone."""
    X = np.stack([np.concatenate([a.reshape(-1) for a in p]) for p in pus]).astype(np.longdouble)
    K = len(X)
    fin = np.isfinite(X).all(axis=1)
    d = np.array([[((X[i] - X[j]) ** 2).sum() if fin[i] and fin[j] and i != j else np.inf for j in range(K)]
                  for i in range(K)])
    return np.sort(d, axis=1)[:, :K - f - 2].sum(axis=1), X


@pytest.mark.parametrize("rule,m", [("krum", 1), ("multi_krum", 7)])
def test_end_to_end_a_vector_outlier_is_not_selected(rule, m):
    from oracle import fedavg_reference_structure
    from substrafl_amd.engine import engine_for
    from substrafl_amd.schemas import FedAvgSharedState
    from substrafl_amd.strategies import FedAvg

    rng = np.random.default_rng(11)
    shapes, K, f = [(37, 5), (1,), (3, 0), (130,)], 9, 2
    base = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    pus = [[b + np.float32(1e-3) * rng.standard_normal(b.shape).astype(np.float32) for b in base] for _ in range(K)]
    pus[2] = [np.full(s, np.nan, np.float32) for s in shapes]
    pus[6] = [-b for b in base]  # every coordinate within the honest range, the vector opposite to all of them
    scores, X = brute_force_scores(pus, f)
    order = sorted(range(K), key=lambda i: (scores[i], i))
    chosen = sorted(order[:m])
    assert 2 not in chosen and 6 not in chosen
    # the selection margin: the gap between the last selected and the first rejected score against
    # the error of a score formed from the device's G: K - f - 2 distances of three entries each, every
    # entry within gamma_M |x_i|.|x_j| <= gamma_M max |x|^2
    M = X.shape[1]
    margin = float(scores[order[m]] - scores[order[m - 1]])
    bound = (K - f - 2) * 4 * (M * 2.0 ** -53) * float((X[np.isfinite(X).all(axis=1)] ** 2).sum(axis=1).max())
    assert margin > 1e3 * bound, (margin, bound)

    states = [FedAvgSharedState(n_samples=n, parameters_update=p) for n, p in zip(range(1, K + 1), pus)]
    got = FedAvg(algo=Algo(), device=0, robust=rule, byzantine=f).avg_shared_states(shared_states=states, _skip=True)
    assert engine_for(0).last_timing["krum_selected"] == chosen
    ref = fedavg_reference_structure([pus[k] for k in chosen], [1] * m)
    for g, r, p in zip(got.avg_parameters_update, ref, pus[chosen[0]]):
        assert isinstance(g, wire.BucketArray) and g.shape == r.shape and g.dtype == np.float32
        assert np.array_equal(g.view(np.uint32), r.view(np.uint32)) and np.isfinite(g).all()
        assert m > 1 or np.array_equal(g.view(np.uint32), p.view(np.uint32))  # Krum: the chosen client's update itself
    plain = FedAvg(algo=Algo(), device=0).avg_shared_states(shared_states=states, _skip=True)
    assert np.isnan(plain.avg_parameters_update[0]).all()  # what the option exists for
