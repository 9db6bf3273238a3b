"""libfedagg_robust.so on the GPU: the trimmed mean and the median against NumPy, bit for bit (NaN by
position), at every padded client count and at the sizes where the kernel changes path."""

from __future__ import annotations

import numpy as np
import pytest
import torch  # before the native libraries: one HIP runtime in the process

from substrafl_amd import _native, _native_robust, wire

pytestmark = pytest.mark.gpu
TILE, VEC_F32, VEC_BF16 = _native_robust.blocking()  # no HIP call
KINDS = {"f32": (_native.FEDAGG_F32, np.uint32, VEC_F32), "bf16": (_native.FEDAGG_BF16, np.uint16, VEC_BF16)}
QNAN = 0x7FC00000
# bit patterns of the few values rows are drawn from, so that ties are the rule: +-0, small integers,
# +-inf, the largest finite, subnormals; then NaNs of both signs
F32_SET = np.array([0, 0x80000000, 0x3F800000, 0xBF800000, 0x40000000, 0xC0000000, 0x40400000, 0xC0400000, 0x7F800000,
                    0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 1, 0x80000001, 0x00400000], np.uint32)
F32_NAN = np.array([0x7FC00000, 0xFFC00001, 0x7F800001], np.uint32)


def widen(bits: np.ndarray) -> np.ndarray:
    return bits.view(np.float32) if bits.dtype == np.uint32 else (bits.astype(np.uint32) << 16).view(np.float32)


def reference(x: np.ndarray, t: int) -> np.ndarray:
    """np.sort's order (NaN last, +-0 equal), the window [t, K - t), fp32 adds from +0.0, one fp32 division."""
    K = x.shape[0]
    kept = np.sort(x, axis=0)[t:K - t]
    with np.errstate(all="ignore"):
        acc = np.zeros(x.shape[1], np.float32)
        for v in kept:
            acc = acc + v
        return acc / np.float32(K - 2 * t)


def run(bits: np.ndarray, kind: int, t: int, off: int = 0) -> np.ndarray:
    """The library over the [K, M] rows of bit patterns; the result's bits.  ``off``: elements by which
    every row and d_out are moved off their 16-B alignment.  A NaN guard band lies around d_out."""
    K, M = bits.shape
    pad = np.zeros(off, bits.dtype)
    rows = [torch.from_numpy(np.concatenate([pad, bits[k]]).view(np.uint8)).cuda() for k in range(K)]
    out = torch.full((M + off + 8,), float("nan"), dtype=torch.float32, device="cuda")
    _native_robust.mean([r.data_ptr() + off * bits.itemsize for r in rows], kind, t, M, out.data_ptr() + 4 * off,
                        int(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert (got[:off] == QNAN).all() and (got[off + M:] == QNAN).all()  # nothing outside the row
    return got[off: off + M]


def same(got_bits, ref, what):
    nan = np.isnan(ref)
    assert np.array_equal((got_bits & 0x7FFFFFFF) > 0x7F800000, nan), f"{what}: NaN positions differ"
    bad = np.flatnonzero((got_bits != ref.view(np.uint32)) & ~nan)
    assert bad.size == 0, (what, bad.size, bad[:8], [hex(v) for v in got_bits[bad[:8]]], ref[bad[:8]])


def rows_of(rng, name: str, K: int, M: int) -> np.ndarray:
    """[K, M] bit patterns of the value set, NaNs of both signs over about 2 % of the positions; from
    M = 2 on the last element is NaN for every client (more NaNs than any t trims)."""
    bits = rng.choice(F32_SET, (K, M))
    nan = rng.random((K, M)) < 0.02
    bits[nan] = rng.choice(F32_NAN, int(nan.sum()))
    if M > 1:
        bits[:, -1] = F32_NAN[0]
    # bf16: the high halves (the largest finite becomes 0x7F7F, the subnormals 2^-133 .. and +-0)
    return bits if name == "f32" else (bits >> 16).astype(np.uint16)


def trims(K: int):
    return sorted({t for t in (0, 1, K // 10, (K - 1) // 2) if 2 * t < K})


K_T = [(K, t) for K in (1, 2, 3, 4, 5, 8, 9, 17, 33, 64, 65, 127, 128) for t in trims(K)]


@pytest.mark.parametrize("name", list(KINDS))
@pytest.mark.parametrize("K,t", K_T, ids=[f"K{K}-t{t}" for K, t in K_T])
def test_kernel_against_numpy(K, t, name):
    kind, _, vec = KINDS[name]
    rng = np.random.default_rng(1000 * K + 10 * t + len(name))
    few = many = False
    for M in (1, vec - 1, TILE - 1, TILE + 1, 2 * TILE + 47):
        bits = rows_of(rng, name, K, M)
        x = widen(bits)
        n_nan = np.isnan(x).sum(axis=0)
        few, many = few or bool((n_nan <= t).any()), many or bool((n_nan > t).any())
        same(run(bits, kind, t), reference(x, t), f"{name} K={K} t={t} M={M}")
    assert few and many  # elements whose NaNs are all trimmed, and elements that stay NaN


@pytest.mark.parametrize("name", list(KINDS))
def test_plain_walk_has_the_vector_walk_bits(name):
    kind, _, _ = KINDS[name]
    K, t, M = 9, 2, TILE + 47
    bits = rows_of(np.random.default_rng(7), name, K, M)
    vector = run(bits, kind, t)
    same(vector, reference(widen(bits), t), name)
    assert np.array_equal(run(bits, kind, t, off=1), vector)


def test_median_special_cases():
    big = np.finfo(np.float32).max
    odd = np.array([[3, -0.0, 7], [1, -5, 1e-40], [2, -0.0, -2], [9, 4, 5], [-1, -0.0, 6]], np.float32)
    got = run(odd.view(np.uint32), _native.FEDAGG_F32, 2)  # an input value exactly, except -0.0 -> +0.0
    assert np.array_equal(got, np.array([2, 0.0, 5], np.float32).view(np.uint32))
    even = np.array([[big], [-1], [big], [big]], np.float32)  # the two middle values: the sum overflows before the division
    assert run(even.view(np.uint32), _native.FEDAGG_F32, 1).tolist() == [0x7F800000]


@pytest.mark.parametrize("robust,trim,t", [("median", None, 2), ("trimmed_mean", 0.2, 1)])
def test_end_to_end_a_bad_client_no_longer_poisons_the_round(robust, trim, t):
    from substrafl_amd.schemas import FedAvgSharedState
    from substrafl_amd.strategies import FedAvg

    class Algo:
        strategies = ["Federated Averaging"]

    rng = np.random.default_rng(3)
    shapes = [(37, 5), (1,), (0,)]
    pus = [[rng.standard_normal(s).astype(np.float32) for s in shapes] for _ in range(5)]
    pus[1] = [np.full(s, np.nan, np.float32) for s in shapes]
    pus[3] = [a * np.float32(1e30) for a in pus[3]]
    states = [FedAvgSharedState(n_samples=n, parameters_update=p) for n, p in zip((5, 1, 9, 2, 7), pus)]
    opts = {} if trim is None else {"trim": trim}
    got = FedAvg(algo=Algo(), device=0, robust=robust, **opts).avg_shared_states(shared_states=states, _skip=True)
    for li, g in enumerate(got.avg_parameters_update):
        ref = reference(np.stack([p[li].reshape(-1) for p in pus]), t).reshape(shapes[li])
        assert isinstance(g, wire.BucketArray) and g.shape == ref.shape and g.dtype == np.float32  # wire=True
        assert np.array_equal(g.view(np.uint32), ref.view(np.uint32)) and np.isfinite(g).all()
    plain = FedAvg(algo=Algo(), device=0).avg_shared_states(shared_states=states, _skip=True)
    assert np.isnan(plain.avg_parameters_update[0]).all()  # what the option exists for
