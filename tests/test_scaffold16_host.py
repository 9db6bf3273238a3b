"""The host-side pieces of Scaffold over 16-bit buckets that need no device: which buckets count
as 16-bit, the server-control-variate equality rule on fp16 / ``wire.BF16`` copies
(scaffold.py:193-196: value equality, +0 == -0, NaN == NaN), the one-bucket plan's byte count, and
the client's ``zeros_like_parameters`` / ``export_numpy`` on CPU tensors."""

import numpy as np
import pytest
import torch

from substrafl_amd import wire
from substrafl_amd.algorithms import weight_manager as wm
from substrafl_amd.engine import ScaffoldBucketPlan, bucket_dtype16, c_mismatches16


def _bf16(x):
    return wire.float32_to_bf16(np.asarray(x, np.float32))


def test_bucket_dtype16():
    h = [np.ones(3, np.float16), np.ones((), np.float16)]
    b = [_bf16([1, 2]), _bf16(3.0)]
    assert bucket_dtype16([h, h]) == np.float16
    assert bucket_dtype16([b, b]) == wire.BF16
    assert bucket_dtype16([h, b]) is None  # two 16-bit kinds in one bucket
    assert bucket_dtype16([h, [np.ones(3, np.float32), h[1]]]) is None
    assert bucket_dtype16([[np.ones(3, np.float64)]]) is None


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_c_equality_rule(kind):
    mk = (lambda x: np.asarray(x, np.float16)) if kind == "f16" else _bf16
    nan = 0x7E00 if kind == "f16" else 0x7FC0
    c = [mk([[1.5, -2.0, 0.0], [3.0, 0.25, -0.0]]), mk(7.0), mk([0.5])]
    copy = [a.copy() for a in c]
    assert c_mismatches16([c, c, c]) == (0, "host-bytes")  # identical objects
    assert c_mismatches16([c, copy]) == (0, "host-bytes")  # byte-identical copies
    # +0 against -0, and NaN against a NaN of another payload: compared by value, equal
    z = [a.copy() for a in c]
    z[0].view(np.uint16)[0, 2] = 0x8000
    z[0].view(np.uint16)[1, 2] = 0x0000
    ref = [a.copy() for a in c]
    ref[2].view(np.uint16)[0] = nan
    z[2].view(np.uint16)[0] = nan | 1
    assert c_mismatches16([ref, z]) == (0, "host-values")
    # NaN against a number, and two different numbers: one mismatch each, per copy
    bad = [a.copy() for a in ref]
    bad[2].view(np.uint16)[0] = c[2].view(np.uint16)[0]
    bad[1].view(np.uint16)[()] ^= 0x0100
    assert c_mismatches16([ref, bad]) == (2, "host-values")
    assert c_mismatches16([ref, bad, ref, bad]) == (4, "host-values")
    assert c_mismatches16([ref]) == (0, "host-bytes")


def test_one_bucket_plan_counts_two_byte_inputs():
    K, M = 4, 1000
    rows, w = [4096 * (k + 1) for k in range(K)], np.full(K, 0.25)
    delta = ScaffoldBucketPlan("bf16", rows, 0, None, None, w, M, 0.7, 1 << 20)
    cv = ScaffoldBucketPlan("f16", rows, 1, 1 << 21, "f64", w, M, 0.7, 1 << 20)
    assert delta.bytes_alg() == 2 * K * M + 8 * M
    assert cv.bytes_alg() == 2 * K * M + 8 * M + 8 * M
    with pytest.raises(ValueError):
        ScaffoldBucketPlan("i8", rows, 0, None, None, w, M, 0.7, 1 << 20)
    with pytest.raises(ValueError):
        ScaffoldBucketPlan("f16", rows, 1, 1 << 21, None, w, M, 0.7, 1 << 20)


def test_export_numpy_fallback_carries_bf16():
    ts = [torch.tensor([[1.0, -2.5], [0.0, 3.0]], dtype=torch.bfloat16), torch.tensor(0.5, dtype=torch.bfloat16)]
    out = wm.export_numpy([ts[0].t(), ts[1]])  # not one flat bucket: the per-tensor fallback
    assert [a.dtype for a in out] == [wire.BF16, wire.BF16] and [a.shape for a in out] == [(2, 2), ()]
    assert np.array_equal(wire.bf16_to_float32(out[0]), ts[0].t().float().numpy())
    assert float(wire.bf16_to_float32(out[1])) == 0.5
    plain = wm.export_numpy([torch.ones(2, 2).t(), torch.ones(3)])
    assert all(isinstance(a, np.ndarray) and a.dtype == np.float32 for a in plain)
    if hasattr(torch, "float8_e4m3fn"):  # a dtype NumPy lacks still raises, as the reference's .numpy()
        with pytest.raises(TypeError):
            wm.export_numpy([torch.zeros(2, dtype=torch.float8_e4m3fn)])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_zeros_like_parameters_keeps_the_model_dtype_on_the_cpu(dtype):
    model = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.BatchNorm1d(4)).to(dtype)
    z = wm.zeros_like_parameters(model, with_batch_norm_parameters=True, device=torch.device("cpu"))
    ps = list(wm.model_parameters(model, with_batch_norm_parameters=True)())
    assert [t.shape for t in z] == [p.shape for p in ps]
    assert all(t.dtype == dtype and not t.is_cuda and not t.any() for t in z)
