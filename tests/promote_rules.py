"""The arithmetic rules of ``include/fedagg_promote.h`` restated in SINGLE-dtype torch ops on the
CPU (no op below sees two dtypes, so torch's promotion is never asked): the second reference of
``tests/test_promote_ops_gpu.py``, itself held to torch-CPU's own mixed-dtype ops over every
16-bit pattern by ``tests/test_promote_rules.py``.  Also the constructed operands on which rounding
a double to 16 bits through float and rounding it directly differ."""

import numpy as np
import torch

MANT_BITS = {torch.float16: 10, torch.bfloat16: 7}
EXP_BIAS = {torch.float16: 15, torch.bfloat16: 127}
# +-0, +-inf, NaN, huge, tiny (1e-320 is an fp64 subnormal) and ordinary values
F64_PARTNERS = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1e300, -1e300, 1e-300, 1e-320,
                1.0, -0.37, 3.0000000001, 1 / 3, -1024.5, 65504.0, 2.0 ** -25]
MULTIPLIERS = [1.0, 0.05, -2.5]
WSUM_CASES = [  # (list kinds: "T" the 16-bit kind, "64" fp64; coefficients)
    (["T", "64"], [1, -1]),
    (["64", "T"], [-1.0, -1.0 / (0.05 * 100)]),
    (["T", "64"], [1, 1]),
    (["T", "T", "64", "T"], [0.3, 1 / 3, -1e-3, 7.7]),
    (["64", "64", "T"], [0.3, 1 / 3, -1e-3]),
]


def _f32(c):
    return torch.tensor(float(c), dtype=torch.float64).to(torch.float32)  # the Python scalar as torch takes it


TORCH_F16_BLOCK = 2048  # elements torch on ROCm serves per block of its vectorised fp16 kernels


def product(x, c, once=None):
    """``x * python_scalar``: a 16-bit list in fp32 with the scalar rounded to fp32, rounded once
    more to T; an fp64 list in fp64.  ``once`` (a bool mask, fp16 only) marks the elements torch
    ON THE DEVICE serves in the unrolled remainder of a tensor (:func:`torch_remainder`): there
    the EXACT product is rounded once to fp16, and an exact zero product is +0."""
    if x.dtype == torch.float64:
        return x * torch.tensor(float(c), dtype=torch.float64)
    p = (x.to(torch.float32) * _f32(c)).to(x.dtype)
    if once is not None and x.dtype == torch.float16:
        exact = x.to(torch.float64) * _f32(c).to(torch.float64)  # 11 x 24 bits: exact in fp64
        with np.errstate(all="ignore"):
            fused = torch.from_numpy(exact.numpy().astype(np.float16))  # NumPy rounds fp64 -> fp16 in one step
        zero = (x == 0) | (_f32(c) == 0)
        fused = torch.where(zero & (fused == 0), torch.zeros_like(fused), fused)
        p = torch.where(once, fused, p)
    return p


def torch_remainder(numel):
    """Mask over layers laid back to back: True where an element lies in the trailing
    ``n mod TORCH_F16_BLOCK`` elements of its layer (a tensor of its own, as the reference has)."""
    parts = [torch.arange(n) >= n // TORCH_F16_BLOCK * TORCH_F16_BLOCK for n in numel]
    return torch.cat(parts) if parts else torch.zeros(0, dtype=torch.bool)


def wsum(lists, coeffs, once=None):
    """Python ``sum()`` from int 0 over ``product(x_j, c_j)``, one layer (a list of tensors, one per list)."""
    acc = None
    for x, c in zip(lists, coeffs):
        p = product(x, c, once)
        if acc is None:  # 0 + p_0 in p_0's own kind: -0 becomes +0
            acc = (torch.zeros((), dtype=torch.float32) + p.to(torch.float32)).to(p.dtype) if p.dtype != torch.float64 \
                else torch.zeros((), dtype=torch.float64) + p
        elif acc.dtype != torch.float64 and p.dtype != torch.float64:
            acc = (acc.to(torch.float32) + p.to(torch.float32)).to(acc.dtype)
        else:  # either side fp64: the 16-bit side widened exactly, the sum in fp64
            acc = acc.to(torch.float64) + p.to(torch.float64)
    return acc


def increment(w, u, m):
    """``w += m * u`` with w 16-bit and u fp64: t = m * u and the sum in fp64, then to T through
    float (two roundings).  Returns the new w."""
    t = u * torch.tensor(float(m), dtype=torch.float64)
    return (w.to(torch.float64) + t).to(torch.float32).to(w.dtype)


def round_direct(s, dtype):
    """fp64 -> dtype in ONE rounding (nearest even), for values whose result is normal and finite:
    what the increment must NOT do."""
    s = np.asarray(s, dtype=np.float64)
    m, e = np.frexp(s)
    q = np.rint(m * 2.0 ** (MANT_BITS[dtype] + 1)) / 2.0 ** (MANT_BITS[dtype] + 1)  # exact in fp64
    return torch.from_numpy(np.ldexp(q, e)).to(dtype)  # exactly representable: no rounding here


def double_rounding_operands(dtype):
    """(w, t): every normal w of ``dtype`` with an exponent well inside the range, and the fp64 t
    for which fl64(w + t) lies just beyond the midpoint of w and its neighbour away from zero
    (even mantissa: by 2^-29 of half an ulp above it) or just short of it (odd mantissa).  Rounded
    to float first the sum lands ON the midpoint and the tie goes to the even neighbour -- the
    opposite of where one direct rounding goes."""
    mb, bias = MANT_BITS[dtype], EXP_BIAS[dtype]
    exps = np.arange(bias - 6, bias + 7, dtype=np.int64)
    mant = np.arange(1 << mb, dtype=np.int64)
    bits = ((exps[:, None] << mb) | mant[None, :]).reshape(-1)
    bits = np.concatenate([bits, bits | 0x8000]).astype(np.uint16)
    w = torch.from_numpy(bits.view(np.int16)).view(dtype)
    wd = w.to(torch.float64).numpy()
    _, e = np.frexp(wd)
    half_ulp = np.ldexp(1.0, e - 1 - mb - 1)  # |w| in [2^(e-1), 2^e): ulp = 2^(e-1-mb)
    odd = (bits & 1).astype(bool)
    t = np.sign(wd) * half_ulp * np.where(odd, 1.0 - 2.0 ** -29, 1.0 + 2.0 ** -29)
    return w, torch.from_numpy(t)


def as_bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int64)


def same_bits(got, ref):
    """Equal bit for bit, NaN-ness only where the reference is NaN; returns the count of elements that differ."""
    nan = torch.isnan(ref)
    bad = (torch.isnan(got) != nan) | (~nan & (as_bits(got) != as_bits(ref)))
    return int(bad.sum())
