"""``tests/promote_rules.py`` (the rules of include/fedagg_promote.h in single-dtype ops) against
torch-CPU's own mixed-dtype ops, the reference's expressions (weight_manager.py:137, :205-210):
all 65536 bit patterns of fp16 and bf16 as ``w`` / ``x`` against a fixed set of fp64 partners, and
the constructed operands where a double goes to 16 bits differently through float and directly."""

import numpy as np
import pytest
import torch

import promote_rules as pr

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}


def _all_patterns(dtype):
    return torch.from_numpy(np.arange(1 << 16, dtype=np.uint16).view(np.int16)).view(dtype)


def _grid(dtype):
    """(x, d): every 16-bit pattern next to every fp64 partner."""
    x = _all_patterns(dtype).repeat(len(pr.F64_PARTNERS))
    d = torch.tensor(pr.F64_PARTNERS, dtype=torch.float64).repeat_interleave(1 << 16)
    return x, d


@pytest.mark.parametrize("kind", sorted(DTYPES))
@pytest.mark.parametrize("mult", pr.MULTIPLIERS)
def test_increment_rule_is_torch_cpu(kind, mult):
    w, u = _grid(DTYPES[kind])
    ref = w.clone()
    ref += mult * u  # weight_manager.py:137 on a 16-bit parameter and an fp64 update
    assert ref.dtype == DTYPES[kind]
    assert pr.same_bits(pr.increment(w, u, mult), ref) == 0


@pytest.mark.parametrize("kind", sorted(DTYPES))
@pytest.mark.parametrize("case", range(len(pr.WSUM_CASES)))
def test_wsum_rule_is_torch_cpu(kind, case):
    kinds, coeffs = pr.WSUM_CASES[case]
    x, d = _grid(DTYPES[kind])
    rolls = iter(range(1, 9))  # the lists differ: the same patterns and partners, shifted against each other
    lists = [torch.roll(x, 257 * next(rolls)) if k == "T" else torch.roll(d, 65536 * next(rolls) + 11) for k in kinds]
    ref = sum(p * c for p, c in zip(lists, coeffs))  # weight_manager.py:205-210
    assert ref.dtype == torch.float64
    assert pr.same_bits(pr.wsum(lists, coeffs), ref) == 0


@pytest.mark.parametrize("kind", sorted(DTYPES))
def test_double_rounding_set_tells_the_two_conversions_apart(kind):
    dtype = DTYPES[kind]
    w, t = pr.double_rounding_operands(dtype)
    for mult in pr.MULTIPLIERS:
        u = t / mult
        ref = w.clone()
        ref += mult * u
        got = pr.increment(w, u, mult)
        assert pr.same_bits(got, ref) == 0
        direct = pr.round_direct((w.to(torch.float64) + mult * u).numpy(), dtype)
        differ = int((pr.as_bits(direct) != pr.as_bits(ref)).sum())
        assert differ >= 100, (kind, mult, differ)  # a direct conversion cannot pass
        assert differ == w.numel(), (kind, mult, differ, w.numel())  # in fact every element of the set


def test_through_float_example_of_the_header():
    """1 + 2^-11 + 2^-40 is fp16 0x3C00 through float and 0x3C01 in one rounding."""
    w = torch.tensor([1.0], dtype=torch.float16)
    u = torch.tensor([2.0 ** -11 + 2.0 ** -40], dtype=torch.float64)
    assert int(pr.as_bits(pr.increment(w, u, 1.0))[0]) == 0x3C00
    assert int(pr.as_bits(pr.round_direct((w.double() + u).numpy(), torch.float16))[0]) == 0x3C01
