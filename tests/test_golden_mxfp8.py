"""tests/golden/golden_mxfp8.npz holds what the reference's own ``FedAvg.avg_shared_states``
returned on exactly decoded MXFP8 updates.  The oracle on ``wire.mxfp8_to_float32`` of the stored
codes and scales must reproduce it bit for bit: the yardstick of the GPU route is the reference's."""

import numpy as np
import pytest

from mxfp8_cases import golden_cases
from oracle import fedavg_reference_structure
from substrafl_amd import wire

CASES = golden_cases()


def test_the_fixture_covers_what_it_should():
    kinds = {kind for _, kind, *_ in CASES}
    assert {"table", "edge", "span", "negative-weight", "huge-counts"} <= kinds
    assert max(len(u) for _, _, u, _, _ in CASES) == 200
    assert any(min(ns) < 0 for *_, ns, _ in CASES) and any(max(ns) > 2 ** 53 for *_, ns, _ in CASES)
    assert all(any(a.size == 1 for a in want) for *_, want in CASES)  # numel == 1 layers in every case


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_oracle_on_the_decoded_inputs_is_the_reference(case):
    key, _kind, updates, ns, want = case
    assert all(wire.is_mxfp8(u) and wire.mxfp8_check(u) == sum(w.size for w in want) for u in updates)
    decoded = [wire.mxfp8_to_float32(u[:-1], u[-1]) for u in updates]
    got = fedavg_reference_structure(decoded, ns)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype == np.float32 and g.shape == w.shape
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), key
