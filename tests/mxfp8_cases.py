"""Inputs shared by the MXFP8 tests (host and GPU): the e4m3fn value table and hand-made blocks
whose scale bytes and codes are worked out here from the rule's text (substrafl_amd/wire.py), not
by running an encoder."""

import numpy as np


def all_values() -> np.ndarray:
    """The 127 non-negative finite e4m3fn values (codes 0x00 .. 0x7E), ascending, as float64."""
    c = np.arange(0x7F)
    E, m = c >> 3, c & 7
    return np.where(E == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (E - 10.0))


def hand_blocks():
    """name -> (x fp32, expected scale bytes, {flat position: expected code})."""
    f = np.float32
    out = {}

    # amax exactly 464: e = 8 - 8 = 0, 464 is not > 464: s = 127, and 464 is the tie that rounds to 448
    x = np.zeros(32, f)
    x[3], x[9] = -464.0, 1.0  # 1.0 = 8 * 2^-3: E = 7, m = 0
    out["amax_464"] = (x, [127], {3: 0xFE, 9: 0x38, 0: 0x00})

    # the next float above 464: e = 1, s = 128; y = 232.00002 lies just above the midpoint of 224 and 240
    x = np.zeros(32, f)
    x[3], x[9] = np.nextafter(f(464.0), f(np.inf)), 1.0  # y(1.0) = 0.5: E = 6
    out["amax_464_next"] = (x, [128], {3: 0x77, 9: 0x30})

    # amax an fp32 subnormal, 1.5 * 2^-127: e = -127 - 8 = -135 clamps to -127, s = 0, y = x * 2^127
    x = np.zeros(32, f)
    x[0] = 1.5 * 2.0 ** -127  # y = 1.5: E = 7, m = 4
    x[1] = -(2.0 ** -149)     # y = -2^-22: below half the granule 2^-9, a negative zero
    x[2] = 2.0 ** -136        # y = 2^-9: the smallest e4m3fn subnormal
    x[5] = -3 * 2.0 ** -136   # y = -3 * 2^-9
    out["amax_subnormal"] = (x, [0], {0: 0x3C, 1: 0x80, 2: 0x01, 5: 0x83, 7: 0x00})

    # amax near 3e38 = 451.4 * 2^119: fl = 127, e = 119, s = 246; 451.4 rounds to 448
    x = np.zeros(32, f)
    x[0], x[5] = 3e38, -1e38  # y(-1e38) = -150.46: between 144 and 160, below their midpoint: 144 = 9 * 2^4
    out["amax_3e38"] = (x, [246], {0: 0x7E, 5: 0xF1})

    # an all-zero block: s = 127, the codes carry the signs
    x = np.zeros(32, f)
    x[1] = x[30] = -0.0
    out["all_zero_negative_zeros"] = (x, [127], {0: 0x00, 1: 0x80, 30: 0x80, 31: 0x00})

    # a NaN poisons its block only: s = 255 and every code 0x00; amax 1.0: e = -8, s = 119, y = 256
    x = np.ones(64, f)
    x[4] = np.nan
    out["nan_block"] = (x, [255, 119], {0: 0x00, 4: 0x00, 31: 0x00, 32: 0x78, 63: 0x78})

    x = np.full(32, 2.0, f)
    x[7] = -np.inf
    out["inf_block"] = (x, [255], {0: 0x00, 7: 0x00, 31: 0x00})

    # M = 40: the last block has 8 elements, amax 3.0: fl = 1, e = -7, s = 120; y = 384 = 12 * 2^5
    x = np.ones(40, f)
    x[32], x[33] = 3.0, -0.75  # y(-0.75) = -96 = 12 * 2^3: E = 13, m = 4
    out["partial_last_block"] = (x, [119, 120], {0: 0x78, 32: 0x7C, 33: 0xEC, 39: 0x70})
    return out


def golden_cases():
    """The cases of tests/golden/golden_mxfp8.npz (the reference's own FedAvg on the decoded
    inputs): [(key, kind, updates, n_samples, expected fp32 layers)], ``updates[k]`` client k's
    MXFP8 update ``[E4M3 layers ..., E8M0 scales]``."""
    import json
    from pathlib import Path

    from substrafl_amd.wire import E4M3, E8M0

    d = Path(__file__).resolve().parent / "golden"
    arrays = np.load(d / "golden_mxfp8.npz", allow_pickle=False)
    out = []
    for case in json.loads((d / "golden_mxfp8_meta.json").read_text())["cases"]:
        key, shapes = case["key"], [tuple(s) for s in case["shapes"]]
        cuts = np.cumsum([0] + [int(np.prod(s)) for s in shapes])
        codes, scales = arrays[f"{key}/codes"], arrays[f"{key}/scales"]
        assert codes.shape == (case["K"], cuts[-1]) and scales.shape == (case["K"], -(-cuts[-1] // 32))
        updates = [[codes[k, a:b].reshape(s).view(E4M3) for a, b, s in zip(cuts, cuts[1:], shapes)]
                   + [scales[k].view(E8M0)] for k in range(case["K"])]
        want = [arrays[f"{key}/out"][a:b].reshape(s) for a, b, s in zip(cuts, cuts[1:], shapes)]
        out.append((key, case["kind"], updates, [int(n) for n in arrays[f"{key}/n_samples"]], want))
    return out
