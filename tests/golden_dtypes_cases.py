"""Readers of ``tests/golden/golden_dtypes.npz`` and ``golden_plumbing_half.npz`` (the reference's
own outputs over every non-fp32 path, tests/golden/gen_golden_dtypes.py and gen_plumbing_half.py)
and the one comparison rule both test files use.  Loaded by path; read-only: the arrays are shared
between tests."""

import json
from pathlib import Path

import numpy as np

D = Path(__file__).resolve().parent / "golden"
_cache = {}


def _load(stem: str, meta_stem: str):
    if stem not in _cache:
        with np.load(D / f"{stem}.npz", allow_pickle=False) as z:
            arrays = {k: z[k] for k in z.files}
        for a in arrays.values():
            a.setflags(write=False)
        _cache[stem] = (arrays, json.loads((D / f"{meta_stem}.json").read_text()))
    return _cache[stem]


def dtypes_fixture():
    return _load("golden_dtypes", "golden_dtypes_meta")


def half_fixture():
    return _load("golden_plumbing_half", "golden_plumbing_half_meta")


def _split(flat, shapes):
    out, off = [], 0
    for s in shapes:
        n = int(np.prod(s))
        out.append(flat[off: off + n].reshape(s))
        off += n
    assert off == flat.size
    return out


def layers(arrays, key: str, role: str, shapes, K=None):
    """The layers ``put_layers`` stored: one list, or with ``K`` one list per client."""
    def one(pre):
        if pre in arrays:
            return _split(arrays[pre], shapes)
        return [arrays[f"{pre}{li}"] for li in range(len(shapes))]

    if K is None:
        return one(f"{key}/{role}")
    if f"{key}/{role}" in arrays:
        a = arrays[f"{key}/{role}"]
        assert a.shape[0] == K
        return [_split(a[k], shapes) for k in range(K)]
    return [one(f"{key}/k{k}/{role}") for k in range(K)]


def fedavg_cases(kinds=None):
    """(case, n_samples as the reference was given them, clients' layers, reference output)."""
    arrays, meta = dtypes_fixture()
    for case in meta["cases"]:
        if case["strategy"] != "fedavg" or (kinds is not None and case["kind"] not in kinds):
            continue
        key, shapes = case["key"], [tuple(s) for s in case["shapes"]]
        ns = case.get("n_samples_as_given") or [int(v) for v in arrays[f"{key}/n_samples"]]
        yield case, ns, layers(arrays, key, "x", shapes, case["K"]), layers(arrays, key, "out", shapes)


def scaffold_cases():
    """(case, n_samples, deltas, control variates, c per client, lr, (avg, new c) or None).  Clients
    that were handed one c share the very same list, as in the reference run."""
    arrays, meta = dtypes_fixture()
    for case in meta["cases"]:
        if case["strategy"] != "scaffold":
            continue
        key, K, shapes = case["key"], case["K"], [tuple(s) for s in case["shapes"]]
        ns = [int(v) for v in arrays[f"{key}/n_samples"]]
        pu, cv = layers(arrays, key, "pu", shapes, K), layers(arrays, key, "cv", shapes, K)
        cs = layers(arrays, key, "c", shapes, K) if case["c_per_client"] else [layers(arrays, key, "c", shapes)] * K
        lr = int(case["lr"]) if case["lr_is_int"] else float(case["lr"])
        out = None
        if case["error"] is None:
            out = (layers(arrays, key, "avg", shapes), layers(arrays, key, "newc", shapes))
        yield case, ns, pu, cv, cs, lr, out


def half_calls():
    """(config name, call, n_samples, deltas, {cv, c per client}, {avg[, c]}) of every recorded
    aggregation of the fp16 simulations."""
    arrays, meta = half_fixture()
    for name, cfg in meta["configs"].items():
        for call in cfg["calls"]:
            key, K, L = call["key"], call["K"], call["layers"]
            ns = [int(v) for v in arrays[f"{key}/n_samples"]]
            pu = [[arrays[f"{key}/k{k}/pu{li}"] for li in range(L)] for k in range(K)]
            extra, out = {}, {"avg": [arrays[f"{key}/out_avg{li}"] for li in range(L)]}
            if call["kind"] == "scaffold":
                extra["cv"] = [[arrays[f"{key}/k{k}/cv{li}"] for li in range(L)] for k in range(K)]
                extra["c"] = [[arrays[f"{key}/k{k}/c{li}"] for li in range(L)] for k in range(K)]
                out["c"] = [arrays[f"{key}/out_c{li}"] for li in range(L)]
            yield name, call, ns, pu, extra, out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(got, ref, what) -> None:
    """The comparison rule: same dtype, same shape, same bits wherever the reference is not NaN,
    NaN exactly where the reference has NaN (a NaN's payload and sign are not compared)."""
    assert len(got) == len(ref), what
    for li, (g, r) in enumerate(zip(got, ref)):
        g, r = np.asarray(g), np.asarray(r)
        assert g.dtype == r.dtype and g.shape == r.shape, (what, li, g.dtype, r.dtype, g.shape, r.shape)
        nan = np.isnan(r)
        assert np.array_equal(np.isnan(g), nan), (what, li, "NaN placement")
        bad = (bits(g) != bits(r)) & ~nan
        assert not bad.any(), (what, li, f"{int(bad.sum())} of {r.size} elements differ, first at "
                                         f"{np.argwhere(bad)[0].tolist()}: {g[bad][0]!r} != {r[bad][0]!r}")


def nan_share(outs) -> float:
    return sum(int(np.isnan(o).sum()) for o in outs) / sum(int(np.asarray(o).size) for o in outs)
