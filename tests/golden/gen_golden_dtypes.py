"""Golden vectors for every non-fp32 aggregation path, produced by the REFERENCE itself.

CONTAINER-ONLY, like ``gen_golden.py`` (whose reference import and ``substra`` stubs it uses): it
refuses to run without the reference, never writes bytecode into it, and writes only data:
``golden_dtypes.npz`` and ``golden_dtypes_meta.json``.  Every case stores its inputs, ``n_samples``
and what ``FedAvg.avg_shared_states`` / ``Scaffold.avg_shared_states`` (``_skip=True``) returned,
dtype and shape as produced.  tests/test_golden_dtypes.py (oracle, stand-in) and
tests/test_golden_dtypes_gpu.py (every engine route) compare with these arrays directly.

Layout of the archive (``meta["cases"]`` lists the keys and the layer ``shapes``).  A list of layers
is one member ``{key}/{role}`` holding the raveled layers end to end when they share a dtype, else
one member ``{key}/{role}{li}`` per layer (``put_layers``; tests/golden_dtypes_cases.py reads both):
  fedavg    ``{key}/n_samples``; role ``k{k}/x`` per client; ``out``.
  scaffold  ``{key}/n_samples``; roles ``k{k}/pu``, ``k{k}/cv``; ``c`` (one c shared by every client,
            as a simulation hands it out) or ``k{k}/c`` (``c_per_client``); ``avg``, ``newc``; a case
            the reference refuses has ``error`` and no outputs.
A role with the same dtype for every client is stacked into one member, ``{key}/{role}`` without
the ``k{k}/`` (rows = clients).

Sizes: the project's contribution rules cap a newly committed file at 1 MiB (tighter than the older
``golden_aggregation.npz``), so the layer sets are small (both ``numel == 1`` forms, a matrix and
a ragged vector), int64 / int32 / uint8 run at fewer K, float32 / float64 inputs at K >= 127 and
in the long-layer cases are float16-representable values, float16 ones there keep 8 significant
bits (compressible; the weights make every product a full-mantissa number anyway, and K <= 9
keeps full-entropy inputs), and the long ragged layer has 20 011 (fp16) or 6 151 (fp64) elements
at K = 2 and 4 099 at K = 8.  The archive is written with fixed zip timestamps, so a second run
reproduces it byte for byte.  Run:  python tests/golden/gen_golden_dtypes.py
"""

from __future__ import annotations

import io
import json
import sys
import zipfile
from pathlib import Path

import numpy as np

sys.dont_write_bytecode = True  # never write into the reference
sys.path.insert(0, str(Path(__file__).resolve().parent))
from gen_golden import _import_reference  # noqa: E402

OUT = Path(__file__).resolve().parent
NAN_SHARE_CAP = 0.25  # a non-finite case whose outputs are mostly NaN compares little

FLOATS = {"f16": np.float16, "f32": np.float32, "f64": np.float64}
DT = dict(FLOATS, i64=np.int64, i32=np.int32, u8=np.uint8, bool=np.bool_)
SMALL = [(3, 5), (1,), (1, 1), (11,)]
WIDE = [(5, 7), (1,), (1, 1), (33,)]  # the non-finite cases: enough elements for a steady NaN share
SC_SHAPES = [(2, 3), (1,), (1, 1), (5,)]
KS_FEDAVG = (1, 2, 7, 8, 9, 127, 128, 129, 130, 257)
KS_INT = (1, 2, 8, 9, 128, 129)  # int64 / int32 / uint8: trimmed first, for the size rule
KS_SCAFFOLD = (1, 7, 8, 127, 128, 129, 257)
TRIPLES = [("f16", "f16", "f16"), ("f16", "f64", "f64"), ("f16", "f16", "f32"), ("f32", "f32", "f32"),
           ("f64", "f64", "f64")]
LRS = (1, 0.7, 0)


def save_npz(path: Path, arrays: dict) -> None:
    """``np.savez_compressed`` with fixed member timestamps (NumPy stamps the wall clock)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def put_layers(arrays: dict, key: str, role: str, rows) -> None:
    """``rows``: one list of layers, or one per client (a list of lists)."""
    per_client = isinstance(rows[0], (list, tuple))
    rows = rows if per_client else [rows]
    dts = {np.asarray(a).dtype for r in rows for a in r}
    if len(dts) == 1:  # one member: rows = clients, the raveled layers end to end
        flat = np.stack([np.concatenate([np.asarray(a).reshape(-1) for a in r]) for r in rows])
        arrays[f"{key}/{role}"] = flat if per_client else flat[0]
        return
    for k, r in enumerate(rows):
        pre = f"{key}/k{k}/{role}" if per_client else f"{key}/{role}"
        if len({np.asarray(a).dtype for a in r}) == 1:
            arrays[pre] = np.concatenate([np.asarray(a).reshape(-1) for a in r])
        else:
            for li, a in enumerate(r):
                arrays[f"{pre}{li}"] = np.asarray(a)


def values(rng, shape, kind: str, coarse: bool = False) -> np.ndarray:
    """Random layer of ``kind``: normal draws scaled per layer by 10^[-2, 2]; ``coarse`` float32 /
    float64 values are float16-representable (compressible inputs, see the module docstring)."""
    scale = 10.0 ** rng.integers(-2, 3)
    if kind in FLOATS:
        x = rng.standard_normal(shape) * scale
        if coarse:  # fp16-representable; fp16 itself keeps 8 significant bits
            x = x.astype(np.float16)
            if kind == "f16":
                x = (x.view(np.uint16) & np.uint16(0xFFF8)).view(np.float16)
        return np.ascontiguousarray(x.astype(FLOATS[kind]))
    if kind == "bool":
        return rng.random(shape) < 0.5
    if kind == "u8":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    x = np.rint(rng.standard_normal(shape) * scale * 10)
    if kind == "i64" and len(shape) == 1 and shape[0] > 1:  # past 2^53: the cast to float64 rounds
        x = x * 2.0 ** 50 + np.rint(rng.standard_normal(shape) * 1000)
        return np.array([int(v) for v in x], dtype=np.int64) | 1
    return x.astype(DT[kind])


def specials(kind: str) -> np.ndarray:
    f = np.finfo(FLOATS[kind])
    t = FLOATS[kind]
    return np.array([np.nan, np.inf, -np.inf, f.max, -f.max, f.tiny, t(f.tiny) / t(4), 0.0, -0.0,
                     f.smallest_subnormal], dtype=t)


def with_specials(rng, x: np.ndarray, kind: str, share: float = 0.05) -> np.ndarray:
    sp = specials(kind)
    hit = rng.random(x.shape) < share
    return np.where(hit, sp[rng.integers(0, sp.size, x.shape)], x).astype(x.dtype)


def nan_share(outs) -> float:
    n = sum(int(np.asarray(o).size) for o in outs)
    return float(sum(int(np.isnan(o).sum()) for o in outs) / n)


def check(case: dict, outs) -> None:
    """The generator's own conditions on the reference's outputs."""
    if case["finite"]:
        assert all(np.isfinite(o).all() for o in outs), (case["key"], "finite case with NaN/inf output")
    else:
        case["nan_share"] = nan_share(outs)
        case["inf_share"] = float(sum(int(np.isinf(o).sum()) for o in outs) / sum(o.size for o in outs))
        assert case["nan_share"] <= NAN_SHARE_CAP, (case["key"], case["nan_share"])


def main():
    FedAvg, Scaffold, FedAvgSharedState, ScaffoldSharedState, DummyAlgo = _import_reference()
    meta = {"numpy": np.__version__, "reference": "Substra/substrafl v1.0.0 @ 2024-10-16", "cases": [],
            "nan_share_cap": NAN_SHARE_CAP}
    arrays = {}
    fedavg = FedAvg(algo=DummyAlgo())

    def counts(K, seed):
        return [int(v) for v in np.random.default_rng(seed).integers(1, 5000, K)]

    def add_fedavg(kind, clients, n_samples, finite=True, **info):
        """``clients[k][li]`` arrays; ``n_samples`` as handed to the reference's schema."""
        key = f"fedavg_{len([c for c in meta['cases'] if c['strategy'] == 'fedavg']):03d}"
        K, L = len(clients), len(clients[0])
        states = [FedAvgSharedState(n_samples=n, parameters_update=list(c)) for n, c in zip(n_samples, clients)]
        res = fedavg.avg_shared_states(shared_states=states, _skip=True).avg_parameters_update
        arrays[f"{key}/n_samples"] = np.array([int(s.n_samples) for s in states], dtype=np.int64)
        put_layers(arrays, key, "x", clients)
        put_layers(arrays, key, "out", res)
        assert [o.shape for o in res] == [a.shape for a in clients[0]], key
        case = dict(info, key=key, strategy="fedavg", kind=kind, K=K, layers=L, finite=finite,
                    shapes=[list(a.shape) for a in clients[0]],
                    dtypes=sorted({str(a.dtype) for c in clients for a in c}),
                    out_dtypes=[str(o.dtype) for o in res])
        if any(isinstance(n, bool) for n in n_samples):
            case["n_samples_as_given"] = list(n_samples)  # JSON keeps true apart from 1
        check(case, res)
        meta["cases"].append(case)

    def uniform(rng, K, shapes, kind, coarse=False):
        return [[values(rng, s, kind, coarse) for s in shapes] for _ in range(K)]

    # ---- FedAvg: one dtype per case ---------------------------------------------------
    for di, kind in enumerate(("f16", "f64", "i64", "i32", "u8", "bool")):
        for K in (KS_INT if kind in ("i64", "i32", "u8") else KS_FEDAVG):
            rng = np.random.default_rng(5000 + 100 * di + K)
            add_fedavg("table", uniform(rng, K, SMALL, kind, coarse=K >= 127), counts(K, 17 + K), dtype=kind)
    # kernel edges: a long ragged layer (no multiple of any vector width, several workgroup tiles)
    # between two numel == 1 layers
    for kind in ("f16", "f64"):
        for K, long in ((2, 20011 if kind == "f16" else 6151), (8, 4099)):
            rng = np.random.default_rng(6000 + K + (kind == "f64"))
            add_fedavg("edge", uniform(rng, K, [(1,), (long,), (1, 1)], kind, coarse=True), counts(K, 23 + K),
                       dtype=kind)
    # bf16-representable float32 past the existing goldens' K = 128
    for K in (129, 257):
        rng = np.random.default_rng(6100 + K)
        cl = [[(a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32) for a in c]
              for c in uniform(rng, K, SMALL, "f32")]
        add_fedavg("bf16", cl, counts(K, 29 + K), dtype="f32")
    # mixed dtypes: one layer that differs between clients; layers of different dtypes in one state
    for oi, other in enumerate(("f64", "f16", "i64")):
        rng = np.random.default_rng(6200 + oi)
        K = 5
        cl = [[values(rng, s, other if k in (1, 3) else "f32") for s in SMALL] for k in range(K)]
        add_fedavg("mixed-clients", cl, counts(K, 31 + oi), other=other)
    for K in (3, 9):
        rng = np.random.default_rng(6300 + K)
        kinds = ("f16", "f32", "f64", "i64", "bool", "u8", "i32", "f16")
        shapes = SMALL + SMALL
        cl = [[values(rng, s, kd) for s, kd in zip(shapes, kinds)] for _ in range(K)]
        add_fedavg("mixed-layers", cl, counts(K, 37 + K), layer_kinds=list(kinds))
    # weights: zero-sample clients, True, counts past 2^53, a negative entry
    for kind in ("f16", "f64"):
        rng = np.random.default_rng(6400 + (kind == "f64"))
        ns = counts(5, 41)
        ns[0] = ns[3] = 0
        add_fedavg("zero-weight", uniform(rng, 5, SMALL, kind), ns, dtype=kind)
        add_fedavg("true-weight", uniform(rng, 2, SMALL, kind), [True, 3], dtype=kind)
        add_fedavg("huge-counts", uniform(rng, 3, SMALL, kind), [2 ** 53 + 1, 2 ** 60 + 12345, 2 ** 53 + 3], dtype=kind)
    add_fedavg("huge-counts", uniform(np.random.default_rng(6410), 3, SMALL, "f32"),
               [2 ** 53 + 1, 2 ** 60 + 12345, 2 ** 53 + 3], dtype="f32")
    for kind in ("f16", "f64"):
        for ns in ([10, -9], [10, -9, 5, -5]):
            rng = np.random.default_rng(6500 + len(ns) + (kind == "f64"))
            cl = uniform(rng, len(ns), SMALL, kind)
            for c in cl:  # every 4th element large: its fp16 product with 10 or -9 overflows
                for a in c:
                    a.reshape(-1)[::4] = (rng.standard_normal(a.reshape(-1)[::4].shape) * 8e3).astype(a.dtype)
            add_fedavg("negative-weight", cl, ns, finite=kind != "f16", dtype=kind)
    # non-finite values: 5 % of each client's elements
    for kind in FLOATS:
        for K in (2, 7, 9, 33):
            rng = np.random.default_rng(6600 + K + 50 * list(FLOATS).index(kind))
            cl = [[with_specials(rng, a, kind) for a in c] for c in uniform(rng, K, WIDE, kind)]
            add_fedavg("nonfinite", cl, counts(K, 43 + K), finite=False, dtype=kind)
    for kind in ("f16", "f64"):  # a column of -0.0 sums to +0.0 (the reduction's identity)
        cl = [[np.full(s, -0.0, FLOATS[kind]) for s in SMALL] for _ in range(3)]
        add_fedavg("negzero", cl, counts(3, 47), dtype=kind)

    # ---- Scaffold -----------------------------------------------------------------------
    errors = {}

    def add_scaffold(kind, triple, pu, cv, cs, n_samples, lr, finite=True, expect_error=False, **info):
        """``cs``: one c (shared by every client, as a simulation hands it out) or one per client."""
        key = f"scaffold_{len([c for c in meta['cases'] if c['strategy'] == 'scaffold']):03d}"
        K, L = len(pu), len(pu[0])
        per_client = isinstance(cs[0], list)
        states = [ScaffoldSharedState(parameters_update=pu[k], control_variate_update=cv[k], n_samples=n_samples[k],
                                      server_control_variate=cs[k] if per_client else cs) for k in range(K)]
        case = dict(info, key=key, strategy="scaffold", kind=kind, triple=list(triple), K=K, layers=L, lr=lr,
                    lr_is_int=isinstance(lr, int), c_per_client=per_client, finite=finite, error=None,
                    shapes=[list(a.shape) for a in pu[0]])
        try:
            res = Scaffold(algo=DummyAlgo(), aggregation_lr=lr).avg_shared_states(shared_states=states, _skip=True)
        except Exception as e:  # noqa: BLE001 - the error's name is the recorded result
            assert expect_error, (key, e)
            case["error"] = errors[key] = type(e).__name__
            res = None
        arrays[f"{key}/n_samples"] = np.array(n_samples, dtype=np.int64)
        put_layers(arrays, key, "pu", pu)
        put_layers(arrays, key, "cv", cv)
        put_layers(arrays, key, "c", cs)
        if res is not None:
            put_layers(arrays, key, "avg", res.avg_parameters_update)
            put_layers(arrays, key, "newc", res.server_control_variate)
            assert [o.shape for o in res.avg_parameters_update + res.server_control_variate] == \
                [a.shape for a in pu[0]] * 2, key
            assert not expect_error, key
            case["out_dtypes"] = sorted({str(a.dtype) for a in res.avg_parameters_update + res.server_control_variate})
            check(case, res.avg_parameters_update + res.server_control_variate)
        meta["cases"].append(case)

    for ti, triple in enumerate(TRIPLES):
        for ki, K in enumerate(KS_SCAFFOLD):
            rng = np.random.default_rng(7000 + 100 * ti + K)
            d, v, s = triple
            add_scaffold("table", triple, uniform(rng, K, SC_SHAPES, d, K >= 127), uniform(rng, K, SC_SHAPES, v, K >= 127),
                         uniform(rng, 1, SC_SHAPES, s)[0], counts(K, 53 + K), LRS[(ti + ki) % 3])
    # a layer long enough that the multi-device engine gives two shards two sub-ranges each (fp64),
    # and that the 2-byte bucket kernel walks whole workgroup steps and a tail (fp16 deltas)
    edge = [(1,), (1537,), (1, 1)]
    for ti, triple in enumerate((("f64", "f64", "f64"), ("f16", "f64", "f64"))):
        rng = np.random.default_rng(7500 + ti)
        d, v, s = triple
        add_scaffold("edge", triple, uniform(rng, 2, edge, d, True), uniform(rng, 2, edge, v, True),
                     uniform(rng, 1, edge, s, True)[0], counts(2, 57), 0.7)
    for kind in FLOATS:  # non-finite: lr = 0 meets infinite sums (0 * inf is NaN), and lr = 0.7
        for lr in (0, 0.7):
            rng = np.random.default_rng(7600 + list(FLOATS).index(kind))
            sp = lambda rows: [[with_specials(rng, a, kind, 0.04) for a in r] for r in rows]  # noqa: E731
            add_scaffold("nonfinite", (kind,) * 3, sp(uniform(rng, 6, SC_SHAPES, kind)), sp(uniform(rng, 6, SC_SHAPES, kind)),
                         sp(uniform(rng, 1, SC_SHAPES, kind))[0], counts(6, 59), lr, finite=False)
    for kind in ("f16", "f64"):
        # c copies that differ from client 0's only by the sign of a zero and by NaN against NaN
        # (assert_array_equal accepts both), then one that differs by value (it raises)
        rng = np.random.default_rng(7700 + (kind == "f64"))
        K = 4
        pu, cv = uniform(rng, K, SC_SHAPES, kind), uniform(rng, K, SC_SHAPES, kind)
        c0 = uniform(rng, 1, SC_SHAPES, kind)[0]
        c0[0][0, 0], c0[3][2], c0[1][0] = 0.0, np.nan, -0.0
        other = [a.copy() for a in c0]
        other[0][0, 0], other[1][0] = -0.0, 0.0
        other[3][2] = -np.nan
        add_scaffold("c-equal-by-value", (kind,) * 3, pu, cv, [c0, other, [a.copy() for a in c0], other],
                     counts(K, 61), 0.7, finite=False)
        wrong = [a.copy() for a in c0]
        wrong[3][4] = wrong[3][4] * 2 + 1
        add_scaffold("c-mismatch", (kind,) * 3, pu, cv, [c0, c0, wrong, c0], counts(K, 61), 0.7, expect_error=True)
    meta["errors"] = errors

    summary = {}
    for c in meta["cases"]:
        tag = c["strategy"] + "/" + c["kind"]
        summary[tag] = summary.get(tag, 0) + 1
    meta["counts"] = summary
    save_npz(OUT / "golden_dtypes.npz", arrays)
    (OUT / "golden_dtypes_meta.json").write_text(json.dumps(meta, indent=1, sort_keys=True) + "\n")
    raw = sum(np.asarray(v).nbytes for v in arrays.values())
    size = (OUT / "golden_dtypes.npz").stat().st_size
    limit = min(1 << 20, (OUT / "golden_aggregation.npz").stat().st_size)
    print(f"wrote {len(arrays)} arrays, {len(meta['cases'])} cases: {raw / 1e6:.2f} MB raw, {size / 1e6:.3f} MB compressed "
          f"(limit {limit / 1e6:.3f} MB)\n{json.dumps(summary, indent=1, sort_keys=True)}\nerrors={errors}")
    assert size <= limit, "golden_dtypes.npz is over the size rule: trim K values of int64 / int32 first"


if __name__ == "__main__":
    main()
