"""The MXFP8 quantiser with error feedback on the GPU (``libfedagg_mxef.so``, include/fedagg_mxef.h):
codes, scales and the new residual, every comparison bit for bit against the NumPy restatement

    r = fl32(x + res);  (c, s) = wire.float32_to_mxfp8(r);  d = wire.mxfp8_to_float32(c, s)
    res' = +0.0 where the block has s == 255 or d is not finite, else r - d

(``res'`` is never NaN, so plain bit equality covers it)."""

from __future__ import annotations

import copy
import functools
import types

import numpy as np
import pytest
import torch  # before the native libraries: one HIP runtime in the process

from oracle import fedavg_reference_structure
from substrafl_amd import _native, _native_mxef, wire

pytestmark = pytest.mark.gpu

GUARD, SENT8, SENT32 = 64, 0xA5, 0x7FA5A5A5
LANE, TILE, SECOND = 8, 2048, 2048 * 2048  # asserted against fedagg_mxef_blocking by test_geometry
M_SIZES = [1, LANE - 1, LANE, LANE + 1, 31, 32, 33, 511, 512, 513, TILE - 1, TILE, TILE + 1, 2 * TILE + 17,
           SECOND + 2 * TILE + 17]  # the last: a second step of both walks' loops
FLT_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def ef():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    yield _native_mxef.load()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _reference(x: np.ndarray, res: np.ndarray):
    with np.errstate(all="ignore"):
        r = (x + res).astype(np.float32)
        c, s = wire.float32_to_mxfp8(r)
        d = wire.mxfp8_to_float32(c, s)
        drop = np.repeat(s["e8m0"] == 255, 32)[: r.size] | ~np.isfinite(d)
        return c["e4m3fn"], s["e8m0"], np.where(drop, np.float32(0.0), r - d).astype(np.float32), d


def _stored(x: np.ndarray, kind: str) -> np.ndarray:
    """What the device holds for the values ``x``: fp32 bits, or bf16 bits (``x`` is bf16-exact)."""
    return x.view(np.uint32) if kind == "f32" else (x.view(np.uint32) >> 16).astype(np.uint16)


class Bufs:
    """x, the residual (in place) and the two outputs on the device; residual, codes and scales each
    between guard bands.  ``ox`` / ``ores``: elements past 16-B alignment; ``oc`` / ``os``: bytes."""

    def __init__(self, M, kind, ox=0, ores=0, oc=0, os=0):
        self.M, self.nb, self.kind, self.ox = M, -(-M // 32), kind, ox
        self.x = torch.zeros(M + ox + 8, dtype=torch.int32 if kind == "f32" else torch.int16, device="cuda")
        self.res = torch.full((GUARD + ores + M + GUARD,), SENT32, dtype=torch.int32, device="cuda")
        self.r0, self.c0 = GUARD + ores, GUARD + oc
        self.s0 = GUARD + M + GUARD + (-M % 16) + os  # 16-B aligned when os == 0
        self.out = torch.full((self.s0 + self.nb + GUARD,), SENT8, dtype=torch.uint8, device="cuda")

    def put(self, x, res):
        self.x[self.ox: self.ox + self.M] = torch.from_numpy(_stored(x, self.kind).view(f"i{self.x.element_size()}")).cuda()
        self.res.fill_(SENT32)
        self.res[self.r0: self.r0 + self.M] = torch.from_numpy(res.view(np.int32)).cuda()
        self.out.fill_(SENT8)

    def call(self, lib, stream=None):
        rc = lib.fedagg_mxef_quantize(self.x.data_ptr() + self.ox * self.x.element_size(),
                                      _native.FEDAGG_F32 if self.kind == "f32" else _native.FEDAGG_BF16, self.M,
                                      self.res.data_ptr() + 4 * self.r0, self.out.data_ptr() + self.c0,
                                      self.out.data_ptr() + self.s0, stream)
        assert rc == 0, lib.fedagg_mxef_last_error()

    def check(self, ref, what):
        torch.cuda.synchronize()
        o, r, M = self.out.cpu().numpy(), self.res.cpu().numpy().view(np.uint32), self.M
        inside = np.zeros(o.size, bool)
        inside[self.c0: self.c0 + M] = inside[self.s0: self.s0 + self.nb] = True
        assert np.all(o[~inside] == SENT8) and np.all(r[: self.r0] == SENT32) and np.all(r[self.r0 + M:] == SENT32), \
            f"{what}: a guard band was written"
        for name, got, want in (("codes", o[self.c0: self.c0 + M], ref[0]), ("scales", o[self.s0: self.s0 + self.nb], ref[1]),
                                ("residual", r[self.r0: self.r0 + M], ref[2].view(np.uint32))):
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, f"{what}: {bad.size} {name} differ, first at {bad[:5]}: {got[bad[:5]]} vs {want[bad[:5]]}"


def _run(lib, x, res, kind, what, ref=None, **offs):
    ref = ref or _reference(x, res)
    b = Bufs(x.size, kind, **offs)
    b.put(x, res)
    b.call(lib)
    b.check(ref, f"{what} {kind} {offs}")
    return ref


@functools.lru_cache(maxsize=None)
def _draw(kind):
    """One draw per kind at the largest M: magnitudes spread over e^+-8 per element, +-0 planted, and
    the residual a previous round left behind (not zeros)."""
    rng = np.random.default_rng(5 if kind == "f32" else 6)
    M = max(M_SIZES)
    x0, x = ((rng.standard_normal(M) * np.exp(rng.uniform(-8, 8, M))).astype(np.float32) for _ in range(2))
    x[3::97], x[5::101] = 0.0, -0.0
    if kind == "bf16":
        x = wire.bf16_to_float32(wire.float32_to_bf16(x))
    return x, _reference(x0, np.zeros(M, np.float32))[2]


@functools.lru_cache(maxsize=None)
def _case(kind, M):
    x, res = (a[:M].copy() for a in _draw(kind))
    return x, res, _reference(x, res)


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_geometry(ef, kind):
    assert _native_mxef.blocking() == (LANE, TILE, SECOND)
    for M in M_SIZES:
        _run(ef, *_case(kind, M)[:2], kind, f"M={M}", ref=_case(kind, M)[2])


@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("offs", [dict(ox=1), dict(ores=2), dict(ox=3, ores=3), dict(oc=1), dict(os=3), dict(oc=3, os=1)],
                         ids=str)
def test_alignment(ef, kind, offs):
    """Misaligned d_x, d_res or d_codes: the element-per-lane walk; a misaligned d_scales alone: the
    vector walk with byte stores of the scales.  The same bits either way."""
    for M in M_SIZES[-2:]:
        _run(ef, *_case(kind, M)[:2], kind, f"M={M}", ref=_case(kind, M)[2], **offs)


def test_every_scale_byte(ef):
    rng = np.random.default_rng(22)
    M = 32 * 3000 + 5
    with np.errstate(over="ignore"):
        x = (rng.standard_normal(M) * np.exp2(rng.integers(-149, 128, M // 32 + 1).repeat(32)[:M])).astype(np.float32)
    x[np.isinf(x)] = FLT_MAX
    res = (x * rng.uniform(-0.06, 0.06, M)).astype(np.float32)
    x[32 * 10 + 3], x[32 * 20 + 4], x[32 * 30 + 5], x[32 * 40 + 6] = FLT_MAX, -3.35e38, np.nan, -np.inf
    x[32 * 50 + 7], res[32 * 50 + 7] = FLT_MAX, FLT_MAX  # x + res overflows
    x[32 * 60: 32 * 61], res[32 * 60: 32 * 61] = np.where(np.arange(32) % 3, 0.0, -0.0), np.where(np.arange(32) % 2, -0.0, 0.0)
    c, s, want, d = _run(ef, x, res, "f32", "every exponent")
    finite_block = np.repeat(s != 255, 32)[:M]
    assert np.isinf(d[finite_block]).sum() >= 1 and set(s[[30, 40, 50]]) == {255} and s[60] == 127
    assert set(s) == set(range(248)) | {255}  # every scale byte the rule can produce
    assert not want.view(np.uint32)[~finite_block | ~np.isfinite(d)].any()  # +0.0 bit for bit
    xb = wire.bf16_to_float32(wire.float32_to_bf16(np.nan_to_num(x, nan=1.0, posinf=FLT_MAX, neginf=-FLT_MAX)))
    _run(ef, xb, np.nan_to_num(res, posinf=0.0), "bf16", "every exponent")


def test_exhaustive_encode(ef):
    """Each of the 254 non-NaN codes under six scales: the decoded value and the midpoints to its two
    neighbours (the ties; above 448 the 464 bump's), res = 0.  An anchor of 448 * 2^(s-127) holds each
    block to the scale s (none exists for s = 254: its values are clipped to FLT_MAX).  The test that
    decides whether the hardware fp8 convert may replace the integer encode."""
    v = wire.mxfp8_to_float32(np.arange(127, dtype=np.uint8).view(wire.E4M3), np.full(4, 127, np.uint8).view(wire.E8M0))
    v = np.concatenate([v.astype(np.float64), [480.0]])
    mag = np.concatenate([v[:127], (v[:127] + np.concatenate([[0.0], v[:126]])) / 2, (v[:127] + v[1:]) / 2])
    blocks = []
    for s in (0, 1, 126, 127, 128, 254):
        exact = np.ldexp(np.concatenate([mag, -mag]), s - 127).clip(-FLT_MAX, FLT_MAX)
        vals = exact.astype(np.float32)
        assert np.all(vals == exact)  # every value and tie is an fp32 number
        vals = np.concatenate([vals, np.zeros(-vals.size % 31, np.float32)]).reshape(-1, 31)
        anchor = np.full((vals.shape[0], 1), np.ldexp(448.0, s - 127) if s < 254 else 0.0, np.float32)
        blocks.append(np.concatenate([anchor, vals], axis=1).reshape(-1))
    x = np.concatenate(blocks)
    c, s, _, _ = _run(ef, x, np.zeros(x.size, np.float32), "f32", "exhaustive encode")
    assert {0, 1, 126, 127, 128} <= set(s) and len(set(c)) == 254  # the anchors held, every code was produced


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_rounds(ef, kind):
    """16 calls on the same buffers, a fresh x each round: every round is the NumPy recurrence, and
    the transmitted sum telescopes: |sum d + res_T - sum x| <= sum 2^-24 |r_t| per element (fp64)."""
    rng = np.random.default_rng(31 if kind == "f32" else 32)
    M = 2 * TILE + 17
    b = Bufs(M, kind)
    res = np.zeros(M, np.float32)
    sum_x, sum_d, bound = np.zeros(M), np.zeros(M), np.zeros(M)
    for t in range(16):
        x = (rng.standard_normal(M) * np.exp(rng.uniform(-8, 8, M)) * 1e-3).astype(np.float32)
        x = x if kind == "f32" else wire.bf16_to_float32(wire.float32_to_bf16(x))
        ref = _reference(x, res)
        if t == 0:
            b.put(x, res)
        else:  # the residual the kernel left stays where it is
            b.x[:M] = torch.from_numpy(_stored(x, kind).view(f"i{b.x.element_size()}")).cuda()
            b.out.fill_(SENT8)
        b.call(ef)
        b.check(ref, f"{kind} round {t}")
        res, d = ref[2], ref[3].astype(np.float64)
        sum_x, sum_d, bound = sum_x + x, sum_d + d, bound + 2.0 ** -24 * np.abs(d + res)  # r_t = d_t + res_t exactly
    assert np.all(np.abs(sum_d + res - sum_x) <= bound), "the telescoping bound"


def test_stream_contract(ef):
    """On a non-blocking side stream, then captured once into a graph -- nothing may run while
    capturing -- and replayed over two data sets in the same buffers: the same bits."""
    M = TILE + 37
    data = {ds: _case("f32", M) if ds == "A" else _case("bf16", M) for ds in "AB"}
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    b = Bufs(M, "f32")
    with torch.cuda.stream(stream):
        b.put(*data["A"][:2])
        b.call(ef, stream.cuda_stream)
    stream.synchronize()
    b.check(data["A"][2], "eager on the side stream")
    with torch.cuda.stream(stream):
        b.put(*data["A"][:2])
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        b.call(ef, stream.cuda_stream)
    torch.cuda.synchronize()
    assert bool((b.out == SENT8).all()), "the kernel ran during the capture"
    for ds in ("B", "A"):
        with torch.cuda.stream(stream):
            b.put(*data[ds][:2])
            graph.replay()
        b.check(data[ds][2], f"replay over data set {ds}")
    del graph


def _algo(dtype, client):
    from standin_substrafl.algorithms.pytorch import TorchFedAvgAlgo
    from standin_substrafl.index_generator import NpIndexGenerator

    from substrafl_amd.algorithms.weight_manager import model_parameters
    from substrafl_amd.integration import accelerate_algo

    torch.manual_seed(7)
    model = torch.nn.Sequential(torch.nn.Linear(6, 24), torch.nn.BatchNorm1d(24), torch.nn.ReLU(),
                                torch.nn.Linear(24, 1)).to(dtype)

    class XY(torch.utils.data.Dataset):
        def __init__(self, data_from_opener, is_inference=False):
            self.x, self.y = data_from_opener

        def __getitem__(self, i):
            return torch.from_numpy(self.x[i]).to(dtype), torch.from_numpy(self.y[i]).to(dtype)

        def __len__(self):
            return len(self.x)

    class MyAlgo(TorchFedAvgAlgo):
        def __init__(self):
            super().__init__(model=model, criterion=torch.nn.MSELoss(), optimizer=torch.optim.SGD(model.parameters(), lr=0.02),
                             index_generator=NpIndexGenerator(batch_size=32, num_updates=3, seed=11 + client),
                             dataset=XY, with_batch_norm_parameters=True, disable_gpu=False)

        def flat(self):
            return torch.cat([p.data.detach().reshape(-1) for p in model_parameters(self.model, True)()])

        def _local_train(self, train_dataset):  # the delta, recomputed beside the kernels
            before = self.flat()
            super()._local_train(train_dataset)
            self.delta = (self.flat() - before).float().cpu().numpy()

        def _get_state_to_save(self):
            return {}

        def _update_from_checkpoint(self, path):
            return torch.load(path)

    return accelerate_algo(MyAlgo, wire="mxfp8", error_feedback=True)()


def _data(n, seed):
    r = np.random.default_rng(seed)
    x = r.standard_normal((n, 6)).astype(np.float32)
    return x, (x @ r.standard_normal((6, 1))).astype(np.float32)


def _flat_bytes(state):
    pu = list(state.parameters_update)
    assert wire.is_mxfp8(pu)
    return np.concatenate([a["e4m3fn"].reshape(-1) for a in pu[:-1]]), pu[-1]["e8m0"]


@pytest.fixture()
def deterministic_training(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "enabled", False)  # the native BatchNorm kernels


def test_federation_end_to_end(ef, deterministic_training):
    """An fp32 MLP and its bf16 copy with ``error_feedback=True`` for three rounds: each export is
    the host encoder on delta + residual, the client's residual is the NumPy res', the average is
    still the oracle on the decoded states."""
    import standin_substrafl.strategies as ss

    from substrafl_amd.integration import accelerate

    algos, datasets = [_algo(torch.float32, 0), _algo(torch.bfloat16, 1)], [_data(120, 1), _data(77, 2)]
    strategy, avg = accelerate(ss.FedAvg)(algo=algos[0]), None
    for rnd in range(3):
        assert rnd or all(a._fedagg_mx_residual is None for a in algos)
        before = [np.zeros(0) if rnd == 0 else a._fedagg_mx_residual.cpu().numpy() for a in algos]
        states = [a.train(data_from_opener=d, shared_state=avg, _skip=True) for a, d in zip(algos, datasets)]
        for a, st, res in zip(algos, states, before):
            c, s, want, _ = _reference(a.delta, res if res.size else np.zeros(a.delta.size, np.float32))
            got_c, got_s = _flat_bytes(st)
            assert np.array_equal(got_c, c) and np.array_equal(got_s, s), rnd
            got = a._fedagg_mx_residual
            assert got.dtype == torch.float32 and got.device == a.model[0].weight.device
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)) and want.any(), rnd
        avg = strategy.avg_shared_states(shared_states=states, _skip=True)
        decoded = [wire.mxfp8_to_float32(list(st.parameters_update)[:-1], st.parameters_update[-1]) for st in states]
        for g, r in zip(avg.avg_parameters_update, fedavg_reference_structure(decoded, [st.n_samples for st in states])):
            assert np.array_equal(np.asarray(g).view(np.uint32), r.view(np.uint32)), rnd
    from substrafl_amd.algorithms import weight_manager as wm

    for bad in (torch.zeros(40), torch.zeros(40, dtype=torch.float64, device="cuda"), torch.zeros(41, device="cuda")):
        with pytest.raises(ValueError, match="residual"):
            wm.export_mxfp8([torch.ones(40, device="cuda")], residual=bad)
    algos[0]._fedagg_mx_residual = torch.zeros(5, device="cuda")
    with pytest.raises(ValueError, match="error_feedback: the residual holds 5 elements"):
        algos[0].train(data_from_opener=datasets[0], shared_state=avg, _skip=True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_checkpoint_round_trip(ef, deterministic_training, tmp_path, dtype):
    """``_get_state_to_save`` -> ``torch.save`` -> a second instance's ``_update_from_checkpoint``: a
    bit-equal residual, an emptied dict, and the same bytes from the next ``train``."""
    a, data = _algo(dtype, 0), _data(120, 1)
    st = a.train(data_from_opener=data, shared_state=None, _skip=True)
    state = a._get_state_to_save()
    assert set(state) == {"fedagg_mx_residual"} and state["fedagg_mx_residual"].any()
    torch.save(state, tmp_path / "state.pt")
    b = copy.deepcopy(a)  # everything but the residual travels by other means
    b._fedagg_mx_residual = None
    assert b._update_from_checkpoint(tmp_path / "state.pt") == {}
    assert b._fedagg_mx_residual is not a._fedagg_mx_residual and torch.equal(
        b._fedagg_mx_residual.view(torch.int32), a._fedagg_mx_residual.view(torch.int32))
    avg = types.SimpleNamespace(avg_parameters_update=[np.zeros(p.shape, np.float32) for p in st.parameters_update[:-1]])
    nxt = [_flat_bytes(o.train(data_from_opener=data, shared_state=avg, _skip=True)) for o in (a, b)]
    assert np.array_equal(nxt[0][0], nxt[1][0]) and np.array_equal(nxt[0][1], nxt[1][1])
    assert not np.array_equal(nxt[0][0], _flat_bytes(st)[0])
