"""libfedagg_topk.so on the GPU, bit for bit: selection and compaction against
wire.topk_error_feedback, the sparse FedAvg against the oracle's dense FedAvg on the densified rows,
at the sizes at which the kernels change path (from fedagg_topk_blocking), and two rounds end to end."""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch  # before the native libraries: one HIP runtime in the process

from oracle import fedavg_reference_structure
from substrafl_amd import _native, _native_topk, wire

pytestmark = pytest.mark.gpu
TILE, SUB, GROUP, _ = _native_topk.blocking()  # the sizes at which the kernels change path (no HIP call)


def dev(a: np.ndarray) -> torch.Tensor:
    """``a``'s bytes in a fresh device buffer (torch allocations are 256-B aligned), 16 spare bytes behind."""
    t = torch.full((a.nbytes + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    t[: a.nbytes] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8))
    return t


def select_compact(x: np.ndarray, res: np.ndarray, k: int, kind: str):
    """One step of the library on the fp32 values ``x`` (bf16-representable for ``kind`` bf16):
    (indices, value bits, res' bits, t)."""
    M, stream = x.size, int(torch.cuda.current_stream().cuda_stream)
    d_x = dev(wire.float32_to_bf16(x)) if kind == "bf16" else dev(x)
    d_res = dev(res)
    ws_bytes = _native_topk.workspace(M)[0]
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    state = torch.full((_native_topk.STATE_WORDS,), -1, dtype=torch.int32, device="cuda")
    _native_topk.select(_native.FEDAGG_BF16 if kind == "bf16" else _native.FEDAGG_F32, d_x.data_ptr(), d_res.data_ptr(), M,
                        k, ws.data_ptr(), ws_bytes, state.data_ptr(), stream)
    st = state.cpu().numpy().view(np.uint32)
    nnz = int(st[_native_topk.STATE_NNZ])
    assert nnz <= M and st[_native_topk.STATE_ERROR] == 0
    out = torch.full((8 * nnz + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    _native_topk.compact(d_res.data_ptr(), M, ws.data_ptr(), state.data_ptr(), nnz, out.data_ptr(),
                         out.data_ptr() + 4 * nnz, stream)
    torch.cuda.synchronize()
    got, r = out.cpu().numpy(), d_res.cpu().numpy()
    assert (got[8 * nnz:] == 0xEE).all() and (r[4 * M:] == 0xEE).all()  # nothing past the rows
    assert state.cpu().numpy()[_native_topk.STATE_ERROR] == 0
    return got[: 4 * nnz].view(np.uint32), got[4 * nnz: 8 * nnz].view(np.uint32), r[: 4 * M].view(np.uint32), int(st[0])


def family(name: str, M: int, rng):
    """(x, res): normal draws with a non-zero residual; small integers, so the threshold falls on a
    large tie; finite values with NaN, +-Inf and -0.0 at the tile edges."""
    if name == "normal":
        return rng.standard_normal(M).astype(np.float32), (rng.standard_normal(M) * 0.3).astype(np.float32)
    if name == "ties":
        return rng.integers(-2, 3, M).astype(np.float32), np.zeros(M, np.float32)
    x = (rng.standard_normal(M) * np.exp(rng.uniform(-4, 4, M))).astype(np.float32)
    for i, v in zip([0, 1, TILE - 2, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, M - 2, M - 1],
                    [np.nan, -0.0, np.inf, -0.0, -np.inf, np.nan, 0.0, np.inf, -0.0, -np.inf]):
        if 0 <= i < M:
            x[i] = v
    return x, np.zeros(M, np.float32)


@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["normal", "ties", "edges"])
@pytest.mark.parametrize("M", [1, 31, TILE - 1, TILE + 1, 3 * TILE + 17])
def test_select_and_compact(kind, name, M):
    rng = np.random.default_rng(M + len(name))
    x, res = family(name, M, rng)
    if kind == "bf16":
        x = wire.bf16_to_float32(wire.float32_to_bf16(x))
    for k in sorted({1, math.ceil(M / 100), M}):
        idx, val, new = wire.topk_error_feedback(x, res, k)
        g_idx, g_val, g_res, t = select_compact(x, res, k, kind)
        what = f"{kind} {name} M={M} k={k}"
        assert g_idx.size == idx.size, (what, g_idx.size, idx.size)
        assert np.array_equal(g_idx, idx["topk_idx"]), what
        assert np.array_equal(g_val, val["topk_f32"].view(np.uint32)), what
        assert np.array_equal(g_res, new.view(np.uint32)), (what, np.flatnonzero(g_res != new.view(np.uint32))[:8])
        with np.errstate(all="ignore"):
            m = (x + res).view(np.uint32) & np.uint32(0x7FFFFFFF)
        assert t == np.partition(m, M - k)[M - k], what
        if name == "ties" and M > 100 and k < M:
            assert idx.size > k, what  # the case is what it claims to be


def test_a_stale_nnz_writes_nothing_but_the_error_word():
    M = TILE + 5
    x = np.arange(M, dtype=np.float32)
    d_x, d_res = dev(x), dev(np.zeros(M, np.float32))
    ws_bytes = _native_topk.workspace(M)[0]
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    state = torch.zeros(_native_topk.STATE_WORDS, dtype=torch.int32, device="cuda")
    _native_topk.select(_native.FEDAGG_F32, d_x.data_ptr(), d_res.data_ptr(), M, 10, ws.data_ptr(), ws_bytes,
                        state.data_ptr(), 0)
    out = torch.full((8 * 9,), 0xEE, dtype=torch.uint8, device="cuda")
    _native_topk.compact(d_res.data_ptr(), M, ws.data_ptr(), state.data_ptr(), 9, out.data_ptr(), out.data_ptr() + 36, 0)
    torch.cuda.synchronize()
    st = state.cpu().numpy()
    assert st[_native_topk.STATE_NNZ] == 10 and st[_native_topk.STATE_ERROR] == 1 and bool((out == 0xEE).all())
    assert np.array_equal(d_res.cpu().numpy()[: 4 * M].view(np.float32), x)  # r, with nothing taken out yet


def sparse_rows(K: int, M: int, rng):
    """K rows over M elements: random densities, then row 0 empty, row 1 fully dense, rows 2 and 3
    on the same indices with cancelling values, and every row past 3 holding the sub-tile edges."""
    rows = []
    for k in range(K):
        n = int(rng.integers(0, max(2, min(M, 200))))
        i = np.sort(rng.choice(M, size=min(n, M), replace=False)).astype(np.uint32)
        if k >= 4:
            edges = [e for s in range(0, M, SUB) for e in (s - 1, s, s + 1) if 0 <= e < M] + [M - 1]
            i = np.union1d(i, np.array(edges, np.uint32)).astype(np.uint32)
        rows.append([i, rng.standard_normal(i.size).astype(np.float32)])
    rows[0] = [np.zeros(0, np.uint32), np.zeros(0, np.float32)]
    if K > 1:
        rows[1] = [np.arange(M, dtype=np.uint32), rng.standard_normal(M).astype(np.float32)]
    if K > 3:
        rows[3] = [rows[2][0].copy(), -rows[2][1]]
    return rows


@pytest.mark.parametrize("K", [1, GROUP - 1, GROUP, GROUP + 1, 128])
@pytest.mark.parametrize("M", [1, SUB + 1, 3 * SUB + 5])
def test_fedavg(K, M):
    rng = np.random.default_rng(1000 * K + M)
    rows = sparse_rows(K, M, rng)
    ns = [int(n) for n in rng.integers(100, 10000, K)]
    if K > 3:
        ns[3] = ns[2]  # so that rows 2 and 3 cancel exactly
    present = set(np.concatenate([r[0] for r in rows[2:]] + [np.zeros(0, np.uint32)]).tolist())
    absent = [i for i in range(M) if i not in present]
    # two numel == 1 indices: the last element, which rows 4.. hold, and one that no row but the dense one holds
    table, pw = layers_with_single(M, sorted({M - 1, absent[0] if absent else 0}))
    dense = [wire.topk_to_float32(r[0].view(wire.TOPK_IDX), r[1].view(wire.TOPK_VAL), table) for r in rows]
    ref = np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in fedavg_reference_structure(dense, ns)])

    from substrafl_amd.engine import fedavg_weights

    d_rows = [(dev(r[0]), dev(r[1])) for r in rows]
    fed_bytes = _native_topk.workspace(M, K)[1]
    ws = torch.empty(fed_bytes, dtype=torch.uint8, device="cuda")
    out = torch.full((M + 4,), float("nan"), dtype=torch.float32, device="cuda")
    _native_topk.fedavg([a.data_ptr() for a, _ in d_rows], [b.data_ptr() for _, b in d_rows], [r[0].size for r in rows],
                        fedavg_weights(ns, "f32"), M, pw, ws.data_ptr(), fed_bytes, out.data_ptr(),
                        int(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert (got[M:] == 0x7FC00000).all()  # nothing past the row
    bad = np.flatnonzero(got[:M] != ref.view(np.uint32))
    assert bad.size == 0, (K, M, bad[:8], got[bad[:8]], ref.view(np.uint32)[bad[:8]])


def layers_with_single(M: int, pw):
    """(shape table, numel == 1 indices) of M elements in layers that make the flat indices ``pw``
    numel == 1 layers; a gap of one element between them is one more such layer."""
    sizes, at = [], 0
    for p in [*pw, M]:
        sizes += [p - at] * (p > at) + [1] * (p < M)
        at = p + 1
    starts = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    return wire.mxfp4_shape_table([(n,) for n in sizes]), [int(s) for s, n in zip(starts, sizes) if n == 1]


def test_two_rounds_end_to_end(tmp_path):
    """An fp32 MLP and its bf16 copy on the top-k wire: each export is the NumPy rule on the previous
    residual, each average the oracle on the densified exports, and the residual survives a checkpoint."""
    from standin_substrafl.algorithms.pytorch import TorchFedAvgAlgo
    from standin_substrafl.index_generator import NpIndexGenerator

    from substrafl_amd import strategies
    from substrafl_amd.algorithms.weight_manager import model_parameters
    from substrafl_amd.engine import engine_for
    from substrafl_amd.integration import accelerate_algo

    def algo(dtype, client):
        torch.manual_seed(7)
        model = torch.nn.Sequential(torch.nn.Linear(6, 24), torch.nn.ReLU(), torch.nn.Linear(24, 1)).to(dtype)

        class XY(torch.utils.data.Dataset):
            def __init__(self, data_from_opener, is_inference=False):
                self.x, self.y = data_from_opener

            def __getitem__(self, i):
                return torch.from_numpy(self.x[i]).to(dtype), torch.from_numpy(self.y[i]).to(dtype)

            def __len__(self):
                return len(self.x)

        class MyAlgo(TorchFedAvgAlgo):
            def __init__(self):
                super().__init__(model=model, criterion=torch.nn.MSELoss(),
                                 optimizer=torch.optim.SGD(model.parameters(), lr=0.02),
                                 index_generator=NpIndexGenerator(batch_size=32, num_updates=3, seed=11 + client),
                                 dataset=XY, disable_gpu=False)

            def flat(self):
                return torch.cat([p.data.detach().reshape(-1) for p in model_parameters(self.model, False)()])

            def _local_train(self, train_dataset):  # the delta, recomputed beside the kernels
                before = self.flat()
                super()._local_train(train_dataset)
                self.delta = (self.flat() - before).float().cpu().numpy()

            def _get_state_to_save(self):
                return {}

            def _update_from_checkpoint(self, path):
                return torch.load(path)

        return accelerate_algo(MyAlgo, wire="topk", error_feedback=True, density=0.05)()

    rng = np.random.default_rng(3)
    datasets = [(rng.standard_normal((n, 6)).astype(np.float32), rng.standard_normal((n, 1)).astype(np.float32))
                for n in (120, 77)]
    algos, avg = [algo(torch.float32, 0), algo(torch.bfloat16, 1)], None
    M = 6 * 24 + 24 + 24 + 1
    k = math.ceil(0.05 * M)
    strategy = strategies.FedAvg(algo=algos[0], device=0)
    for rnd in range(2):
        before = [np.zeros(M, np.float32) if rnd == 0 else a._fedagg_mx_residual.cpu().numpy() for a in algos]
        states = [a.train(data_from_opener=d, shared_state=avg, _skip=True) for a, d in zip(algos, datasets)]
        for a, st, res in zip(algos, states, before):
            pu = list(st.parameters_update)
            idx, val, want = wire.topk_error_feedback(a.delta, res, k)
            assert wire.is_topk(pu) and wire.topk_check(pu) == M and len({id(p._bucket) for p in pu}) == 1
            assert wire.mxfp4_layer_shapes(pu[2]) == [(24, 6), (24,), (1, 24), (1,)] and idx.size >= k
            assert np.array_equal(pu[0]["topk_idx"], idx["topk_idx"]), rnd
            assert np.array_equal(pu[1]["topk_f32"].view(np.uint32), val["topk_f32"].view(np.uint32)), rnd
            assert np.array_equal(a._fedagg_mx_residual.cpu().numpy().view(np.uint32), want.view(np.uint32)) and want.any()
        avg = strategy.avg_shared_states(shared_states=states, _skip=True)
        assert engine_for(0).last_timing["staging"] == "topk-host-rows"
        dense = [wire.topk_to_float32(*st.parameters_update) for st in states]
        ref = fedavg_reference_structure(dense, [st.n_samples for st in states])
        assert len(avg.avg_parameters_update) == len(ref) == 4
        for g, r in zip(avg.avg_parameters_update, ref):
            assert g.dtype == np.float32 and g.shape == r.shape
            assert np.array_equal(np.asarray(g).view(np.uint32), r.view(np.uint32)), rnd
    assert any(np.any(np.asarray(g) != 0) for g in avg.avg_parameters_update)

    a = algos[0]
    state = a._get_state_to_save()
    assert set(state) == {"fedagg_mx_residual"}
    torch.save(state, tmp_path / "state.pt")
    kept, a._fedagg_mx_residual = a._fedagg_mx_residual.clone(), None
    assert a._update_from_checkpoint(tmp_path / "state.pt") == {}
    assert torch.equal(a._fedagg_mx_residual.view(torch.int32), kept.view(torch.int32))
