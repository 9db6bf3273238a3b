"""The two promises ``include/fedagg.h`` opens with, pinned for every entry point that takes a
``void* stream`` (``tests/stream_contract_cases.py`` is the table, ``test_stream_contract_table.py``
keeps it in step with the header):

  * "Every call is asynchronous on that stream": each case runs on ONE non-blocking side stream and
    only that stream is synchronised, so a launch that slipped onto another stream is unordered
    against the uploads before it and the read-back after it;
  * "nothing is allocated and every call is capturable into a hipGraph": the same calls are captured
    (nothing may run while capturing), every host array that was passed is then overwritten with
    garbage and released, and the graph is replayed over new data written into the same buffers.

A case: upload data set A on the side stream, call, synchronise that stream, compare; refill the
outputs with the sentinel, capture the same call(s) with fresh host arrays, check that the outputs
are still the sentinel; trash the host arrays; replay over data set B, then over A again.  Every
output element is compared bit for bit (NaN-ness only where the reference is NaN) with a reference
that shares no code with the kernels -- NumPy, the oracle, or torch eager ops on the CPU -- and
every buffer sits between guard bands of the sentinel.  A captured graph is a single chain on the
side stream; no further stream is created and no environment variable is set.

The second half pins the client-count paths of ``fedagg_equal_count_*`` (the remainder loop after
the groups of four copies, the seam between two chunks of 128 copies) on the legacy stream."""

from __future__ import annotations

import ctypes
import gc

import numpy as np
import pytest
import torch  # before libfedagg: one HIP runtime in the process

from oracle import numpy_pairwise_sum
from substrafl_amd import _native
from substrafl_amd.engine import fedavg_weights, tiled_elems, tiled_index
from test_product_dispatch_gpu import SENTINEL, _np_sequential, _oracle_layers, _sc_reference
from test_scaffold16_kernel_gpu import reference as _rows_reference

pytestmark = pytest.mark.gpu

GUARD = 64  # elements before and after every device buffer (64 x 2 B keeps 16-B alignment)
M0 = 4096 + 37  # whole 16-B vectors, a partial workgroup step and a scalar tail for every kind
LR = 0.7
NB = {"f16": 2, "bf16": 2, "f32": 4, "f64": 8, "i64": 8, "raw4": 4, "raw8": 8}
L_OF = {"f32": 4, "bf16": 8, "f16": 8, "f64": 2}
OUT_OF = {"f32": "f32", "bf16": "f32", "f16": "f16", "f64": "f64"}  # FedAvg output kind per bucket kind
NP_OF = {"f16": np.float16, "f32": np.float32, "f64": np.float64}
UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}
SINT = {2: np.int16, 4: np.int32, 8: np.int64}
TINT = {2: torch.int16, 4: torch.int32, 8: torch.int64}
CODE = {"f16": _native.FEDAGG_F16, "bf16": _native.FEDAGG_BF16, "f32": _native.FEDAGG_F32, "f64": _native.FEDAGG_F64,
        "i64": 6}
TILES = [("f32", _native.FEDAGG_TILE_VECTORS_F32), ("f32", _native.FEDAGG_TILE_VECTORS_F32_FEW),
         ("bf16", _native.FEDAGG_TILE_VECTORS_BF16)]


# =============================================================================================
# device buffers, host argument arrays, comparison
# =============================================================================================
class Dev:
    """``n`` elements of ``nb`` bytes on the device between two guard bands, handled as bit patterns."""

    def __init__(self, n: int, nb: int):
        self.n, self.nb = int(n), nb
        self.t = torch.empty(GUARD + self.n + GUARD, dtype=TINT[nb], device="cuda")
        self.t.fill_(SENTINEL[nb])
        self.body = self.t[GUARD: GUARD + self.n]
        self.ptr = self.t.data_ptr() + GUARD * nb
        assert self.ptr % 16 == 0

    def fill(self):
        self.body.fill_(SENTINEL[self.nb])

    def put(self, a: np.ndarray):
        a = np.ascontiguousarray(a).reshape(-1)
        assert a.dtype.itemsize == self.nb and a.size == self.n, (a.dtype, a.size, self.nb, self.n)
        self.body.copy_(torch.from_numpy(a.view(SINT[self.nb])))

    def get(self) -> np.ndarray:
        return self.body.cpu().numpy().view(UINT[self.nb])

    def guards_intact(self) -> bool:
        g = self.t.cpu().numpy().view(UINT[self.nb])
        return bool(np.all(g[:GUARD] == SENTINEL[self.nb]) and np.all(g[GUARD + self.n:] == SENTINEL[self.nb]))


class Host:
    """The host argument arrays of one call sequence, built fresh for it and remembered by role so
    that they can be overwritten with garbage once the calls have returned."""

    def __init__(self):
        self.arrays = []

    def _keep(self, role, arr):
        self.arrays.append((role, arr))
        return arr

    def ptrs(self, ps):
        return self._keep("ptr", _native.ptr_array([int(p) for p in ps]))

    def weights(self, w, kind):
        """FedAvg weights in the product type: float, double, or fp16 bit patterns."""
        if kind == "f16":
            bits = np.asarray(w, np.float16).view(np.uint16)
            return self._keep("w16", (ctypes.c_uint16 * len(w))(*[int(v) for v in bits]))
        ct = ctypes.c_double if kind == "f64" else ctypes.c_float
        return self._keep("w", (ct * len(w))(*[float(v) for v in w]))

    def doubles(self, v):
        return self._keep("w", (ctypes.c_double * len(v))(*[float(x) for x in v]))

    def idx(self, idx):
        return self._keep("idx", (ctypes.c_uint64 * max(1, len(idx)))(*[int(i) for i in idx]))

    def numel(self, numel):
        return self._keep("numel", (ctypes.c_uint64 * len(numel))(*[int(n) for n in numel]))

    def kinds(self, kinds):
        return self._keep("kinds", (ctypes.c_int * len(kinds))(*[int(k) for k in kinds]))

    def trash(self):
        """weights -> NaN, indices -> 2^63, pointer tables -> 0, numel -> 0, kinds -> 99; then drop them."""
        garbage = {"w": float("nan"), "w16": 0x7E00, "idx": 1 << 63, "ptr": 0, "numel": 0, "kinds": 99}
        for role, arr in self.arrays:
            for i in range(len(arr)):
                arr[i] = garbage[role]
        self.arrays = []


def _bits(a) -> np.ndarray:
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view(UINT[a.dtype.itemsize])


def _nan_bits(b: np.ndarray, kind: str) -> np.ndarray:
    if kind == "f16":
        return (b & 0x7FFF) > 0x7C00
    if kind == "bf16":
        return (b & 0x7FFF) > 0x7F80
    if kind == "f32":
        return (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    if kind == "f64":
        return (b & np.uint64(0x7FFFFFFFFFFFFFFF)) > np.uint64(0x7FF0000000000000)
    return np.zeros(b.shape, bool)  # integers and raw words


def _compare(dev: Dev, kind: str, ref, at, what: str):
    """``dev`` against ``ref`` bit for bit (NaN-ness where the reference is NaN).  ``at``: the only
    elements the entry writes; every other element must still be the sentinel."""
    assert NB[kind] == dev.nb, (kind, dev.nb)
    got, want = dev.get(), _bits(ref)
    if at is not None:
        at = np.asarray(at, np.int64)
        rest = np.ones(dev.n, bool)
        rest[at] = False
        assert np.all(got[rest] == SENTINEL[dev.nb]), f"{what}: elements the entry does not own were written"
        got = got[at]
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = _nan_bits(want, kind)
    assert np.array_equal(_nan_bits(got, kind), nan), f"{what}: NaN positions differ"
    bad = np.flatnonzero((got != want) & ~nan)
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} elements differ; first at {bad[:6]}: got "
                           f"{[hex(int(v)) for v in got[bad[:6]]]} reference {[hex(int(v)) for v in want[bad[:6]]]}")


class Job:
    """One case: ``ins`` [(Dev, {"A": bits, "B": bits})] are written before every run, ``outs`` are
    refilled with the sentinel; ``inouts`` are the inputs the calls modify in place; ``call(stream)``
    makes the calls with fresh host arrays and returns the Host; ``expect(ds)`` lists
    (Dev, kind, reference, at)."""

    def __init__(self):
        self.ins, self.outs, self.inouts, self.scratch = [], [], [], []
        self.call = self.expect = None
        self._expected = {}

    def input(self, dev, a, b, inout=False):
        self.ins.append((dev, {"A": np.ascontiguousarray(a).reshape(-1), "B": np.ascontiguousarray(b).reshape(-1)}))
        if inout:
            self.inouts.append(self.ins[-1])
        return dev

    def output(self, dev):
        self.outs.append(dev)
        return dev

    def expected(self, ds):
        if ds not in self._expected:
            self._expected[ds] = self.expect(ds)
        return self._expected[ds]

    def devs(self):
        return [d for d, _ in self.ins] + self.outs + self.scratch


@pytest.fixture(scope="module")
def side_stream():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _native.load()
    s = torch.cuda.Stream()  # torch creates its streams non-blocking; the one stream of this file
    assert s.cuda_stream != 0
    yield s
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _ok(lib, rc):
    assert rc == 0, lib.fedagg_last_error()


def _run_case(build, stream, cid):
    lib = _native.load()
    sp = stream.cuda_stream

    def prepare(job, ds):
        for dev, data in job.ins:
            dev.put(data[ds])
        for dev in job.outs:
            dev.fill()

    def check(job, ds, stage):
        for n, (dev, kind, ref, at) in enumerate(job.expected(ds)):
            _compare(dev, kind, ref, at, f"{cid} output {n}, {stage}")
        assert all(d.guards_intact() for d in job.devs()), f"{cid}, {stage}: a guard band was written"

    # eager on the side stream, only that stream synchronised (also loads the code object)
    with torch.cuda.stream(stream):
        job = build(lib)
        prepare(job, "A")
        host = job.call(lib, sp)
    stream.synchronize()
    check(job, "A", "eager on the side stream")
    host.trash()

    # capture: nothing may run
    with torch.cuda.stream(stream):
        prepare(job, "A")
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        host = job.call(lib, sp)
    torch.cuda.synchronize()
    for dev in job.outs:
        assert bool(np.all(dev.get() == SENTINEL[dev.nb])), f"{cid}: a kernel ran during the capture"
    for dev, data in job.inouts:
        assert np.array_equal(dev.get(), _bits(data["A"])), f"{cid}: a kernel ran during the capture (in-place operand)"
    host.trash()
    del host
    gc.collect()

    # replay over new data in the same buffers, then over the first data again
    for ds in ("B", "A"):
        with torch.cuda.stream(stream):
            prepare(job, ds)
            graph.replay()
        torch.cuda.synchronize()
        check(job, ds, f"replay over data set {ds}")
    del graph


# =============================================================================================
# data
# =============================================================================================
def _rng(tag: str, ds: str):
    return np.random.default_rng([sum(map(ord, tag)), len(tag), ord(ds)])


def _draw(rng, kind: str, shape) -> np.ndarray:
    """Stored values of ``kind``: float16 / float32 / float64 arrays, bf16 as uint16 bit patterns."""
    x = rng.standard_normal(shape)
    if kind == "bf16":
        return (x.astype(np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    return x.astype(NP_OF[kind])


def _upcast(a: np.ndarray, kind: str) -> np.ndarray:
    """What the reference computes on (bf16: its exact fp32 upcast)."""
    return (a.astype(np.uint32) << np.uint32(16)).view(np.float32) if kind == "bf16" else a


def _samples(K: int):
    return [int(v) for v in np.random.default_rng(1000 + K).integers(100, 10000, K)]


def _sc_weights(K: int) -> np.ndarray:
    n = np.random.default_rng(2000 + K).integers(1, 5000, K)
    return (n / np.sum(n)).astype(np.float64)


def _idx(M: int, P: int):
    """P numel == 1 indices >= 3 apart: element 0, inside the vectors, M - 1 in the scalar tail."""
    idx = [M - 1] if P == 1 else [0] + [7 + 61 * i for i in range(P - 2)] + [M - 1]
    assert len(set(idx)) == P and max(idx) == M - 1 and all(b - a >= 3 for a, b in zip(idx, idx[1:]))
    return idx


class Rows:
    """K rows of M elements, every row 16-B aligned, in one guarded buffer."""

    def __init__(self, K, M, nb):
        self.K, self.M, self.pitch = K, M, -(-M // 16) * 16
        self.dev = Dev(K * self.pitch, nb)
        self.ptrs = [self.dev.ptr + k * self.pitch * nb for k in range(K)]

    def host(self, a):
        out = np.zeros((self.K, self.pitch), a.dtype)
        out[:, : self.M] = a
        return out


def _rows_input(job, a, b):
    rows = Rows(a.shape[0], a.shape[1], a.dtype.itemsize)
    job.input(rows.dev, rows.host(a), rows.host(b))
    return rows


def _tiled_input(job, kind, a, b, tv):
    """The rows in the tile-interleaved layout of fedagg_fedavg_tiled_*."""
    K, M = a.shape
    dev = Dev(tiled_elems(kind, K, M, tv), a.dtype.itemsize)
    at = tiled_index(kind, K, np.arange(K)[:, None], np.arange(M)[None, :], tv)

    def lay(x):
        out = np.zeros(dev.n, x.dtype)
        out[at] = x
        return out

    job.input(dev, lay(a), lay(b))
    return dev


def _workspace(job, nbytes):
    dev = Dev(nbytes // 8 + 2, 8)
    job.scratch.append(dev)
    return dev


# =============================================================================================
# FedAvg and Scaffold entry points with the numel == 1 patch
# =============================================================================================
def _fedavg(kind, K, P, tv=None):
    def build(lib):
        job = Job()
        M = M0 if tv is None else tv * L_OF[kind] + 37
        tag = f"fedavg-{kind}-{K}-{P}-{tv}"
        ns, idx = _samples(K), _idx(M, P)
        w = fedavg_weights(ns, kind)
        x = {ds: _draw(_rng(tag, ds), kind, (K, M)) for ds in "AB"}
        rows = _rows_input(job, x["A"], x["B"]) if tv is None else _tiled_input(job, kind, x["A"], x["B"], tv)
        out = job.output(Dev(M, NB[OUT_OF[kind]]))
        ws = _workspace(job, lib.fedagg_pairwise_ws_bytes(K, P, 8))

        def call(lib, sp):
            h = Host()
            if tv is None:
                _ok(lib, getattr(lib, f"fedagg_fedavg_{kind}")(h.ptrs(rows.ptrs), h.weights(w, kind), K, M, h.idx(idx), P,
                                                                ws.ptr, out.ptr, sp))
            else:
                _ok(lib, getattr(lib, f"fedagg_fedavg_tiled_{kind}")(rows.ptr, h.weights(w, kind), K, M, tv, h.idx(idx), P,
                                                                      ws.ptr, out.ptr, sp))
            return h

        job.call = call
        job.expect = lambda ds: [(out, OUT_OF[kind], _oracle_layers(_upcast(x[ds], kind), ns, idx), None)]
        return job

    return build


def _scaffold_two(kind, K, P):
    def build(lib):
        job = Job()
        M, tag = M0, f"scaffold-{kind}-{K}-{P}"
        w, idx = _sc_weights(K), _idx(M0, P)
        d = {ds: _draw(_rng(tag + "d", ds), kind, (K, M)) for ds in "AB"}
        cv = {ds: _draw(_rng(tag + "cv", ds), kind, (K, M)) for ds in "AB"}
        c = {ds: _draw(_rng(tag + "c", ds), kind, M) for ds in "AB"}
        rd, rcv = _rows_input(job, d["A"], d["B"]), _rows_input(job, cv["A"], cv["B"])
        dc = job.input(Dev(M, NB[kind]), c["A"], c["B"])
        dout, cout = job.output(Dev(M, 8)), job.output(Dev(M, 8))
        ws = _workspace(job, lib.fedagg_pairwise_ws_bytes(K, P, 8))

        def call(lib, sp):
            h = Host()
            _ok(lib, getattr(lib, f"fedagg_scaffold_{kind}")(h.ptrs(rd.ptrs), h.ptrs(rcv.ptrs), dc.ptr, h.doubles(w), K, M,
                                                              h.idx(idx), P, ws.ptr, LR, dout.ptr, cout.ptr, sp))
            return h

        job.call = call
        job.expect = lambda ds: [(dout, "f64", _sc_reference(d[ds], w, 0, None, LR, idx, None, True), None),
                                 (cout, "f64", _sc_reference(cv[ds], w, 1, c[ds], LR, idx, None, True), None)]
        return job

    return build


def _scaffold_bucket(kind, c_kind, phase, K, P):
    def build(lib):
        job = Job()
        M, tag = M0, f"bucket-{kind}-{c_kind}-{phase}-{K}"
        w, idx = _sc_weights(K), _idx(M0, P)
        x = {ds: _draw(_rng(tag, ds), kind, (K, M)) for ds in "AB"}
        c = {ds: _draw(_rng(tag + "c", ds), c_kind, M) for ds in "AB"}
        rows = _rows_input(job, x["A"], x["B"])
        dc = job.input(Dev(M, NB[c_kind]), c["A"], c["B"])
        out = job.output(Dev(M, 8))
        ws = _workspace(job, lib.fedagg_pairwise_ws_bytes(K, P, 8))

        def call(lib, sp):
            h = Host()
            _ok(lib, lib.fedagg_scaffold_bucket(h.ptrs(rows.ptrs), CODE[kind], h.doubles(w), K, M, phase,
                                                dc.ptr if phase == 1 else None, CODE[c_kind], LR, h.idx(idx), P, ws.ptr,
                                                out.ptr, sp))
            return h

        job.call = call
        job.expect = lambda ds: [(out, "f64", _rows_reference(x[ds], kind, w, phase, c[ds], c_kind, LR, idx), None)]
        return job

    return build


# =============================================================================================
# chains: two calls in ONE capture, the second continuing the first
# =============================================================================================
def _fedavg_chain(kind, tv=None):
    """Block 0 (2 clients, seed = 1), then block 1 (3 clients, seed = 0) into the same output: the
    5-client sequential sum.  A replay re-seeds by itself."""
    def build(lib):
        job = Job()
        M = M0 if tv is None else tv * L_OF[kind] + 37
        tag = f"chain-{kind}-{tv}"
        w = fedavg_weights(_samples(5), kind)
        x = {ds: _draw(_rng(tag, ds), kind, (5, M)) for ds in "AB"}
        blocks = [(0, 2, 1), (2, 5, 0)]
        if tv is None:
            ins = [_rows_input(job, x["A"][a:b], x["B"][a:b]) for a, b, _ in blocks]
        else:
            ins = [_tiled_input(job, kind, x["A"][a:b], x["B"][a:b], tv) for a, b, _ in blocks]
        out = job.output(Dev(M, NB[OUT_OF[kind]]))

        def call(lib, sp):
            h = Host()
            for (a, b, seed), rows in zip(blocks, ins):
                if tv is None:
                    fn = getattr(lib, f"fedagg_fedavg_chain_{kind}")
                    _ok(lib, fn(h.ptrs(rows.ptrs), h.weights(w[a:b], kind), b - a, M, seed, out.ptr, sp))
                else:
                    fn = getattr(lib, f"fedagg_fedavg_chain_tiled_{kind}")
                    _ok(lib, fn(rows.ptr, h.weights(w[a:b], kind), b - a, M, tv, seed, out.ptr, sp))
            return h

        job.call = call
        job.expect = lambda ds: [(out, OUT_OF[kind], _np_sequential(_upcast(x[ds], kind), w, None), None)]
        return job

    return build


def _fedavg_chain_push(kind):
    """d_in = NULL into a first buffer (2 clients), then that buffer as the separate d_in of a
    second call (3 clients): the 2-client and the 5-client sequential sums."""
    def build(lib):
        job = Job()
        M, tag = M0, f"push-{kind}"
        w = fedavg_weights(_samples(5), kind)
        x = {ds: _draw(_rng(tag, ds), kind, (5, M)) for ds in "AB"}
        r0, r1 = _rows_input(job, x["A"][:2], x["B"][:2]), _rows_input(job, x["A"][2:], x["B"][2:])
        mid, out = job.output(Dev(M, 4)), job.output(Dev(M, 4))

        def call(lib, sp):
            h = Host()
            fn = getattr(lib, f"fedagg_fedavg_chain_push_{kind}")
            _ok(lib, fn(h.ptrs(r0.ptrs), h.weights(w[:2], kind), 2, M, None, mid.ptr, sp))
            _ok(lib, fn(h.ptrs(r1.ptrs), h.weights(w[2:], kind), 3, M, mid.ptr, out.ptr, sp))
            return h

        job.call = call
        job.expect = lambda ds: [(mid, "f32", _np_sequential(_upcast(x[ds], kind)[:2], w[:2], None), None),
                                 (out, "f32", _np_sequential(_upcast(x[ds], kind), w, None), None)]
        return job

    return build


def _scaffold_chain(kind):
    """Block 0 (2 clients, seed = 1, finish = 0), then block 1 (3 clients, seed = 0, finish = 1)."""
    def build(lib):
        job = Job()
        M, tag = M0, f"sc-chain-{kind}"
        w = _sc_weights(5)
        d = {ds: _draw(_rng(tag + "d", ds), kind, (5, M)) for ds in "AB"}
        cv = {ds: _draw(_rng(tag + "cv", ds), kind, (5, M)) for ds in "AB"}
        c = {ds: _draw(_rng(tag + "c", ds), kind, M) for ds in "AB"}
        blocks = [(0, 2, 1, 0), (2, 5, 0, 1)]
        rd = [_rows_input(job, d["A"][a:b], d["B"][a:b]) for a, b, _, _ in blocks]
        rcv = [_rows_input(job, cv["A"][a:b], cv["B"][a:b]) for a, b, _, _ in blocks]
        dc = job.input(Dev(M, NB[kind]), c["A"], c["B"])
        dout, cout = job.output(Dev(M, 8)), job.output(Dev(M, 8))

        def call(lib, sp):
            h = Host()
            for n, (a, b, seed, finish) in enumerate(blocks):
                _ok(lib, getattr(lib, f"fedagg_scaffold_chain_{kind}")(
                    h.ptrs(rd[n].ptrs), h.ptrs(rcv[n].ptrs), dc.ptr if finish else None, h.doubles(w[a:b]), b - a, M, seed,
                    finish, LR, dout.ptr, cout.ptr, sp))
            return h

        job.call = call
        job.expect = lambda ds: [(dout, "f64", _sc_reference(d[ds], w, 0, None, LR, [], None, True), None),
                                 (cout, "f64", _sc_reference(cv[ds], w, 1, c[ds], LR, [], None, True), None)]
        return job

    return build


def _scaffold_chain_push(kind, phase):
    """9 clients from d_in = NULL with finish = 0 into a first buffer, then 65 clients (two chunks)
    continuing that buffer as the separate d_in with finish = 1."""
    def build(lib):
        job = Job()
        M, tag, K0, K1 = M0, f"sc-push-{kind}-{phase}", 9, 65
        w = _sc_weights(K0 + K1)
        x = {ds: _draw(_rng(tag, ds), kind, (K0 + K1, M)) for ds in "AB"}
        c = {ds: _draw(_rng(tag + "c", ds), kind, M) for ds in "AB"}
        r0, r1 = _rows_input(job, x["A"][:K0], x["B"][:K0]), _rows_input(job, x["A"][K0:], x["B"][K0:])
        dc = job.input(Dev(M, NB[kind]), c["A"], c["B"])
        mid, out = job.output(Dev(M, 8)), job.output(Dev(M, 8))

        def call(lib, sp):
            h = Host()
            fn = getattr(lib, f"fedagg_scaffold_chain_push_{kind}")
            _ok(lib, fn(h.ptrs(r0.ptrs), h.doubles(w[:K0]), K0, M, phase, None, LR, 0, None, mid.ptr, sp))
            _ok(lib, fn(h.ptrs(r1.ptrs), h.doubles(w[K0:]), K1, M, phase, dc.ptr if phase == 1 else None, LR, 1, mid.ptr,
                        out.ptr, sp))
            return h

        def expect(ds):
            sums = _sc_reference(x[ds][:K0], w[:K0], phase, c[ds], LR, [], None, False)
            return [(mid, "f64", sums, None),
                    (out, "f64", _sc_reference(x[ds][K0:], w[K0:], phase, c[ds], LR, [], sums, True), None)]

        job.call, job.expect = call, expect
        return job

    return build


# =============================================================================================
# split numel == 1 trees: two product blocks, then the finish, in one capture
# =============================================================================================
PW_BLOCKS = [(0, 70), (70, 60)]  # (kbase, K): stride 130


def _pairwise(kind, P):
    def build(lib):
        job = Job()
        M, K, tag = M0, 130, f"pairwise-{kind}-{P}"
        w, idx = fedavg_weights(_samples(K), kind), _idx(M0, P)
        x = {ds: _draw(_rng(tag, ds), kind, (K, M)) for ds in "AB"}
        rows = [_rows_input(job, x["A"][a: a + n], x["B"][a: a + n]) for a, n in PW_BLOCKS]
        wnb = 8 if kind == "f64" else 4  # the pairwise-sum type: fp32 for f32 / bf16 / f16
        ws = job.output(Dev(P * K, wnb))
        out = job.output(Dev(M, NB[OUT_OF[kind]]))
        finish = {"f32": "f32", "bf16": "f32", "f64": "f64", "f16": "f16"}[kind]

        def call(lib, sp):
            h = Host()
            for (a, n), r in zip(PW_BLOCKS, rows):
                _ok(lib, getattr(lib, f"fedagg_pairwise_products_{kind}")(h.ptrs(r.ptrs), h.weights(w[a: a + n], kind), n,
                                                                           h.idx(idx), P, K, a, ws.ptr, sp))
            _ok(lib, getattr(lib, f"fedagg_pairwise_finish_{finish}")(ws.ptr, K, K, h.idx(idx), P, out.ptr, sp))
            return h

        def expect(ds):
            wide = np.float64 if kind == "f64" else np.float32
            with np.errstate(all="ignore"):
                prods = (_upcast(x[ds], kind)[:, idx] * w[:, None]).astype(wide).T  # [P, K], rounded in the product type
                assert prods.shape == (P, K)
                sums = np.array([numpy_pairwise_sum(np.ascontiguousarray(row)) for row in prods], wide)
                res = sums.astype(NP_OF[OUT_OF[kind]])
                res = res.dtype.type(0.0) + res
            return [(ws, "f64" if kind == "f64" else "f32", prods, None), (out, OUT_OF[kind], res, idx)]

        job.call, job.expect = call, expect
        return job

    return build


def _scaffold_pairwise(kind, P):
    def build(lib):
        job = Job()
        M, K, tag = M0, 130, f"sc-pairwise-{kind}-{P}"
        w, idx = _sc_weights(K), _idx(M0, P)
        d = {ds: _draw(_rng(tag + "d", ds), kind, (K, M)) for ds in "AB"}
        cv = {ds: _draw(_rng(tag + "cv", ds), kind, (K, M)) for ds in "AB"}
        c = {ds: _draw(_rng(tag + "c", ds), kind, M) for ds in "AB"}
        rd = [_rows_input(job, d["A"][a: a + n], d["B"][a: a + n]) for a, n in PW_BLOCKS]
        rcv = [_rows_input(job, cv["A"][a: a + n], cv["B"][a: a + n]) for a, n in PW_BLOCKS]
        dc = job.input(Dev(M, NB[kind]), c["A"], c["B"])
        ws = _workspace(job, P * (2 * K + 1) * 8)
        dout, cout = job.output(Dev(M, 8)), job.output(Dev(M, 8))

        def call(lib, sp):
            h = Host()
            for n, (a, k) in enumerate(PW_BLOCKS):
                _ok(lib, getattr(lib, f"fedagg_scaffold_products_{kind}")(h.ptrs(rd[n].ptrs), h.ptrs(rcv[n].ptrs),
                                                                           h.doubles(w[a: a + k]), k, a, K, h.idx(idx), P,
                                                                           ws.ptr, sp))
            _ok(lib, getattr(lib, f"fedagg_scaffold_finish_{kind}")(ws.ptr, K, dc.ptr, h.idx(idx), P, LR, dout.ptr, cout.ptr,
                                                                     sp))
            return h

        job.call = call
        job.expect = lambda ds: [(dout, "f64", _sc_reference(d[ds], w, 0, None, LR, idx, None, True)[idx], idx),
                                 (cout, "f64", _sc_reference(cv[ds], w, 1, c[ds], LR, idx, None, True)[idx], idx)]
        return job

    return build


# =============================================================================================
# client flat ops: 33 layers (two launches), torch eager ops on the CPU as the reference
# =============================================================================================
NUMEL = ([1, 7, 8, 300, 4099] * 7)[:33]
TORCH_OF = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "f64": torch.float64}
COEFFS = [0.1, -1.0 / (0.05 * 7)]  # neither representable in fp32


def _cpu(a: np.ndarray, kind: str):
    """Stored values as a CPU tensor of the kind."""
    return torch.from_numpy(_bits(a).view(SINT[NB[kind]]).copy()).view(TORCH_OF[kind])


def _stored(t) -> np.ndarray:
    """A CPU tensor's bit patterns."""
    nb = t.element_size()
    return t.contiguous().view(TINT[nb]).numpy().view(UINT[nb])


def _layers(job, kind, tag, inout=False):
    """33 layers of ``kind``, each a guarded 16-B aligned buffer; returns (devs, {ds: [arrays]})."""
    data = {ds: [_draw(_rng(f"{tag}{n}", ds), kind, m) for n, m in enumerate(NUMEL)] for ds in "AB"}
    devs = [job.input(Dev(m, NB[kind]), data["A"][n], data["B"][n], inout=inout) for n, m in enumerate(NUMEL)]
    return devs, data


def _flat_gather(kind, typed):
    def build(lib):
        job = Job()
        devs, data = _layers(job, kind, f"gather-{kind}")
        flat = job.output(Dev(sum(NUMEL), NB[kind]))

        def call(lib, sp):
            h = Host()
            ptrs, numel = h.ptrs([d.ptr for d in devs]), h.numel(NUMEL)
            if typed:
                _ok(lib, lib.fedagg_flat_gather_f32(ptrs, numel, len(NUMEL), flat.ptr, sp))
            else:
                _ok(lib, lib.fedagg_flat_gather(ptrs, CODE[kind], numel, len(NUMEL), flat.ptr, sp))
            return h

        job.call = call
        # concat(layers), every bit kept: compared as raw words
        job.expect = lambda ds: [(flat, kind, _stored(torch.cat([_cpu(a, kind) for a in data[ds]])), None)]
        return job

    return build


def _flat_scatter():
    def build(lib):
        job = Job()
        src = {ds: _draw(_rng("scatter", ds), "f32", sum(NUMEL)) for ds in "AB"}
        flat = job.input(Dev(sum(NUMEL), 4), src["A"], src["B"])
        devs = [job.output(Dev(m, 4)) for m in NUMEL]

        def call(lib, sp):
            h = Host()
            _ok(lib, lib.fedagg_flat_scatter_f32(h.ptrs([d.ptr for d in devs]), h.numel(NUMEL), len(NUMEL), flat.ptr, sp))
            return h

        job.call = call
        job.expect = lambda ds: [(d, "f32", _stored(t), None)
                                 for d, t in zip(devs, torch.split(_cpu(src[ds], "f32"), NUMEL))]
        return job

    return build


def _flat_wsum(kinds, flat_kind, typed=False):
    def build(lib):
        job = Job()
        lists = [_layers(job, k, f"wsum-{'-'.join(kinds)}-{j}") for j, k in enumerate(kinds)]
        flat = job.output(Dev(sum(NUMEL), NB[flat_kind]))

        def call(lib, sp):
            h = Host()
            ptrs = h.ptrs([d.ptr for devs, _ in lists for d in devs])  # list-major [nlists][L]
            if typed:
                _ok(lib, lib.fedagg_flat_wsum_f32(ptrs, len(kinds), h.doubles(COEFFS), h.numel(NUMEL), len(NUMEL), flat.ptr,
                                                  sp))
            else:
                _ok(lib, lib.fedagg_flat_wsum(ptrs, h.kinds([CODE[k] for k in kinds]), len(kinds), h.doubles(COEFFS),
                                              h.numel(NUMEL), len(NUMEL), flat.ptr, CODE[flat_kind], sp))
            return h

        def expect(ds):  # weight_manager.py:205-210 on CPU tensors: Python sum() from int 0, list order
            layers = [sum(_cpu(data[ds][n], k) * c for (_, data), k, c in zip(lists, kinds, COEFFS))
                      for n in range(len(NUMEL))]
            ref = torch.cat(layers)
            assert ref.dtype == TORCH_OF[flat_kind]
            return [(flat, flat_kind, _stored(ref), None)]

        job.call, job.expect = call, expect
        return job

    return build


def _flat_increment(layer_kind, flat_kind, entry):
    def build(lib):
        job = Job()
        mult = 0.1
        devs, data = _layers(job, layer_kind, f"incr-{layer_kind}-{flat_kind}", inout=True)
        u = {ds: _draw(_rng(f"incr-u-{layer_kind}-{flat_kind}", ds), flat_kind, sum(NUMEL)) for ds in "AB"}
        flat = job.input(Dev(sum(NUMEL), NB[flat_kind]), u["A"], u["B"])

        def call(lib, sp):
            h = Host()
            ptrs, numel = h.ptrs([d.ptr for d in devs]), h.numel(NUMEL)
            if entry == "f32":
                _ok(lib, lib.fedagg_flat_increment_f32(ptrs, numel, len(NUMEL), flat.ptr, mult, sp))
            elif entry == "flat":
                _ok(lib, lib.fedagg_flat_increment(ptrs, numel, len(NUMEL), flat.ptr, CODE[flat_kind], mult, sp))
            else:
                _ok(lib, lib.fedagg_flat_increment_kind(ptrs, CODE[layer_kind], numel, len(NUMEL), flat.ptr, CODE[flat_kind],
                                                        mult, sp))
            return h

        def expect(ds):  # weight_manager.py:137 on CPU tensors, layer by layer
            out = []
            for d, a, x in zip(devs, data[ds], torch.split(_cpu(u[ds], flat_kind), NUMEL)):
                w = _cpu(a, layer_kind)
                w += mult * x
                assert w.dtype == TORCH_OF[layer_kind]
                out.append((d, layer_kind, _stored(w), None))
            return out

        job.call, job.expect = call, expect
        return job

    return build


# =============================================================================================
# casts, read probes, equality check
# =============================================================================================
def _cast(in_kind, out_kind, scale=None):
    def build(lib):
        job = Job()
        n = 1003
        src = {}
        for ds in "AB":
            rng = _rng(f"cast-{in_kind}-{out_kind}-{scale}", ds)
            if in_kind == "i64":  # every magnitude, beyond 2^53 too
                src[ds] = (rng.integers(-(1 << 62), 1 << 62, n) >> rng.integers(0, 62, n)).astype(np.int64)
            else:
                src[ds] = (rng.standard_normal(n) * 10.0 ** rng.integers(-9, 6, n)).astype(NP_OF[in_kind])
        d_in = job.input(Dev(n, NB[in_kind]), src["A"], src["B"])
        out = job.output(Dev(n, NB[out_kind]))

        def call(lib, sp):
            if scale is None:
                _ok(lib, lib.fedagg_cast(d_in.ptr, CODE[in_kind], out.ptr, CODE[out_kind], n, sp))
            else:
                _ok(lib, lib.fedagg_scale_cast(d_in.ptr, CODE[in_kind], scale, out.ptr, CODE[out_kind], n, sp))
            return Host()

        def expect(ds):
            with np.errstate(all="ignore"):
                v = src[ds] if scale is None else src[ds] * src[ds].dtype.type(scale)
                assert v.dtype == src[ds].dtype
                return [(out, out_kind, v.astype(NP_OF[out_kind]), None)]

        job.call, job.expect = call, expect
        return job

    return build


def _read_probe():
    """The check of misc-read-probe-stream: sink[b] = the sum over wave 0 of workgroup b of what its
    lanes read (small integers: every order of the fp32 adds gives the same sum)."""
    def build(lib):
        job = Job()
        grid, nvec = 3, 5 * 256 + 77
        x = {ds: _rng("probe", ds).integers(-8, 9, nvec * 4 + 3).astype(np.float32) for ds in "AB"}
        d_x = job.input(Dev(x["A"].size, 4), x["A"], x["B"])
        sink = job.output(Dev(grid, 4))

        def call(lib, sp):
            _ok(lib, lib.fedagg_read_probe_f32(d_x.ptr, x["A"].size, sink.ptr, grid, sp))
            return Host()

        def expect(ds):
            lane = np.arange(nvec) % (grid * 256)
            v = x[ds][: nvec * 4].reshape(nvec, 4)
            ref = np.array([v[(lane >= b * 256) & (lane < b * 256 + 64)].sum(dtype=np.float64) for b in range(grid)])
            return [(sink, "f32", ref.astype(np.float32), None)]

        job.call, job.expect = call, expect
        return job

    return build


def _read_probe_tile(vpt):
    """The check of misc-read-probe-tile-*: the sink is written only by a thread whose XOR fold of
    its vectors is the marker.  Data set A: one marker word in the partial tile; B: none."""
    def build(lib):
        job = Job()
        tile, marker = vpt * 256, 0x9E3779B9
        nvec = 2 * tile + (vpt - 1) * 256 + 100
        a, b = np.zeros(nvec * 4, np.uint32), np.zeros(nvec * 4, np.uint32)
        a[(2 * tile + 256 + 150) * 4 + 3] = marker
        d_x = job.input(Dev(a.size, 4), a, b)
        sink = job.output(Dev(1, 4))

        def call(lib, sp):
            _ok(lib, lib.fedagg_read_probe_tile_f32(d_x.ptr, a.size, sink.ptr, vpt, sp))
            return Host()

        job.call = call
        job.expect = lambda ds: [(sink, "raw4", np.array([marker], np.uint32), None) if ds == "A"
                                 else (sink, "raw4", np.zeros(0, np.uint32), [])]
        return job

    return build


# ---- equality check data (also part of the client-count test below) ----
EQ_VPT, FA_BLOCK = 4, 256  # equal_launch's EQ_VPT and the workgroup size FA_BLOCK of fedagg.hip
SPECIAL_COLUMNS = 10  # first of five columns, planted where M >= 64


def _eq_copies(kind: str, K: int, M: int, rng) -> np.ndarray:
    """[K, M] copies of one row; five columns of special pairs (M >= 64), one position where copy 0
    differs from everyone, and LAST one differing element in every copy k >= 1 at (k * 7919) % M."""
    ft, ut = NP_OF[kind], UINT[NB[kind]]
    c = np.tile(rng.standard_normal(M).astype(ft), (K, 1))
    bits = c.view(ut)
    if M >= 64:
        s = SPECIAL_COLUMNS
        sign = ut(1) << ut(8 * NB[kind] - 1)
        qnan = ut(0x7FC00000) if kind == "f32" else ut(0x7FF8000000000000)
        c[0, s], c[1:, s] = 0.0, -0.0  # +0 against -0: equal
        bits[0, s + 1], bits[1:, s + 1] = qnan, qnan | sign | ut(0x1234)  # NaN against another NaN: equal
        bits[0, s + 2] = qnan  # NaN against a number: unequal
        c[0, s + 3], c[1:, s + 3] = np.inf, -np.inf  # unequal
        bits[0, s + 4], bits[1:, s + 4] = 0, 1  # 0 against the smallest subnormal: unequal
    c[0, M // 2] = c[1 % K, M // 2] - ft(1.0) if K > 1 else c[0, M // 2]
    base = c[0].copy()
    for k in range(1, K):
        p = (k * 7919) % M
        v = base[p] + ft(1.0)
        c[k, p] = v if np.isfinite(base[p]) and v != base[p] else ft(3.0)  # a number that copy 0 does not hold
    return c


def _eq_expected(c: np.ndarray) -> int:
    """scaffold.py:193-196 by value: +0 == -0, NaN == NaN; summed over copies 1 .. K-1."""
    with np.errstate(all="ignore"):
        x, r = c[1:], c[:1]
        return int(np.sum(~((x == r) | (np.isnan(x) & np.isnan(r)))))


def _equal_count(kind, K):
    """The counter adds: it is zeroed on the stream before each run, like a caller must."""
    def build(lib):
        job = Job()
        M = M0
        c = {ds: _eq_copies(kind, K, M, _rng(f"eq-{kind}-{K}", ds)) for ds in "AB"}
        c["B"][K - 1, 77] += NP_OF[kind](2.0)  # another count than A's
        rows = _rows_input(job, c["A"], c["B"])
        zero = np.zeros(1, np.uint64)
        cnt = job.input(Dev(1, 8), zero, zero, inout=True)

        def call(lib, sp):
            h = Host()
            _ok(lib, getattr(lib, f"fedagg_equal_count_{kind}")(h.ptrs(rows.ptrs), K, M, cnt.ptr, sp))
            return h

        def expect(ds):
            n = _eq_expected(c[ds])
            assert n >= K - 1
            return [(cnt, "raw8", np.array([n], np.uint64), None)]

        job.call, job.expect = call, expect
        return job

    return build


# =============================================================================================
# the cases: id -> (the fedagg.h entry points the case calls, its builder)
# =============================================================================================
def _cases():
    cases = {}

    def add(cid, entries, build):
        assert cid not in cases, cid
        cases[cid] = (tuple(entries), build)

    # K = 3 with P = 2: one launch, fused patch; P = 17: the separate path; P = 65: two index
    # batches; K = 129, P = 2: two chunks, two gathers and the tree
    shapes = [(3, 2), (3, 17), (3, 65), (129, 2)]
    for kind in ("f32", "bf16", "f64", "f16"):
        for K, P in shapes:
            add(f"fedavg_{kind}-K{K}-P{P}", [f"fedagg_fedavg_{kind}"], _fedavg(kind, K, P))
    for kind, tv in TILES:
        for K, P in shapes:
            add(f"fedavg_tiled_{kind}-T{tv}-K{K}-P{P}", [f"fedagg_fedavg_tiled_{kind}"], _fedavg(kind, K, P, tv))
    # K = 3: one walk over both buckets (f32; f64 takes the one-bucket pair); K = 17: two launches
    # per chunk; K = 65: two chunks and the separate patch
    for kind in ("f32", "f64"):
        for K, P in ((3, 2), (17, 2), (65, 1)):
            add(f"scaffold_{kind}-K{K}-P{P}", [f"fedagg_scaffold_{kind}"], _scaffold_two(kind, K, P))
    for kind in ("f16", "bf16", "f32", "f64"):
        for c_kind in ((kind, "f64") if kind in ("f16", "bf16") else (kind,)):
            for phase in (0, 1):
                for K, P in ((3, 2), (65, 1)):
                    add(f"scaffold_bucket-{kind}-c{c_kind}-ph{phase}-K{K}-P{P}", ["fedagg_scaffold_bucket"],
                        _scaffold_bucket(kind, c_kind, phase, K, P))
    for kind in ("f32", "bf16", "f64", "f16"):
        add(f"fedavg_chain_{kind}", [f"fedagg_fedavg_chain_{kind}"], _fedavg_chain(kind))
    for kind, tv in TILES:
        add(f"fedavg_chain_tiled_{kind}-T{tv}", [f"fedagg_fedavg_chain_tiled_{kind}"], _fedavg_chain(kind, tv))
    for kind in ("f32", "bf16"):
        add(f"fedavg_chain_push_{kind}", [f"fedagg_fedavg_chain_push_{kind}"], _fedavg_chain_push(kind))
    for kind in ("f32", "f64"):
        add(f"scaffold_chain_{kind}", [f"fedagg_scaffold_chain_{kind}"], _scaffold_chain(kind))
        for phase in (0, 1):
            add(f"scaffold_chain_push_{kind}-ph{phase}", [f"fedagg_scaffold_chain_push_{kind}"],
                _scaffold_chain_push(kind, phase))
    for P in (3, 65):
        for kind, finish in (("f32", "f32"), ("bf16", "f32"), ("f64", "f64"), ("f16", "f16")):
            add(f"pairwise_{kind}-P{P}", [f"fedagg_pairwise_products_{kind}", f"fedagg_pairwise_finish_{finish}"],
                _pairwise(kind, P))
        for kind in ("f32", "f64"):
            add(f"scaffold_pairwise_{kind}-P{P}", [f"fedagg_scaffold_products_{kind}", f"fedagg_scaffold_finish_{kind}"],
                _scaffold_pairwise(kind, P))
    add("flat_gather_f32", ["fedagg_flat_gather_f32"], _flat_gather("f32", True))
    add("flat_scatter_f32", ["fedagg_flat_scatter_f32"], _flat_scatter())
    add("flat_wsum_f32", ["fedagg_flat_wsum_f32"], _flat_wsum(("f32", "f32"), "f32", True))
    add("flat_increment_f32", ["fedagg_flat_increment_f32"], _flat_increment("f32", "f32", "f32"))
    for kind in ("f16", "bf16", "f32", "f64"):
        add(f"flat_gather-{kind}", ["fedagg_flat_gather"], _flat_gather(kind, False))
    # every (list kinds, result kind) fedagg.h accepts: fp32 / fp64 lists with the promoted result,
    # every list and the result of one 16-bit kind
    for kinds, fk in ((("f32", "f32"), "f32"), (("f32", "f64"), "f64"), (("f64", "f32"), "f64"), (("f64", "f64"), "f64"),
                      (("f16", "f16"), "f16"), (("bf16", "bf16"), "bf16")):
        add(f"flat_wsum-{kinds[0]}-{kinds[1]}-to-{fk}", ["fedagg_flat_wsum"], _flat_wsum(kinds, fk))
    for fk in ("f32", "f64"):
        add(f"flat_increment-{fk}", ["fedagg_flat_increment"], _flat_increment("f32", fk, "flat"))
    for lk, fk in (("f16", "f16"), ("bf16", "bf16"), ("bf16", "f32")):
        add(f"flat_increment_kind-{lk}-{fk}", ["fedagg_flat_increment_kind"], _flat_increment(lk, fk, "kind"))
    for a, b in (("i64", "f64"), ("f64", "f16"), ("f32", "f64")):
        add(f"cast-{a}-{b}", ["fedagg_cast"], _cast(a, b))
    for a, b in (("f64", "f16"), ("f32", "f64")):  # float inputs only: the product is formed in the input's type
        add(f"scale_cast-{a}-{b}", ["fedagg_scale_cast"], _cast(a, b, scale=0.3))
    add("read_probe", ["fedagg_read_probe_f32"], _read_probe())
    for vpt in (4, 8, 16):
        add(f"read_probe_tile-{vpt}", ["fedagg_read_probe_tile_f32"], _read_probe_tile(vpt))
    for kind in ("f32", "f64"):
        for K in (7, 131):
            add(f"equal_count_{kind}-K{K}", [f"fedagg_equal_count_{kind}"], _equal_count(kind, K))
    return cases


CASES = _cases()
CASE_IDS = list(CASES)
CASE_ENTRIES = {cid: entries for cid, (entries, _) in CASES.items()}


@pytest.mark.parametrize("cid", CASE_IDS)
def test_stream_contract(cid, side_stream):
    _run_case(CASES[cid][1], side_stream, cid)


# =============================================================================================
# Equality check: every copy counts (legacy stream, eager calls)
# =============================================================================================
def _eq_sizes(kind: str):
    """1, L - 1, L, T - 1, T + L + 1, 2T + 5: L elements per 16 bytes, T = EQ_VPT * FA_BLOCK * L the
    vector kernel's workgroup step."""
    L = 16 // NB[kind]
    T = EQ_VPT * FA_BLOCK * L
    return sorted({1, L - 1, L, T - 1, T + L + 1, 2 * T + 5})


def _eq_count(lib, kind, dev_rows: Rows, off: int, K: int, M: int, cnt: Dev) -> None:
    nb = NB[kind]
    ptrs = _native.ptr_array([p + off * nb for p in dev_rows.ptrs])
    _ok(lib, getattr(lib, f"fedagg_equal_count_{kind}")(ptrs, K, M, cnt.ptr, None))


# K - 1 compared copies: the remainder loop alone (1, 2, 3), one whole group of four, a group plus
# one, one full chunk of 128, a chunk plus one and plus two
@pytest.mark.parametrize("K", [2, 3, 4, 5, 6, 129, 130, 131])
@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_equal_count_every_copy_counts(kind, K):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    lib = _native.load()
    cross_checked, launches, wrong = 0, 0, []
    try:
        for M in _eq_sizes(kind):
            c = _eq_copies(kind, K, M, np.random.default_rng([K, M]))
            want = _eq_expected(c)
            assert want >= K - 1  # every copy k >= 1 differs from copy 0 somewhere
            if M in _eq_sizes(kind)[:3]:  # the formula is zero exactly when assert_array_equal(c_0, c_k) passes
                for rows in (c, np.tile(c[0], (K, 1))):
                    for k in range(1, K):
                        try:
                            np.testing.assert_array_equal(rows[0], rows[k])
                            passes = True
                        except AssertionError:
                            passes = False
                        assert passes == (_eq_expected(rows[[0, k]]) == 0), (M, k)
                cross_checked += 1
            # rows aligned (offset 0) and shifted by one element (the scalar kernel), in one buffer
            dev = {}
            for off in (0, 1):
                dev[off] = Rows(K, M + 1, NB[kind])
                host = np.zeros((K, dev[off].pitch), c.dtype)
                host[:, off: off + M] = c
                dev[off].dev.put(host)
            cnt = Dev(1, 8)
            for eq_vec in (1, 0):
                for cap in (0, 1):  # 1: one workgroup strides over every tile
                    _native.tune(eq_vec=eq_vec, grid_cap=cap)
                    for off in (0, 1):
                        what = f"{kind} K={K} M={M} eq_vec={eq_vec} grid_cap={cap} offset={off}"
                        cnt.put(np.zeros(1, np.uint64))
                        _eq_count(lib, kind, dev[off], off, K, M, cnt)
                        torch.cuda.synchronize()
                        first = int(cnt.get()[0])
                        _eq_count(lib, kind, dev[off], off, K, M, cnt)  # the entry ADDS to the counter
                        torch.cuda.synchronize()
                        launches += 1
                        if (first, int(cnt.get()[0])) != (want, 2 * want):
                            wrong.append(f"{what}: counted {first}, then {int(cnt.get()[0])}; expected {want}, "
                                         f"then {2 * want}")
                        assert cnt.guards_intact(), what
            assert dev[0].dev.guards_intact() and dev[1].dev.guards_intact(), (kind, K, M)
    finally:
        _native.tune(eq_vec=1, grid_cap=0)
    assert not wrong, f"{len(wrong)} of {launches} launch pairs miscounted: " + "; ".join(wrong[:16])
    assert cross_checked == 3


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_equal_count_without_work_touches_nothing(kind):
    """K = 1 (nothing to compare) and M = 0 return 0 and leave the counter alone."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    lib = _native.load()
    c = _eq_copies(kind, 3, 100, np.random.default_rng(3))
    rows = Rows(3, 100, NB[kind])
    rows.dev.put(rows.host(c))
    cnt = Dev(1, 8)
    for K, M in ((1, 100), (3, 0), (1, 0)):
        _eq_count(lib, kind, rows, 0, K, M, cnt)
        torch.cuda.synchronize()
        assert int(cnt.get()[0]) == SENTINEL[8] and cnt.guards_intact(), (K, M)
