"""Single-process, multi-device aggregation: parameter-range shards over the node's GPUs.

A Substra aggregate task is ONE OS process (``remote/register/register.py:96-121`` runs one
``function.py``), so a multi-process ``torch.distributed`` launch does not fit the drop-in path
("Single process, multi-device").  :class:`MultiDeviceEngine` therefore drives
several GPUs from one process:

* the flat bucket range ``[0, M)`` is cut into one contiguous shard per device
  (``sharding.shard_bounds``, 512-element aligned, so every shard row starts 256-B aligned);
* a thread per shard stages bytes ``[lo, hi)`` of every client's row over that GPU's own PCIe link
  (``fedagg_session_stage_range``: the pinned-ring pack reads straight from the clients' layer
  arrays, no host-side re-slicing), runs the same bucket kernel with the same client order on it,
  and fetches the result straight into its slice of the one output array;
* a shard too large for its GPU's free HBM (``K x M`` beyond 288 GB, e.g. 256 clients x 350M
  fp32) is streamed through that GPU in sub-ranges (out-of-core), so any size aggregates.

Each output element is computed by exactly the arithmetic of the single-GPU kernel, so results
are bit-identical to :class:`engine.AggregationEngine` and to the reference (no collective, no
re-association).  numel == 1 layers are patched by the shard that owns them.  Layer sets the
range path does not cover (several dtype groups in one update, dtype conversions, Scaffold lists
of different shapes) run on the first device's single-GPU engine -- still the HIP path.

Reference behaviour replaced: ``FedAvg.avg_shared_states`` (substrafl/strategies/fed_avg.py:
207-222) and ``Scaffold.avg_shared_states`` (substrafl/strategies/scaffold.py:297-337).
"""

from __future__ import annotations

import os
import threading
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native, runtime
from .engine import (KIND_CODES, TILED_KINDS, AggregationEngine, FedAvgPlan, ScaffoldBucketPlan, ScaffoldPlan,
                     TiledFedAvgPlan, bucket_dtype16, direct_rows, equal_count, fedavg_weights, kind_of,
                     native_byte_order, reject_bf16, reject_mxfp8, scaffold_bucket_dtypes, scaffold_weights, serialized, tiled_elems,
                     tiled_recommended, tiled_tile)
from .layout import ROW_ALIGN_BYTES, BucketLayout
from .sharding import SHARD_ALIGN, shard_bounds
from .wire import BF16

HBM_HEADROOM = 0.85  # fraction of a device's free HBM one sub-range may use when no cap is given


PACK_THREADS_CAP = 32  # per GPU: past this the pack no longer scales (DESIGN.md §7 "Host ingress")


def pack_threads_per_gpu(cpus: int, gpus: int, cap: int = PACK_THREADS_CAP) -> int:
    """Pack workers per GPU: the CPUs this process may run on, divided among the GPUs -- not the
    single-session default of 16 divided among them, which left 2 workers per GPU at 8 GPUs on a
    256-CPU host (VERDICT r04 "Next 4") -- at least 2, at most ``cap``."""
    return max(2, min(cap, int(cpus) // max(1, int(gpus))))


def _cpulist(text: str) -> List[int]:
    """``0-3,8,10-11`` (sysfs cpulist) -> [0, 1, 2, 3, 8, 10, 11]."""
    out: List[int] = []
    for part in text.strip().split(","):
        if not part:
            continue
        a, _, b = part.partition("-")
        out += list(range(int(a), int(b or a) + 1))
    return out


def gpu_numa_node(bus_id: str, sysfs: str = "/sys/bus/pci/devices") -> Optional[int]:
    """NUMA node of the PCI device ``bus_id`` (``dddd:bb:dd.f``): its sysfs ``numa_node``; None when
    unknown (-1 in sysfs, a single-node host, or no sysfs)."""
    try:
        with open(os.path.join(sysfs, bus_id, "numa_node")) as f:
            node = int(f.read().strip())
    except (OSError, ValueError):
        return None
    return node if node >= 0 else None


def node_cpus(node: Optional[int], allowed: Sequence[int], sysfs: str = "/sys/devices/system/node") -> List[int]:
    """The CPUs of NUMA ``node`` this process may run on (``allowed``), [] when unknown."""
    if node is None:
        return []
    try:
        with open(os.path.join(sysfs, f"node{int(node)}", "cpulist")) as f:
            cpus = _cpulist(f.read())
    except (OSError, ValueError):
        return []
    allowed = set(int(c) for c in allowed)
    return [c for c in cpus if c in allowed]


def host_placement(bus_ids: Sequence[str], pack_threads: Optional[int] = None,
                   allowed: Optional[Sequence[int]] = None, pci_sysfs: str = "/sys/bus/pci/devices",
                   node_sysfs: str = "/sys/devices/system/node") -> List[Dict[str, object]]:
    """Per GPU (its PCI bus id), where its host ingress runs: ``threads`` pack workers
    (:func:`pack_threads_per_gpu` over the CPUs this process may use, unless given), bound to the
    allowed CPUs of the GPU's NUMA node (``cpus``; [] = unbound: unknown node, or none of its CPUs
    allowed), where its pinned ring is allocated too (``fedagg_session_affinity``)."""
    allowed = sorted(allowed if allowed is not None else os.sched_getaffinity(0))
    per = int(pack_threads) if pack_threads else pack_threads_per_gpu(len(allowed), len(bus_ids))
    out = []
    for bus in bus_ids:
        node = gpu_numa_node(bus, pci_sysfs)
        out.append({"bus_id": bus, "numa_node": node, "threads": per,
                    "cpus": node_cpus(node, allowed, node_sysfs)})
    return out


def _ld(n: int, isz: int) -> int:
    per_row = max(1, ROW_ALIGN_BYTES // isz)
    return max(per_row, -(-n // per_row) * per_row)


def _split(lo: int, hi: int, max_elems: int) -> List[Tuple[int, int]]:
    """Cut ``[lo, hi)`` into sub-ranges of at most ``max_elems`` (SHARD_ALIGN multiples)."""
    if hi <= lo:
        return []
    step = max(SHARD_ALIGN, (max_elems // SHARD_ALIGN) * SHARD_ALIGN)
    return [(a, min(hi, a + step)) for a in range(lo, hi, step)]


def _range_rows(rows: List[List[np.ndarray]], lo: int, hi: int) -> List[List[np.ndarray]]:
    """Elements ``[lo, hi)`` of every row (contiguous arrays in bucket order) as flat views."""
    out = []
    for row in rows:
        segs, a0 = [], 0
        for a in row:
            a1 = a0 + a.size
            if a1 > lo and a0 < hi:
                segs.append(a.reshape(-1)[max(lo, a0) - a0:min(hi, a1) - a0])
            a0 = a1
        out.append(segs)
    return out


class MultiDeviceEngine:
    """Drop-in host path over ``devices`` (GPU indices; a repeated index gets its own session,
    which lets a one-GPU box rehearse the sharded path).  ``max_shard_bytes`` caps the HBM one
    sub-range of a shard may take (default: 85 % of the device's free HBM)."""

    # HBM buffer slots (same numbering as AggregationEngine)
    _B_BUCKET, _B_OUT, _B_WS, _B_CV, _B_C, _B_COUT, _B_CNT = 0, 1, 2, 4, 5, 6, 7

    def __init__(self, devices: Sequence[int], max_shard_bytes: Optional[int] = None,
                 pack_threads: Optional[int] = None):
        self.devices = [int(d) for d in devices]
        if not self.devices:
            raise ValueError("MultiDeviceEngine needs at least one device")
        self.max_shard_bytes = max_shard_bytes
        self._pack_threads = pack_threads
        self._sessions = None
        self._fallback: Optional[AggregationEngine] = None
        self.last_timing: Dict[str, object] = {}
        # measurement switch (bench.py --engine multi-device): time each shard's kernel with HIP
        # events on its session stream (adds one event pair per sub-range)
        self.kernel_events = False
        # FedAvg sub-ranges in the tile-interleaved layout: off unless FEDAGG_TILED=1 ("auto" =
        # where the library recommends it for the sub-range's K x n).  Off by default: at C3 on
        # one GPU it staged 0.61-0.82 s per call against 0.61-0.64 s on rows, with the kernel no
        # faster right after the staging (profiles/r02i_md_bench_c3*.jsonl)
        self.tiled = {"1": True, "auto": "auto"}.get(os.environ.get("FEDAGG_TILED", "0"), False)

    def lock_devices(self) -> List[int]:
        return list(self.devices)

    # ----------------------------------------------------------------------------------
    def sessions(self):
        """One native session per shard (created on first use).  A shard's session is the GPU's
        process-wide one, which other engines stage on: its threads and CPUs are changed under the
        device locks (``runtime.device_lock``, reentrant: an engine call already holds them)."""
        if self._sessions is not None:
            return self._sessions
        locks = [runtime.device_lock(d) for d in sorted(set(self.devices))]
        for lk in locks:
            lk.acquire()
        try:
            return self._make_sessions()
        finally:
            for lk in reversed(locks):
                lk.release()

    def _make_sessions(self):
        if self._sessions is None:
            place = host_placement([runtime.device_pci_bus_id(d) for d in self.devices], self._pack_threads)
            seen = set()
            out = []
            for d, pl in zip(self.devices, place):
                if d in seen:
                    s = runtime.Session(d, threads=pl["threads"])  # private session: same GPU, second shard
                else:
                    s = runtime.session(d)
                    s.set("threads", pl["threads"])
                    seen.add(d)
                s.affinity(pl["cpus"])  # workers + pinned ring on the GPU's NUMA node
                out.append(s)
            self.placement = [{"device": d, "bus_id": pl["bus_id"], "numa_node": pl["numa_node"],
                               "threads": pl["threads"], "cpus": len(pl["cpus"])} for d, pl in zip(self.devices, place)]
            self._sessions = out
        return self._sessions

    def placement_report(self) -> List[Dict[str, object]]:
        """Per shard: device, PCI bus id, NUMA node, pack threads, CPUs they are bound to, and the
        node its pinned ring actually landed on (after a call: -1 before the ring exists)."""
        sess = self.sessions()
        return [dict(p, ring_node=s.ring_node()) for p, s in zip(self.placement, sess)]

    def prewarm(self) -> None:
        for d in sorted(set(self.devices)):
            runtime.prewarm(d)

    def ingest(self, paths: Sequence, strategy: str, load, max_workers: int = 0) -> List:
        """Threaded load of the shared-state files (the shards are staged by the aggregation
        call, each over its own link)."""
        from concurrent.futures import ThreadPoolExecutor

        paths = list(paths)
        if not paths:
            return []
        t0 = time.perf_counter()
        with ThreadPoolExecutor(max_workers or min(len(paths), 16, os.cpu_count() or 1)) as ex:
            futures = [ex.submit(load, p) for p in paths]
            states = [f.result() for f in futures]
        self.last_ingest = {"load_and_stage_s": time.perf_counter() - t0, "prestaged_clients": 0}
        return states

    def _single(self) -> AggregationEngine:
        if self._fallback is None:
            from .engine import engine_for

            self._fallback = engine_for(self.devices[0])
        return self._fallback

    def sequential_sum(self, rows, n_samples, wire: bool = False):
        """NewtonRaphson's averaging (:meth:`engine.AggregationEngine.sequential_sum`) on the first
        device: its inputs (a P x P Hessian per client) are not sharded by this engine."""
        return self._single().sequential_sum(rows, n_samples, wire)

    _FEDAVG_SLOTS = (0, 1, 2)
    _SCAFFOLD_SLOTS = (0, 1, 2, 4, 5, 6, 7)

    def _budget(self, g: int, slots: Sequence[int]) -> int:
        """HBM one sub-range may take on shard ``g``: free HBM plus the session buffers the call
        reuses (``slots``; buffers of other calls stay allocated and are not counted)."""
        if self.max_shard_bytes:
            return int(self.max_shard_bytes)

        free, _ = runtime.device_memory(self.devices[g])
        return int((free + self.sessions()[g].held_bytes(slots)) * HBM_HEADROOM)

    def plan_ranges(self, M: int, bytes_per_elem: int, slots: Sequence[int] = _SCAFFOLD_SLOTS
                    ) -> List[List[Tuple[int, int]]]:
        """Per shard, the sub-ranges it streams through its GPU."""
        bounds = shard_bounds(M, len(self.devices))
        plan = []
        for g, (lo, hi) in enumerate(bounds):
            cap = max(SHARD_ALIGN, self._budget(g, slots) // max(1, bytes_per_elem))
            plan.append(_split(lo, hi, cap))
        return plan

    def _run(self, work) -> None:
        """Run ``work(g, session)`` for every shard on its own thread; re-raise the first error."""
        sess = self.sessions()
        errors: List[Optional[BaseException]] = [None] * len(sess)

        def body(g):
            try:
                sess[g].activate()
                work(g, sess[g])
            except BaseException as e:  # noqa: BLE001 - re-raised on the calling thread
                errors[g] = e

        threads = [threading.Thread(target=body, args=(g,), name=f"fedagg-shard-{g}") for g in range(len(sess))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        for e in errors:
            if e is not None:
                raise e

    # ----------------------------------------------------------------------------------
    @serialized
    def fedavg(self, parameters_updates: List[List[np.ndarray]], n_samples: Sequence[int],
               wire: bool = False) -> List[np.ndarray]:
        """fed_avg.py:217-222 for validated inputs, sharded by parameter range over the devices."""
        t_start = time.perf_counter()
        parameters_updates = native_byte_order(parameters_updates)
        L = len(parameters_updates[0])
        if L == 0:
            return []
        reject_mxfp8(parameters_updates, "MultiDeviceEngine.fedavg (several devices, or out of core)")
        reject_bf16(parameters_updates, "MultiDeviceEngine.fedavg")
        dts = {a.dtype for pu in parameters_updates for a in pu}
        R = np.result_type(next(iter(dts)), 1.0) if len(dts) == 1 else None
        if R is None or R != next(iter(dts)) or R not in (np.float16, np.float32, np.float64):
            return self._single().fedavg(parameters_updates, n_samples, wire)  # dtype groups / casts
        return self._fedavg_ranges(parameters_updates, n_samples, wire, R, R, t_start)

    def _fedavg_ranges(self, parameters_updates, n_samples, wire: bool, R: np.dtype, Rout: np.dtype, t_start: float):
        """The sharded plan over rows uniformly of dtype ``R`` averaged into ``Rout`` (``R`` itself,
        or float32 for ``wire.BF16`` rows): per sub-range ``K`` rows of ``R`` in, one of ``Rout`` out."""
        K, L = len(parameters_updates), len(parameters_updates[0])
        layout = BucketLayout(list(range(L)), [a.shape for a in parameters_updates[0]], R)
        M, isz, osz = layout.M, R.itemsize, Rout.itemsize
        rows = direct_rows(parameters_updates, R, M)
        kind = kind_of(R)
        w = fedavg_weights(n_samples, kind)
        pw_all = layout.pairwise_idx.astype(np.int64)
        out = runtime.reusable_host_array(M, Rout, "multi-fedavg")
        ranges = self.plan_ranges(M, K * isz + osz, self._FEDAVG_SLOTS)
        ws_bytes = _native.load().fedagg_pairwise_ws_bytes(K, max(1, pw_all.size), 8)
        timing: List[Dict[str, float]] = [dict() for _ in self.devices]

        def work(g, s):
            tm = timing[g]
            for lo, hi in ranges[g]:
                n = hi - lo
                ld = _ld(n, isz)
                t0 = time.perf_counter()
                tv = None
                if kind in TILED_KINDS and self.tiled is not False and (
                        self.tiled is True or tiled_recommended(kind, K, n)):
                    tv = tiled_tile(kind, K, n)
                    d_bucket = s.buffer(self._B_BUCKET, tiled_elems(kind, K, n, tv) * isz)
                    s.stage_tiled(d_bucket, tv * 16, _range_rows(rows, lo, hi))
                else:
                    d_bucket = s.buffer(self._B_BUCKET, K * ld * isz)
                    s.stage(d_bucket, ld * isz, rows, byte_range=(lo * isz, hi * isz))
                t1 = time.perf_counter()
                d_out = s.buffer(self._B_OUT, _ld(n, osz) * osz)
                ws = s.buffer(self._B_WS, ws_bytes)
                pw = (pw_all[(pw_all >= lo) & (pw_all < hi)] - lo).astype(np.uint64)
                if self.kernel_events:
                    s.event_record(0)
                if tv is not None:
                    TiledFedAvgPlan(kind, d_bucket, K, w, n, d_out, pw, ws, tv).launch(s.stream)
                else:
                    FedAvgPlan(kind, [d_bucket + k * ld * isz for k in range(K)], w, n, d_out, pw, ws).launch(s.stream)
                if self.kernel_events:
                    s.event_record(1)
                s.fetch(d_out, out[lo:hi])
                if self.kernel_events:
                    tm["kernel_ms"] = tm.get("kernel_ms", 0.0) + s.event_elapsed_ms(0, 1)
                tm["stage_s"] = tm.get("stage_s", 0.0) + t1 - t0
                tm["kernel_fetch_s"] = tm.get("kernel_fetch_s", 0.0) + time.perf_counter() - t1
                tm["ranges"] = tm.get("ranges", 0) + 1
                tm["layout"] = "tiles" if tv is not None else "rows"

        self._run(work)
        self.last_timing = {"shards": timing, "total_s": time.perf_counter() - t_start,
                            "ranges": [r for r in ranges]}
        results: List[Optional[np.ndarray]] = [None] * L
        for li, arr in layout.unpack(out, wire):
            results[li] = arr
        return results  # type: ignore[return-value]

    def fedavg_routed(self, parameters_updates: List[List[np.ndarray]], n_samples: Sequence[int],
                      wire: bool = False) -> List[np.ndarray]:
        """What the strategies call: :meth:`fedavg`, and for updates that are uniformly
        ``wire.BF16`` the same sharded plan over 2-byte rows with an fp32 result (each sub-range one
        ``fedagg_fedavg_bf16`` / ``_tiled_bf16`` launch, ``K * 2 + 4`` bytes of HBM per element), bit-
        identical to :class:`engine.AggregationEngine` on one GPU.  :meth:`fedavg` itself keeps
        refusing ``wire.BF16`` (its refusal is pinned by tests), so the route is this name."""
        reject_mxfp8(parameters_updates, "MultiDeviceEngine.fedavg_routed (several devices, or out of core)")
        if (not parameters_updates or not parameters_updates[0]
                or not all(np.asarray(a).dtype == BF16 for pu in parameters_updates for a in pu)):
            return self.fedavg(parameters_updates, n_samples, wire)
        return self._fedavg_bf16(parameters_updates, n_samples, wire)

    @serialized
    def _fedavg_bf16(self, parameters_updates, n_samples, wire: bool):
        return self._fedavg_ranges(native_byte_order(parameters_updates), n_samples, wire, BF16,
                                   np.dtype(np.float32), time.perf_counter())

    # ----------------------------------------------------------------------------------
    @serialized
    def scaffold(self, parameters_updates, control_variate_updates, server_control_variates, n_samples,
                 aggregation_lr, wire: bool = False):
        """scaffold.py:193-196 (c equality, as a mismatch count) and :297-337 (fp64 sums), sharded by
        parameter range.  Returns ``(mismatches, new_server_control_variate, avg_parameters_update)``."""
        t_start = time.perf_counter()
        parameters_updates, control_variate_updates, server_control_variates = (
            native_byte_order(x) for x in (parameters_updates, control_variate_updates, server_control_variates))
        K = len(parameters_updates)
        L = len(parameters_updates[0])
        if L == 0:
            return 0, [], []
        lists = (parameters_updates, control_variate_updates, server_control_variates)
        for lst in lists:
            reject_mxfp8(lst, "MultiDeviceEngine.scaffold")
        dts = {a.dtype for lst in lists for client in lst for a in client}
        shapes = [[a.shape for a in lst[0]] for lst in lists]
        uniform = len(dts) == 1 and next(iter(dts)) in (np.float32, np.float64)
        if not uniform or not shapes[0] == shapes[1] == shapes[2]:
            return self._single().scaffold(*lists, n_samples, aggregation_lr, wire)
        sdt = next(iter(dts))
        kind = "f32" if sdt == np.float32 else "f64"
        isz = sdt.itemsize
        layout = BucketLayout(list(range(L)), shapes[0], sdt)
        M = layout.M
        rows_d = direct_rows(parameters_updates, sdt, M)
        rows_c = direct_rows(control_variate_updates, sdt, M)
        same_c = all(len(row) == len(server_control_variates[0]) and all(a is b for a, b in zip(row, server_control_variates[0]))
                     for row in server_control_variates[1:])
        rows_s = direct_rows(server_control_variates[:1] if same_c else server_control_variates, sdt, M)
        # identical c objects: one staged copy, no check; otherwise one staged copy and the check of
        # the others on the host while staging (Session.stage_check; see engine.scaffold)
        host_c = not same_c and self._single().c_check == "host"
        Kc = 1 if same_c or host_c else K
        w = scaffold_weights(n_samples)
        lr = float(aggregation_lr)
        pw_all = layout.pairwise_idx.astype(np.int64)
        out_d = runtime.reusable_host_array(M, np.float64, "multi-scaffold-delta")
        out_c = runtime.reusable_host_array(M, np.float64, "multi-scaffold-c")
        mism = [0] * len(self.devices)
        # per element: K deltas + K control variates + K server-c copies in, two fp64 outputs
        ranges = self.plan_ranges(M, (2 * K + Kc) * isz + 16, self._SCAFFOLD_SLOTS)
        ws_bytes = _native.load().fedagg_pairwise_ws_bytes(K, max(1, pw_all.size), 8)

        def work(g, s):
            for lo, hi in ranges[g]:
                n = hi - lo
                ld = _ld(n, isz)
                br = (lo * isz, hi * isz)
                d_d = s.buffer(self._B_BUCKET, K * ld * isz)
                d_cv = s.buffer(self._B_CV, K * ld * isz)
                d_cc = s.buffer(self._B_C, Kc * ld * isz)
                s.stage(d_d, ld * isz, rows_d, byte_range=br)
                s.stage(d_cv, ld * isz, rows_c, byte_range=br)
                if host_c:
                    mism[g] += s.stage_check(d_cc, rows_s, sdt, byte_range=br)
                else:
                    s.stage(d_cc, ld * isz, rows_s, byte_range=br)
                cnt = s.buffer(self._B_CNT, 8)
                s.memset(cnt, 0, 8)
                if not same_c and not host_c:
                    equal_count(kind, [d_cc + k * ld * isz for k in range(K)], n, cnt, s.stream)
                dout = s.buffer(self._B_OUT, _ld(n, 8) * 8)
                cout = s.buffer(self._B_COUT, _ld(n, 8) * 8)
                ws = s.buffer(self._B_WS, ws_bytes)
                pw = (pw_all[(pw_all >= lo) & (pw_all < hi)] - lo).astype(np.uint64)
                ScaffoldPlan(kind, [d_d + k * ld * isz for k in range(K)], [d_cv + k * ld * isz for k in range(K)],
                             d_cc, w, n, lr, dout, cout, pw, ws).launch(s.stream)
                m = np.zeros(1, np.int64)
                s.fetch(cnt, m)
                s.fetch(dout, out_d[lo:hi])
                s.fetch(cout, out_c[lo:hi])
                mism[g] += int(m[0])

        self._run(work)
        self.last_timing = {"total_s": time.perf_counter() - t_start, "ranges": ranges}
        avg = [a for _, a in layout.unpack(out_d, wire)]
        new_c = [a for _, a in layout.unpack(out_c, wire)]
        return int(sum(mism)), new_c, avg

    # ----------------------------------------------------------------------------------
    def scaffold_per_bucket(self, parameters_updates, control_variate_updates, server_control_variates, n_samples,
                            aggregation_lr, wire: bool = False):
        """:meth:`engine.AggregationEngine.scaffold_per_bucket` over the devices: what the strategies
        call.  With no 16-bit bucket this is :meth:`scaffold`.  Otherwise the kinds are chosen per
        bucket as on one GPU (``engine.scaffold_bucket_dtypes``) and, when every bucket's arrays
        already have its kind, each bucket is sharded by parameter range: raw rows staged per
        sub-range (2 B per element and client for a 16-bit bucket), the clients' ``c`` compared on
        the pack workers while one copy is staged (any kind), one ``fedagg_scaffold_bucket`` launch
        per sub-range, fp64 slices fetched into the one output.  Buckets that need a cast run on
        the first device's engine.  Same return as :meth:`scaffold`."""
        if (not parameters_updates or not parameters_updates[0] or (
                bucket_dtype16(parameters_updates) is None and bucket_dtype16(control_variate_updates) is None)):
            return self.scaffold(parameters_updates, control_variate_updates, server_control_variates, n_samples,
                                 aggregation_lr, wire)
        return self._scaffold_buckets(parameters_updates, control_variate_updates, server_control_variates, n_samples,
                                      aggregation_lr, wire)

    _BUCKET_SLOTS = (0, 1, 2, 5)

    @serialized
    def _scaffold_buckets(self, pus, cvs, scv, n_samples, aggregation_lr, wire: bool):
        t_start = time.perf_counter()
        pus, cvs, scv = (native_byte_order(x) for x in (pus, cvs, scv))
        K, L = len(pus), len(pus[0])
        dt_d, dt_c, dt_s, _ = scaffold_bucket_dtypes(pus, cvs, scv)
        lid = list(range(L))
        lay_d = BucketLayout(lid, [a.shape for a in pus[0]], dt_d)
        lay_c = BucketLayout(lid, [a.shape for a in cvs[0]], dt_c)
        lay_s = BucketLayout(lid, [a.shape for a in scv[0]], dt_s)
        same_c = all(len(row) == len(scv[0]) and all(a is b for a, b in zip(row, scv[0])) for row in scv[1:])
        rows_d = direct_rows(pus, dt_d, lay_d.M)
        rows_c = direct_rows(cvs, dt_c, lay_c.M)
        rows_s = direct_rows(scv[:1] if same_c else scv, dt_s, lay_s.M)
        if rows_d is None or rows_c is None or rows_s is None or lay_s.M != lay_c.M:
            return self._single().scaffold_per_bucket(pus, cvs, scv, n_samples, aggregation_lr, wire)  # casts
        kd, kc, ks = kind_of(dt_d), kind_of(dt_c), kind_of(dt_s)
        isz_d, isz_c, isz_s = dt_d.itemsize, dt_c.itemsize, dt_s.itemsize
        w = scaffold_weights(n_samples)
        lr = float(aggregation_lr)
        pw_d, pw_c = lay_d.pairwise_idx.astype(np.int64), lay_c.pairwise_idx.astype(np.int64)
        out_d = runtime.reusable_host_array(lay_d.M, np.float64, "multi-scaffold-delta")
        out_c = runtime.reusable_host_array(lay_c.M, np.float64, "multi-scaffold-c")
        # per element of a sub-range: K rows in, one fp64 out, and the one staged copy of c
        ranges_d = self.plan_ranges(lay_d.M, K * isz_d + 8, self._BUCKET_SLOTS)
        ranges_c = self.plan_ranges(lay_c.M, K * isz_c + 8 + isz_s, self._BUCKET_SLOTS)
        ws_bytes = _native.load().fedagg_pairwise_ws_bytes(K, max(1, pw_d.size, pw_c.size), 8)
        mism = [0] * len(self.devices)

        def work(g, s):
            for phase, rows, kind, isz, ranges, pw_all, out in ((0, rows_d, kd, isz_d, ranges_d, pw_d, out_d),
                                                                (1, rows_c, kc, isz_c, ranges_c, pw_c, out_c)):
                for lo, hi in ranges[g]:
                    n = hi - lo
                    ld = _ld(n, isz)
                    d_rows = s.buffer(self._B_BUCKET, K * ld * isz)
                    s.stage(d_rows, ld * isz, rows, byte_range=(lo * isz, hi * isz))
                    d_cc = None
                    if phase == 1:
                        ld_s = _ld(n, isz_s)
                        d_cc = s.buffer(self._B_C, ld_s * isz_s)
                        if same_c:
                            s.stage(d_cc, ld_s * isz_s, rows_s, byte_range=(lo * isz_s, hi * isz_s))
                        else:
                            mism[g] += s.stage_check(d_cc, rows_s, dt_s, byte_range=(lo * isz_s, hi * isz_s))
                    d_out = s.buffer(self._B_OUT, _ld(n, 8) * 8)
                    ws = s.buffer(self._B_WS, ws_bytes)
                    pw = (pw_all[(pw_all >= lo) & (pw_all < hi)] - lo).astype(np.uint64)
                    ScaffoldBucketPlan(kind, [d_rows + k * ld * isz for k in range(K)], phase, d_cc,
                                       ks if phase == 1 else None, w, n, lr, d_out, pw, ws).launch(s.stream)
                    s.fetch(d_out, out[lo:hi])

        self._run(work)
        self.last_timing = {"total_s": time.perf_counter() - t_start, "ranges": ranges_d, "ranges_cv": ranges_c,
                            "bucket_kinds": (kd, kc, ks), "c_check": "identity" if same_c else "host"}
        avg = [a for _, a in lay_d.unpack(out_d, wire)]
        new_c = [a for _, a in lay_c.unpack(out_c, wire)]
        return int(sum(mism)), new_c, avg


class NativeMultiFedAvg:
    """The one-call C entry ``fedagg_multi_*`` (csrc/multi.hip) from Python: the same
    parameter-range plan as :class:`MultiDeviceEngine` -- shards, one thread and one private session
    per device, NUMA-bound pack workers, HBM-sized sub-ranges -- run entirely in C++, one ctypes call
    per aggregation (what a host in another language binds).  FedAvg over
    uniform fp16, fp32 or fp64 layer lists (:meth:`fedavg`) or ``wire.BF16`` ones
    (:meth:`fedavg_bf16`); bit-identical to :class:`MultiDeviceEngine` and to the reference
    (fed_avg.py:217-222)."""

    def __init__(self, devices: Sequence[int], pack_threads: int = 0, max_shard_bytes: int = 0):
        import ctypes

        self.lib = _native.load()
        self.devices = [int(d) for d in devices]
        arr = (ctypes.c_int * len(self.devices))(*self.devices)
        self._h = self.lib.fedagg_multi_create(len(self.devices), arr, int(pack_threads))
        if not self._h:
            raise _native.NativeLibraryError(
                "fedagg_multi_create failed: " + self.lib.fedagg_last_error().decode(errors="replace"))
        if max_shard_bytes:
            _native.check(self.lib.fedagg_multi_set(self._h, b"max_shard_bytes", int(max_shard_bytes)), "multi_set")

    def close(self) -> None:
        if getattr(self, "_h", None):
            self.lib.fedagg_multi_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def fedavg(self, parameters_updates: List[List[np.ndarray]], n_samples: Sequence[int]) -> List[np.ndarray]:
        """fed_avg.py:217-222 for validated inputs whose layers all share one dtype, fp16, fp32 or fp64."""
        import ctypes

        K, L = len(parameters_updates), len(parameters_updates[0])
        dts = {a.dtype for pu in parameters_updates for a in pu}
        if len(dts) != 1 or next(iter(dts)) not in (np.float16, np.float32, np.float64):
            raise NotImplementedError("fedagg_multi_fedavg takes layers of one dtype, float16, float32 or float64")
        dt = np.dtype(next(iter(dts)))
        kind = kind_of(dt)
        layout = BucketLayout(list(range(L)), [a.shape for a in parameters_updates[0]], dt)
        nseg, ptrs, sizes, keep = runtime._segments(native_byte_order(parameters_updates))
        w = fedavg_weights(n_samples, kind)  # fp16: the weights' bit patterns, as the C entry takes them
        idx = layout.pairwise_idx.astype(np.uint64)
        out = runtime.reusable_host_array(layout.M, dt, "multi-native")
        fn = getattr(self.lib, f"fedagg_multi_fedavg_{kind}")
        _native.check(fn(self._h, K, nseg, ptrs, sizes, w.ctypes.data, idx.ctypes.data if idx.size else None,
                         int(idx.size), out.ctypes.data), "fedagg_multi_fedavg")
        del keep
        return [a for _, a in layout.unpack(out)]

    def fedavg_bf16(self, parameters_updates: List[List[np.ndarray]], n_samples: Sequence[int]) -> List[np.ndarray]:
        """fed_avg.py:217-222 on the exact fp32 upcast of validated inputs whose layers are all
        ``wire.BF16`` (``fedagg_multi_fedavg_bf16``): fp32 weights, fp32 layers back."""
        K, L = len(parameters_updates), len(parameters_updates[0])
        if not all(np.asarray(a).dtype == BF16 for pu in parameters_updates for a in pu):
            raise NotImplementedError("fedagg_multi_fedavg_bf16 takes layers that are all wire.BF16")
        layout = BucketLayout(list(range(L)), [a.shape for a in parameters_updates[0]], BF16)
        nseg, ptrs, sizes, keep = runtime._segments(native_byte_order(parameters_updates))
        w = fedavg_weights(n_samples, "bf16")
        idx = layout.pairwise_idx.astype(np.uint64)
        out = runtime.reusable_host_array(layout.M, np.float32, "multi-native")
        _native.check(self.lib.fedagg_multi_fedavg_bf16(self._h, K, nseg, ptrs, sizes, w.ctypes.data,
                                                        idx.ctypes.data if idx.size else None, int(idx.size),
                                                        out.ctypes.data), "fedagg_multi_fedavg_bf16")
        del keep
        return [a for _, a in layout.unpack(out)]

    def shard_info(self) -> List[Dict[str, int]]:
        """Per shard: device, NUMA node, pack workers, bound CPUs, and of the last call its element
        range and sub-ranges (``fedagg_multi_shard_info``)."""
        import ctypes

        out = []
        for g in range(len(self.devices)):
            v = [ctypes.c_int() for _ in range(4)] + [ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int()]
            _native.check(self.lib.fedagg_multi_shard_info(self._h, g, *[ctypes.byref(x) for x in v]), "shard_info")
            out.append(dict(zip(("device", "numa_node", "threads", "cpus", "lo", "hi", "ranges"), [x.value for x in v])))
        return out


class NativeMultiScaffold(NativeMultiFedAvg):
    """Scaffold on the one-call C entry (``fedagg_multi_scaffold_bucket``, csrc/multi.hip): one
    aggregation is two ctypes calls, the delta bucket then the control-variate bucket, each
    sharded by parameter range over ``devices`` entirely in C++ (what a host in another language
    binds).  Each bucket's arrays are uniformly fp16, ``wire.BF16``, fp32 or
    fp64 and are staged as they are; ``c`` may be any of the four next to a 16-bit
    control-variate bucket and has the bucket's kind next to an fp32 / fp64 one.  Bit-identical to
    ``fedagg_scaffold_bucket`` over the whole range and to the reference (scaffold.py:193-196,
    262-263, 293)."""

    @staticmethod
    def _uniform(rows, what: str) -> np.dtype:
        dts = {np.asarray(a).dtype for row in rows for a in row}
        dt = next(iter(dts)) if len(dts) == 1 else None
        if dt is None or not (dt == BF16 or dt in (np.float16, np.float32, np.float64)):
            raise NotImplementedError(f"fedagg_multi_scaffold_bucket takes {what} of one dtype: float16, wire.BF16, "
                                      "float32 or float64")
        return np.dtype(dt)

    def scaffold(self, parameters_updates, control_variate_updates, server_control_variates, n_samples,
                 aggregation_lr):
        """scaffold.py:193-196 (the equality of the clients' ``c``, as a mismatch count) and
        :297-337 for validated inputs.  Returns ``(mismatches, new_server_control_variate,
        avg_parameters_update)``, both fp64."""
        import ctypes

        pus, cvs, scv = (native_byte_order(x) for x in (parameters_updates, control_variate_updates,
                                                        server_control_variates))
        K, L = len(pus), len(pus[0])
        dt_d, dt_c, dt_s = (self._uniform(pus, "parameter updates"), self._uniform(cvs, "control-variate updates"),
                            self._uniform(scv, "server control variates"))
        if dt_c.itemsize != 2 and dt_s != dt_c:
            raise NotImplementedError("fedagg_multi_scaffold_bucket: next to a float32 / float64 control-variate "
                                      "bucket the server control variate has the bucket's dtype")
        lid = list(range(L))
        lay_d = BucketLayout(lid, [a.shape for a in pus[0]], dt_d)
        lay_c = BucketLayout(lid, [a.shape for a in cvs[0]], dt_c)
        same_c = all(len(row) == len(scv[0]) and all(a is b for a, b in zip(row, scv[0])) for row in scv[1:])
        Kc = 1 if same_c else K
        w = scaffold_weights(n_samples)
        out_d = runtime.reusable_host_array(lay_d.M, np.float64, "multi-native-scaffold-delta")
        out_c = runtime.reusable_host_array(lay_c.M, np.float64, "multi-native-scaffold-c")
        fn = self.lib.fedagg_multi_scaffold_bucket
        nseg, ptrs, sizes, keep = runtime._segments(pus)
        idx = lay_d.pairwise_idx.astype(np.uint64)
        _native.check(fn(self._h, 0, K, nseg, ptrs, sizes, KIND_CODES[kind_of(dt_d)], w.ctypes.data,
                         float(aggregation_lr), 0, 0, None, None, 0, idx.ctypes.data if idx.size else None,
                         int(idx.size), out_d.ctypes.data, None), "fedagg_multi_scaffold_bucket (delta)")
        nseg, ptrs, sizes, keep = runtime._segments(cvs)
        c_nseg, c_ptrs, c_sizes, c_keep = runtime._segments(scv[:Kc])
        idx = lay_c.pairwise_idx.astype(np.uint64)
        mism = ctypes.c_uint64(0)
        _native.check(fn(self._h, 1, K, nseg, ptrs, sizes, KIND_CODES[kind_of(dt_c)], w.ctypes.data,
                         float(aggregation_lr), Kc, c_nseg, c_ptrs, c_sizes, KIND_CODES[kind_of(dt_s)],
                         idx.ctypes.data if idx.size else None, int(idx.size), out_c.ctypes.data,
                         ctypes.byref(mism)), "fedagg_multi_scaffold_bucket (control variate)")
        del keep, c_keep
        avg = [a for _, a in lay_d.unpack(out_d)]
        new_c = [a for _, a in lay_c.unpack(out_c)]
        return int(mism.value), new_c, avg
