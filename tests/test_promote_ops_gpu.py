"""The promoted flat ops of a 16-bit model next to fp64 operands (``fedagg_promote_wsum`` /
``fedagg_promote_increment``, include/fedagg_promote.h, and their dispatch in
:mod:`substrafl_amd.algorithms.weight_manager`) against two references:

  (a) the reference's own expressions (weight_manager.py:137, :205-210) in torch ON THE DEVICE,
      every layer's operands tensors of their own -- the yardstick;
  (b) ``tests/promote_rules.py``: the rules of the header in single-dtype torch ops on the CPU.

(a) and (b) disagree on one class of elements, and (a) decides: torch on ROCm (2.10, MI355X)
multiplies an fp16 tensor by a Python scalar with ONE rounding of the exact product in the
tensor's trailing ``numel mod 2048`` elements (its unrolled loop fuses the multiply and the
conversion; an exact zero product is +0 there), and with the CPU's two roundings (fp32 product,
then fp16) in the full 2048-element blocks before them.  Measured with the values below and the
coefficients 0.3 and 7.7: 7 of 40993 sums ("edges") and 11 of 2485 ("many") differ from the CPU
rule (61 of the 2 x 2485 products of "many", most of them only in the sign of a zero, which no
sum shows), none for bf16, none for the coefficients +-1, -0.2, 1/3 and -1e-3 (whose
products never come near a rounding tie), none in ``fedagg_promote_increment``.  The kernel
reproduces the device (include/fedagg_promote.h); (b) is therefore taken with
``promote_rules.torch_remainder``, and how many elements that changes is printed.

Bit for bit on integer views, NaN-ness only where the reference is NaN.  Geometries, values and
guard bands are those of ``test_half_client_ops_gpu.py``.  Then the weight_manager level, a
three-round Scaffold federation of 16-bit models with the launches counted, and the stream
contract (side stream, capture and replay)."""

import copy
import ctypes
import functools
import gc

import numpy as np
import pytest
import torch

import promote_rules as pr
import test_scaffold16_federation_gpu as fed
from substrafl_amd import _native, _native_promote
from substrafl_amd.algorithms import weight_manager as wm
from test_half_client_ops_gpu import GEOMETRY, GUARD, KINDS, SENTINEL, _guarded, _guards_intact, _ptrs, _stream, _values

pytestmark = pytest.mark.gpu

SENTINEL64 = 0x5A5A5A5A5A5A5A5A
F64 = _native.FEDAGG_F64
F64_SPECIALS = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1e300, -1e300, 1e-300, 1e-320]
WSUM_CASES = pr.WSUM_CASES
MULTIPLIERS = pr.MULTIPLIERS


@pytest.fixture(params=[1, 0], ids=["vec", "scalar"])
def vec(request):
    _native_promote.tune(request.param)
    yield request.param
    _native_promote.tune(1)


def _values64(n, dtype, seed):
    """n doubles on the device: ~15 % specials, ~25 % exactly representable in ``dtype`` (sums that
    cancel, ties), the rest N(0, 1) scaled over twelve decades."""
    rng = np.random.default_rng(seed)
    normal = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)
    special = rng.choice(np.array(F64_SPECIALS), n)
    exact = _values(n, dtype, seed + 17).to(torch.float64).cpu().numpy()
    pick = rng.random(n)
    return torch.from_numpy(np.where(pick < 0.15, special, np.where(pick < 0.4, exact, normal))).cuda()


def _guarded64(numel, dtype, seed):
    bufs, layers = [], []
    for i, n in enumerate(numel):
        buf = torch.full((n + GUARD,), SENTINEL64, dtype=torch.int64, device="cuda").view(torch.float64)
        buf[:n] = _values64(n, dtype, seed * 1000 + i)
        bufs.append(buf)
        layers.append(buf[:n])
    return bufs, layers


def _guards_intact64(bufs, numel):
    return all(bool((b.view(torch.int64)[n:] == SENTINEL64).all()) for b, n in zip(bufs, numel))


def _flat64(total):
    return torch.full((total + GUARD,), SENTINEL64, dtype=torch.int64, device="cuda").view(torch.float64)


def _cat(layers):
    return torch.cat([t.reshape(-1) for t in layers])


def _report(what, got, ref_a, ref_b, cpu_rule=None):
    """Print the figures, then hold the result to (a), (a) to (b), and the result to (b).
    ``cpu_rule``: (b) without the device's fp16 remainder rule, for the record only."""
    da, db, dab = pr.same_bits(got, ref_a), pr.same_bits(got.cpu(), ref_b), pr.same_bits(ref_a.cpu(), ref_b)
    print(f"{what}: {got.numel()} elements; differ from torch on the device {da}, from the rules {db}; "
          f"device torch vs rules {dab}"
          + ("" if cpu_rule is None else f"; device torch vs the CPU rule {pr.same_bits(ref_a.cpu(), cpu_rule)}"))
    assert da == 0, f"{what}: {da} of {got.numel()} elements differ from torch on the device"
    assert dab == 0, f"{what}: torch on the device and the rules disagree on {dab} elements"
    assert db == 0, what


@functools.lru_cache(maxsize=None)
def _wsum_inputs(kind, geometry):
    """Four 16-bit and four fp64 lists (read only), and per case the two references."""
    dtype, _ = KINDS[kind]
    numel = GEOMETRY[geometry]
    b16 = [_guarded(numel, dtype, seed) for seed in range(4)]
    b64 = [_guarded64(numel, dtype, 40 + seed) for seed in range(4)]
    cases = []
    for kinds, coeffs in WSUM_CASES:
        lists = [(b16 if k == "T" else b64)[j][1] for j, k in enumerate(kinds)]
        with torch.no_grad():  # weight_manager.py:205-210, layer by layer
            ref_a = _cat([sum(p * c for p, c in zip(layer, coeffs)) for layer in zip(*lists)])
        flat_lists = [_cat(lst).cpu() for lst in lists]
        ref_b = pr.wsum(flat_lists, coeffs, once=pr.torch_remainder(numel))
        before = [_cat(lst).clone() for lst in lists]
        cases.append((kinds, coeffs, lists, ref_a, ref_b, before, pr.wsum(flat_lists, coeffs)))
    return b16, b64, cases


@pytest.mark.parametrize("geometry", sorted(GEOMETRY))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_promote_wsum_bit_exact_with_guard_bands(kind, geometry, vec):
    assert torch.cuda.is_available()
    _, code = KINDS[kind]
    numel = GEOMETRY[geometry]
    total = sum(numel)
    lib = _native_promote.load()
    n_arr = (ctypes.c_uint64 * len(numel))(*numel)
    b16, b64, cases = _wsum_inputs(kind, geometry)
    for kinds, coeffs, lists, ref_a, ref_b, before, cpu_rule in cases:
        nl = len(kinds)
        flat = _flat64(total)
        k_arr = (ctypes.c_int * nl)(*[code if k == "T" else F64 for k in kinds])
        c_arr = (ctypes.c_double * nl)(*[float(c) for c in coeffs])
        _native_promote.check(lib.fedagg_promote_wsum(_ptrs(lists), k_arr, nl, c_arr, n_arr, len(numel),
                                                      flat.data_ptr(), _stream()), "flat_promote_wsum")
        assert ref_a.dtype == torch.float64
        _report(f"wsum {kind} {kinds} {coeffs}", flat[:total], ref_a, ref_b, cpu_rule)
        assert bool((flat.view(torch.int64)[total:] == SENTINEL64).all()), kinds
        for lst, b in zip(lists, before):  # the lists are only read
            assert pr.same_bits(_cat(lst), b) == 0 and torch.equal(pr.as_bits(_cat(lst)), pr.as_bits(b))
    assert all(_guards_intact(b[0], numel) for b in b16) and all(_guards_intact64(b[0], numel) for b in b64)


@functools.lru_cache(maxsize=None)
def _increment_inputs(kind, geometry, mult):
    """w and u of every layer (with the constructed double-rounding operands on every third
    element), and the two references."""
    dtype, _ = KINDS[kind]
    numel = GEOMETRY[geometry]
    total = sum(numel)
    cw, ct = pr.double_rounding_operands(dtype)
    w0 = _values(total, dtype, 7)
    u0 = _values64(total, dtype, 8)
    third = torch.arange(0, total, 3)
    pick = third % cw.numel()
    w0[third.cuda()] = cw[pick].cuda()
    u0[third.cuda()] = (ct[pick] / mult).cuda()
    ws, us = list(torch.split(w0, numel)), list(torch.split(u0, numel))
    ref = [t.clone() for t in ws]  # each layer's operands tensors of their own
    with torch.no_grad():
        for r, uu in zip(ref, us):
            r.data += mult * uu.clone().data  # weight_manager.py:137
    ref_b = pr.increment(w0.cpu(), u0.cpu(), mult)
    n_constructed = int((pr.as_bits(pr.round_direct((w0.cpu().double() + mult * u0.cpu())[third].numpy(), dtype))
                         != pr.as_bits(ref_b[third])).sum())
    return w0, u0, _cat(ref), ref_b, n_constructed


@pytest.mark.parametrize("geometry", sorted(GEOMETRY))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_promote_increment_bit_exact_with_guard_bands(kind, geometry, vec):
    assert torch.cuda.is_available()
    dtype, code = KINDS[kind]
    numel = GEOMETRY[geometry]
    total = sum(numel)
    lib = _native_promote.load()
    n_arr = (ctypes.c_uint64 * len(numel))(*numel)
    for mult in MULTIPLIERS:
        w0, u0, ref_a, ref_b, n_constructed = _increment_inputs(kind, geometry, mult)
        assert n_constructed >= min(100, total // 4), n_constructed  # a direct conversion cannot pass
        w_bufs, w = _guarded(numel, dtype, 7)
        for t, src in zip(w, torch.split(w0, numel)):
            t.copy_(src)
        u = _flat64(total)
        u[:total] = u0
        u_before = u.clone()
        _native_promote.check(lib.fedagg_promote_increment(_ptrs([w]), code, n_arr, len(numel), u.data_ptr(), mult,
                                                           _stream()), "flat_promote_increment")
        _report(f"increment {kind} x {mult}", _cat(w), ref_a, ref_b)
        assert _guards_intact(w_bufs, numel)
        assert torch.equal(u.view(torch.int64), u_before.view(torch.int64))  # the update is only read


# ---------------------------------------------------------------------------------------------
# weight_manager
# ---------------------------------------------------------------------------------------------
def _mlp(dtype):
    torch.manual_seed(3)
    m = torch.nn.Sequential(torch.nn.Linear(6, 24), torch.nn.BatchNorm1d(24), torch.nn.ReLU(),
                            torch.nn.Linear(24, 16), torch.nn.ReLU(), torch.nn.Linear(16, 1)).to(dtype).cuda()
    with torch.no_grad():
        m[1].running_mean.normal_()
        m[1].running_var.uniform_(0.5, 2.0)
    return m


@pytest.fixture
def labels(monkeypatch):
    """The labels weight_manager hands to ``_native_promote.check``, in order."""
    seen, real = [], _native_promote.check

    def check(rc, what):
        seen.append(what)
        real(rc, what)

    monkeypatch.setattr(_native_promote, "check", check)
    return seen


def _state_bits(model):
    return [pr.as_bits(p.data).clone() for p in wm.model_parameters(model, True)()]


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_weight_manager_promoted_ops_equal_the_torch_loops(kind, vec, labels, monkeypatch):
    assert torch.cuda.is_available()
    dtype, _ = KINDS[kind]
    model = _mlp(dtype)
    shapes = [tuple(p.shape) for p in wm.model_parameters(model, True)()]
    numel = [int(np.prod(s)) for s in shapes]
    rng = np.random.default_rng(5)
    host = [rng.standard_normal(s) * 1e-2 for s in shapes]  # fp64 host layers, one array each
    bucket = torch.from_numpy(rng.standard_normal(sum(numel))).cuda()
    views = [v.view(s) for v, s in zip(torch.split(bucket, numel), shapes)]  # views of one fp64 device bucket
    bucket_before = pr.as_bits(bucket).clone()

    for name, u in (("host", host), ("device", views)):
        for mult in MULTIPLIERS:
            twin = copy.deepcopy(model)
            monkeypatch.setenv("FEDAGG_FLAT_PROMOTE", "0")  # the reference's torch loop
            wm.increment_parameters(twin, list(u), with_batch_norm_parameters=True, updates_multiplier=mult)
            monkeypatch.delenv("FEDAGG_FLAT_PROMOTE")
            assert labels == []
            wm.increment_parameters(model, list(u), with_batch_norm_parameters=True, updates_multiplier=mult)
            assert labels == ["flat_promote_increment"], (name, mult)
            labels.clear()
            for li, (g, r) in enumerate(zip(_state_bits(model), _state_bits(twin))):
                assert torch.equal(g, r), f"increment {name} x {mult}, layer {li}"
    assert torch.equal(pr.as_bits(bucket), bucket_before)  # the update is only read

    # Scaffold's three operand sets of round 2: c_i - c, -c - delta / (lr n), c_i + cv_update
    c_i = [_values(n, dtype, 60 + i).view(s) for i, (n, s) in enumerate(zip(numel, shapes))]
    delta = wm.get_parameters(model, True)  # views of one 16-bit bucket
    for lists, coeffs in (([c_i, views], [1, -1]), ([views, delta], [-1.0, -1.0 / (0.05 * 5)]), ([c_i, views], [1, 1])):
        monkeypatch.setenv("FEDAGG_FLAT_PROMOTE", "0")
        ref = wm.weighted_sum_parameters(lists, coeffs)
        monkeypatch.delenv("FEDAGG_FLAT_PROMOTE")
        assert labels == []
        got = wm.weighted_sum_parameters(lists, coeffs)
        assert labels == ["flat_promote_wsum"], coeffs
        labels.clear()
        assert wm.flat_bucket(got) is not None and wm.flat_bucket(got).dtype == torch.float64
        for li, (g, r) in enumerate(zip(got, ref)):
            assert g.dtype == r.dtype == torch.float64 and g.shape == r.shape
            assert pr.same_bits(g, r) == 0, f"wsum {coeffs}, layer {li}"
    # what the issue leaves to torch stays there: fp32 next to 16-bit
    mixed = wm.weighted_sum_parameters([c_i, [t.float() for t in c_i]], [1, -1])
    assert all(t.dtype == torch.float32 for t in mixed) and labels == []


# ---------------------------------------------------------------------------------------------
# federation: three rounds, bit-identical, launches counted per client train call
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_scaffold_16_bit_federation_three_rounds_counted(dtype, labels, monkeypatch):
    assert torch.cuda.is_available()
    _native.load()
    monkeypatch.setattr(torch.backends.cudnn, "enabled", False)  # deterministic BatchNorm, as in the two-round test
    monkeypatch.setattr(fed, "ROUNDS", 3)
    ref, _ = fed._run(dtype, accelerated=False)
    assert labels == []

    per_train, real_export = [], wm.export_numpy

    def export_numpy(tensors, wire=True, tag="export"):
        if tag == "export":  # the delta's export: the first export of a train call, after all of its weight moves
            per_train.append((labels.count("flat_promote_increment"), labels.count("flat_promote_wsum")))
            labels.clear()
        return real_export(tensors, wire=wire, tag=tag)

    monkeypatch.setattr(wm, "export_numpy", export_numpy)
    acc, kinds = fed._run(dtype, accelerated=True)
    fed._compare(ref, acc)
    k16 = "f16" if dtype == torch.float16 else "bf16"
    assert kinds == [(k16, k16, k16), (k16, "f64", "f64"), (k16, "f64", "f64")]
    # round 1: 16-bit only; round 2: the update + 5 steps, and c_i - c, cv_update, c_i + cv_update;
    # round 3: c_i is fp64 by now, so only cv_update mixes kinds (the fp64-only sums: fedagg_flat_wsum)
    assert per_train == [(0, 0)] * fed.CLIENTS + [(6, 3)] * fed.CLIENTS + [(6, 1)] * fed.CLIENTS


# ---------------------------------------------------------------------------------------------
# stream contract: asynchronous on the caller's stream, capturable
# ---------------------------------------------------------------------------------------------
def _stream_case(kind):
    dtype, code = KINDS[kind]
    numel = [8, 8192 + 9, 777]  # layer 1 starts 16-B aligned (wide), layer 2 at an odd element (element by element)
    total = sum(numel)
    data = []
    for seed in (1, 2):
        w = _values(total, dtype, 90 + seed)
        u = _values64(total, dtype, 95 + seed)
        x64 = _values64(total, dtype, 97 + seed)
        inc = pr.increment(w.cpu(), u.cpu(), 0.05)
        ws = pr.wsum([w.cpu(), x64.cpu()], [1, -1])
        data.append((w, u, x64, inc, ws))
    return dtype, code, numel, total, data


def _calls(lib, code, numel, w, x64, u, out, stream):
    """wsum [w, x64] * [1, -1] into ``out``, then w += 0.05 * u: fresh host arrays per call, returned to be trashed."""
    L = len(numel)
    host = [(ctypes.c_uint64 * L)(*numel), (ctypes.c_int * 2)(code, F64), (ctypes.c_double * 2)(1.0, -1.0)]
    offs = np.cumsum([0] + numel[:-1])
    p_w = _native.ptr_array([w.data_ptr() + 2 * int(o) for o in offs])
    p_2 = _native.ptr_array([w.data_ptr() + 2 * int(o) for o in offs] + [x64.data_ptr() + 8 * int(o) for o in offs])
    host += [p_w, p_2]
    _native_promote.check(lib.fedagg_promote_wsum(p_2, host[1], 2, host[2], host[0], L, out.data_ptr(), stream),
                          "flat_promote_wsum")
    _native_promote.check(lib.fedagg_promote_increment(p_w, code, host[0], L, u.data_ptr(), 0.05, stream),
                          "flat_promote_increment")
    return host


def _trash(host):
    for arr in host:
        for i in range(len(arr)):
            arr[i] = 0


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_promote_ops_ordered_on_a_side_stream(kind):
    """The inputs are produced by kernels on a non-blocking side stream; the calls follow on that
    stream and only that stream is synchronised."""
    assert torch.cuda.is_available()
    lib = _native_promote.load()
    dtype, code, numel, total, data = _stream_case(kind)
    w_src, u_src, x_src, ref_inc, ref_ws = data[0]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    with torch.cuda.stream(side):
        w = torch.empty_like(w_src)
        u, x64, out = torch.empty_like(u_src), torch.empty_like(x_src), _flat64(total)
        for _ in range(8):  # the producers: a chain of kernels the calls must wait for
            w.copy_(w_src.flip(0)), u.copy_(u_src.flip(0)), x64.copy_(x_src.flip(0))
        w.copy_(w_src), u.copy_(u_src), x64.copy_(x_src)
        _calls(lib, code, numel, w, x64, u, out, side.cuda_stream)
        side.synchronize()  # no device-wide synchronisation
        assert pr.same_bits(out[:total].cpu(), ref_ws) == 0
        assert pr.same_bits(w.cpu(), ref_inc) == 0
        assert bool((out.view(torch.int64)[total:] == SENTINEL64).all())
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_promote_ops_capture_and_replay(kind):
    """A single-stream, linear graph: nothing runs while capturing, the host arrays may go once the
    calls have returned, and a replay over new data in the same buffers gives that data's bits."""
    assert torch.cuda.is_available()
    lib = _native_promote.load()
    dtype, code, numel, total, data = _stream_case(kind)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    sp = side.cuda_stream
    with torch.cuda.stream(side):
        w = torch.full((total,), SENTINEL, dtype=torch.int16, device="cuda").view(dtype)
        u, x64, out = _flat64(total)[:total].clone(), _flat64(total)[:total].clone(), _flat64(total)

        def prepare(ds):
            w.copy_(data[ds][0]), u.copy_(data[ds][1]), x64.copy_(data[ds][2])
            out.view(torch.int64).fill_(SENTINEL64)

        def check(ds, stage):
            assert pr.same_bits(out[:total].cpu(), data[ds][4]) == 0, stage
            assert pr.same_bits(w.cpu(), data[ds][3]) == 0, stage
            assert bool((out.view(torch.int64)[total:] == SENTINEL64).all()), stage

        prepare(0)
        host = _calls(lib, code, numel, w, x64, u, out, sp)  # eager first: also loads the code object
    side.synchronize()
    check(0, "eager")
    _trash(host)

    with torch.cuda.stream(side):
        prepare(0)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        host = _calls(lib, code, numel, w, x64, u, out, sp)
    torch.cuda.synchronize()
    assert bool((out.view(torch.int64) == SENTINEL64).all())  # captured, not run
    assert torch.equal(pr.as_bits(w), pr.as_bits(data[0][0]))
    _trash(host)
    del host
    gc.collect()
    for ds in (1, 0):
        with torch.cuda.stream(side):
            prepare(ds)
            graph.replay()
        torch.cuda.synchronize()
        check(ds, f"replay over data set {ds}")
    del graph
