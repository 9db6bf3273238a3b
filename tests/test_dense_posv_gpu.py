"""The symmetry test and the Cholesky solve of libfedagg_dense.so (include/fedagg_dense.h,
``fedagg_dense_symcopy_f64`` and ``fedagg_dense_potrs_f64``; substrafl_amd/csrc/dense_posv.hip), the
pieces behind ``accelerate(NewtonRaphson, solve="cholesky")`` next to ``fedagg_dense_potrf_f64``.

u = 2^-53, gamma_n = n u / (1 - n u).  Sizes: those of the Cholesky tests (``_potrf_sizes``).

  * an exact family, ``_exact_rhs``: the integer L of ``_exact_factor``, an integer x in [-2, 2],
    y = L^T x and b = L y.  Every partial sum of either substitution is a small integer in any
    order and every quotient is exact, so x has one right value and is compared with
    ``np.array_equal`` -- these matrices are conditioned up to 1e16, nothing inexact passes;
  * the bound families of the Cholesky tests with a standard normal b, held to Higham's thm 10.4,
    |b - A x| <= gamma_{3n+3} |L| |L^T| |x| (L the device's factor; two units of the 3n + 3 are for
    the test's own products, the residual itself is exact), and to eta <= n u, the LU tests' gate;
  * ``symcopy`` against ``np.array_equal(A, A.T)``, one ulp, NaN and signed-zero cases.

Every buffer lies between guard bands and is pre-filled, wherever the library has nothing to write,
with a NaN bit pattern that must come back bit for bit: the padding of the rows, the strict upper
triangle of d_L, the whole of d_A and, for ``potrs`` alone, the whole of d_L.
"""

import ctypes
import functools
import gc
import json
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from test_dense_potrf_gpu import (BOUND_FAMILIES, GUARD, INFO_FILL, LARGE, NAN_BITS, _bits, _bound_matrix, _exact_factor,
                                  _potrf_sizes)
from test_dense_solve_gpu import U, _gamma, _scaled_ints

gpu = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
ETA_RECORD = ROOT / "profiles" / "dense_posv_eta.json"
TILE = 64  # the symmetry test's tile (fedagg_dense_blocking's tile_m == tile_n, asserted on the device)


@functools.lru_cache(maxsize=None)
def _exact_rhs(n, seed=0):
    """``(L, x, b)`` of the exact family, built once per size and read-only."""
    L = _exact_factor(n)[1]
    x = np.random.default_rng([n, seed, 7]).integers(-2, 3, n).astype(np.float64)
    y = L.T @ x  # integers below 2 (2 n + 2): exact in any order
    b = L @ y
    assert np.all(b == np.round(b)) and np.abs(b).max() < 2.0 ** 40
    x.flags.writeable = b.flags.writeable = False
    return L, x, b


def _residual(A, x, b):
    """|b - A x| per row, the residual computed exactly (integers scaled by powers of two) and
    rounded once."""
    n = A.shape[0]
    ai, ae = _scaled_ints(A)
    xi, xe = _scaled_ints(x)
    bi, be = _scaled_ints(b)
    sa, sb = Fraction(2) ** (ae + xe), Fraction(2) ** be
    return np.array([float(abs(Fraction(bi[i]) * sb - Fraction(sum(p * q for p, q in zip(ai[i * n:(i + 1) * n], xi))) * sa))
                     for i in range(n)])


def _eta(A, x, b, r):
    return r.max() / (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max())


def _lapack_solve(A, b):
    """``(L, x)`` of LAPACK's Cholesky solve (scipy's ``cho_solve`` where it imports; else NumPy's
    factor with two triangular systems through ``np.linalg.solve``)."""
    L = np.linalg.cholesky(A)
    try:
        from scipy.linalg import cho_solve
    except ImportError:
        return L, np.linalg.solve(L.T, np.linalg.solve(L, b))
    return L, cho_solve((L, True), b)


class Dev:
    """The three calls on torch-owned device buffers with guard bands on both sides."""

    def __init__(self):
        import torch

        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        from substrafl_amd import _native_dense

        self.torch = torch
        self.lib = _native_dense.load()
        self.check = _native_dense.check
        assert _native_dense.blocking()[1:] == (TILE, TILE)

    @staticmethod
    def images(n, lda, ldl, A=None, L=None, b=None):
        """The host images as uint64 bits, [guard | body | guard] each: ``A`` whole, ``L``'s lower
        triangle, ``b``; the NaN pattern everywhere else and for what is not given."""
        guard = np.full(GUARD, NAN_BITS, np.uint64)
        a = np.full((n, lda), NAN_BITS, np.uint64)
        if A is not None:
            a[:, :n] = _bits(A)
        l = np.full((n, ldl), NAN_BITS, np.uint64)
        if L is not None:
            low = np.tril(np.ones((n, n), bool))
            l[:, :n][low] = _bits(L)[low]
        v = np.full(n, NAN_BITS, np.uint64) if b is None else _bits(b).copy()
        return {k: np.concatenate([guard, body.reshape(-1), guard]) for k, body in (("A", a), ("L", l), ("b", v))}

    def enqueue(self, ops, d, n, lda, ldl, stream):
        """``ops`` in order on ``stream``: "symcopy" (A -> flag, L), "symtest" (A -> flag, d_L = NULL),
        "potrf" (L -> L, info), "potrs" (L, b -> b)."""
        vp = ctypes.c_void_p
        pA, pL, pb = (vp(d[k].data_ptr() + 8 * GUARD) for k in ("A", "L", "b"))
        p_flag, p_info, sp = vp(d["int"].data_ptr() + 4 * GUARD), vp(d["int"].data_ptr() + 4 * GUARD + 4), vp(stream.cuda_stream)
        for op in ops:
            if op == "symcopy":
                self.check(self.lib.fedagg_dense_symcopy_f64(pA, n, lda, pL, ldl, p_flag, sp), op)
            elif op == "symtest":
                self.check(self.lib.fedagg_dense_symcopy_f64(pA, n, lda, None, 0, p_flag, sp), op)
            elif op == "potrf":
                self.check(self.lib.fedagg_dense_potrf_f64(pL, n, ldl, p_info, sp), op)
            else:
                assert op == "potrs"
                self.check(self.lib.fedagg_dense_potrs_f64(pL, n, ldl, pb, sp), op)

    def upload(self, images):
        d = {k: self.torch.from_numpy(v.view(np.int64)).cuda() for k, v in images.items()}
        d["int"] = self.torch.full((2 * GUARD + 2,), INFO_FILL, dtype=self.torch.int32, device="cuda")  # flag, info
        return d

    @staticmethod
    def result(ops, images, d, n, lda, ldl):
        """``flag``, ``info`` (INFO_FILL where no call wrote one), ``L`` (lower triangle, zeros above), ``x``
        and ``intact``: every bit that no call of ``ops`` may write is what it was."""
        out = {k: d[k].cpu().numpy().view(np.uint64) for k in ("A", "L", "b")}
        oi = d["int"].cpu().numpy()
        body = out["L"][GUARD:GUARD + n * ldl].reshape(n, ldl)
        was = images["L"][GUARD:GUARD + n * ldl].reshape(n, ldl)
        outside = np.ones((n, ldl), bool)
        if "symcopy" in ops or "potrf" in ops:
            outside[:, :n] = ~np.tril(np.ones((n, n), bool))
        intact = (np.array_equal(out["A"], images["A"]) and np.array_equal(body[outside], was[outside])
                  and np.array_equal(out["L"][:GUARD], images["L"][:GUARD])
                  and np.array_equal(out["L"][GUARD + n * ldl:], images["L"][GUARD + n * ldl:])
                  and np.array_equal(out["b"][:GUARD], images["b"][:GUARD])
                  and np.array_equal(out["b"][GUARD + n:], images["b"][GUARD + n:])
                  and ("potrs" in ops or np.array_equal(out["b"], images["b"]))
                  and bool(np.all(oi[:GUARD] == INFO_FILL)) and bool(np.all(oi[GUARD + 2:] == INFO_FILL))
                  and ("symcopy" in ops or "symtest" in ops or oi[GUARD] == INFO_FILL)
                  and ("potrf" in ops or oi[GUARD + 1] == INFO_FILL))
        return {"flag": int(oi[GUARD]), "info": int(oi[GUARD + 1]), "L": np.tril(body[:, :n].view(np.float64)),
                "x": out["b"][GUARD:GUARD + n].view(np.float64).copy(), "intact": bool(intact)}

    def run(self, ops, n, A=None, L=None, b=None, lda=None, ldl=None, stream=None, fill_on_stream=False):
        """``fill_on_stream``: the operands reach their buffers by device copies enqueued on
        ``stream`` directly before the library calls (nothing synchronises in between)."""
        torch = self.torch
        lda, ldl = lda or n, ldl or n
        images = self.images(n, lda, ldl, A, L, b)
        src = self.upload(images)
        torch.cuda.synchronize()
        st = stream if stream is not None else torch.cuda.current_stream()
        if fill_on_stream:
            d = {k: torch.zeros_like(v) for k, v in src.items()}  # what calls that ran ahead of the copies would read
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                for k in d:
                    d[k].copy_(src[k], non_blocking=True)
        else:
            d = src
        self.enqueue(ops, d, n, lda, ldl, st)
        st.synchronize()
        torch.cuda.synchronize()
        return self.result(ops, images, d, n, lda, ldl)


@pytest.fixture(scope="module")
def dev():
    return Dev()


POSV = ("symcopy", "potrf", "potrs")


# ------------------------------------------------------------------ 1. the exact family
@gpu
def test_exact_family(dev):
    for n in _potrf_sizes():
        A = _exact_factor(n)[0]
        L, x, b = _exact_rhs(n)
        for ops, kw in ((("potrs",), {"L": L}), (("potrs",), {"L": L, "ldl": n + 5}), (("potrf", "potrs"), {"L": A}),
                        (POSV, {"A": A}), (POSV, {"A": A, "lda": n + 3, "ldl": n + 5})):
            out = dev.run(ops, n, b=b, **kw)
            assert out["intact"], (n, ops, kw.keys())
            assert out["info"] == (0 if "potrf" in ops else INFO_FILL) and out["flag"] == (0 if "symcopy" in ops else INFO_FILL)
            assert np.array_equal(out["x"], x), (n, ops, np.flatnonzero(out["x"] != x)[:4])
            if "potrf" in ops:
                assert np.array_equal(out["L"], L), (n, ops)


# ------------------------------------------------------------------ 2. the componentwise bound
_record = {}


@gpu
@pytest.mark.parametrize("family", BOUND_FAMILIES)
def test_solution_bounds(dev, family):
    worst = {"componentwise_device": 0.0, "componentwise_lapack": 0.0, "eta_device_u": 0.0, "eta_lapack_u": 0.0}
    for n in _potrf_sizes():
        A = _bound_matrix(family, n)
        b = np.random.default_rng([BOUND_FAMILIES.index(family), n, 3]).standard_normal(n)
        out = dev.run(POSV, n, A=A, b=b)
        assert out["intact"] and out["flag"] == 0 and out["info"] == 0, (family, n, out["flag"], out["info"])
        figures = {}
        for who, (L, x) in (("device", (out["L"], out["x"])), ("lapack", _lapack_solve(A, b))):
            r = _residual(A, x, b)
            bound = _gamma(3 * n + 3) * (np.abs(L) @ (np.abs(L).T @ np.abs(x)))
            figures[who] = (float((r / bound).max()), float(_eta(A, x, b, r) / U), r, bound)
            worst[f"componentwise_{who}"] = max(worst[f"componentwise_{who}"], figures[who][0])
            worst[f"eta_{who}_u"] = max(worst[f"eta_{who}_u"], figures[who][1])
        print(f"{family} n={n}: |r| / bound device {figures['device'][0]:.4f} lapack {figures['lapack'][0]:.4f}; "
              f"eta device {figures['device'][1]:.2f} u lapack {figures['lapack'][1]:.2f} u, gate {n} u")
        ratio, eta_u, r, bound = figures["device"]
        assert np.all(r <= bound), (family, n, ratio)
        assert eta_u <= n, (family, n, eta_u)
    _record[family] = worst


@gpu
def test_eta_record():
    """The record of the worst ratios per family (device and LAPACK); no second gate."""
    if len(_record) != len(BOUND_FAMILIES):
        return  # the bound cases did not all run in this session: the record is left as it is
    ETA_RECORD.write_text(json.dumps({
        "what": "worst over the sizes of |b - A x| / (gamma_{3n+3} |L| |L^T| |x|) and of eta / u, u = 2^-53",
        "sizes": _potrf_sizes(), "families": _record}, indent=1, sort_keys=True) + "\n")


# ------------------------------------------------------------------ 3. symcopy
def _one_ulp_positions(n):
    """Off-diagonal (i, j), i > j: the corners, the last partial tile, and pairs whose two halves
    lie in different tiles."""
    last = (n - 1) // TILE * TILE  # first row and column of the last tile
    cand = {(1, 0), (n - 1, 0), (n - 1, n - 2), (n - 1, last), (last + 1, last), (TILE, TILE - 1), (TILE + 6, 3),
            (n - 1, TILE - 1), (2 * TILE + 1, TILE)}
    return sorted((i, j) for i, j in cand if 0 <= j < i < n)


@gpu
def test_symcopy_flag_and_copy(dev):
    for n in _potrf_sizes():
        A = _bound_matrix("gram_half_l2", n)
        assert np.array_equal(A, A.T)
        for kw in ({}, {"lda": n + 3, "ldl": n + 5}):
            out = dev.run(("symcopy",), n, A=A, **kw)
            assert out["intact"] and out["flag"] == 0, (n, kw)
            assert np.array_equal(_bits(out["L"]), _bits(np.tril(A))), (n, kw)
        only = dev.run(("symtest",), n, A=A)  # d_L = NULL: its buffer keeps every bit
        assert only["intact"] and only["flag"] == 0, n
        for i, j in _one_ulp_positions(n):
            for r, c in ((i, j), (j, i)):  # the element below the diagonal, then the one above
                B = A.copy()
                B[r, c] = np.nextafter(B[r, c], np.inf)
                assert not np.array_equal(B, B.T)
                out = dev.run(("symcopy",), n, A=B)
                assert out["intact"] and out["flag"] == 1, (n, r, c, out["flag"])
                assert np.array_equal(_bits(out["L"]), _bits(np.tril(B))), (n, r, c)  # copied whatever the flag
            B = A.copy()
            B[i, j] = np.nextafter(B[i, j], np.inf)
            assert dev.run(("symtest",), n, A=B)["flag"] == 1, (n, i, j)


@gpu
def test_symcopy_nan_and_signed_zero(dev):
    """``np.array_equal(A, A.T)``'s rules: a NaN differs from itself, on the diagonal too, and
    -0.0 equals 0.0 (the copy keeps the sign bit)."""
    for n in _potrf_sizes():
        A = _bound_matrix("gram_half_l2", n)
        for d in sorted({0, n // 2, n - 1}):
            B = A.copy()
            B[d, d] = np.nan
            assert not np.array_equal(B, B.T)
            out = dev.run(("symcopy",), n, A=B)
            assert out["intact"] and out["flag"] == 1, (n, d)
        if n == 1:
            continue
        i, j = n - 1, (n - 1) // 2
        B = A.copy()
        B[i, j] = B[j, i] = np.nan
        out = dev.run(("symcopy",), n, A=B)
        assert out["intact"] and out["flag"] == 1, (n, "nan pair")
        B = A.copy()
        B[i, j], B[j, i] = 0.0, -0.0
        assert np.array_equal(B, B.T)
        out = dev.run(("symcopy",), n, A=B)
        assert out["intact"] and out["flag"] == 0, (n, "signed zero")
        assert np.array_equal(_bits(out["L"]), _bits(np.tril(B))), n
        B[i, j], B[j, i] = -0.0, 0.0
        out = dev.run(("symcopy",), n, A=B)
        assert out["flag"] == 0 and np.signbit(out["L"][i, j]), (n, "signed zero, the lower one negative")


# ------------------------------------------------------------------ 4. determinism and stream order
@gpu
def test_deterministic_and_ordered_by_the_stream(dev):
    n = LARGE
    A = _bound_matrix("gram_4n", n)
    b = np.random.default_rng([n, 4]).standard_normal(n)
    first, again = dev.run(POSV, n, A=A, b=b), dev.run(POSV, n, A=A, b=b)
    side = dev.run(POSV, n, A=A, b=b, stream=dev.torch.cuda.Stream(), fill_on_stream=True)
    padded_side = dev.run(POSV, n, A=A, b=b, lda=n + 3, ldl=n + 5, stream=dev.torch.cuda.Stream(), fill_on_stream=True)
    for other in (again, side, padded_side):
        assert other["intact"] and first["intact"] and other["flag"] == first["flag"] == 0 and other["info"] == first["info"] == 0
        assert np.array_equal(_bits(other["L"]), _bits(first["L"])) and np.array_equal(_bits(other["x"]), _bits(first["x"]))
    L, x, bx = _exact_rhs(n)
    out = dev.run(POSV, n, A=_exact_factor(n)[0], b=bx, stream=dev.torch.cuda.Stream(), fill_on_stream=True)
    assert out["intact"] and out["flag"] == 0 and out["info"] == 0 and np.array_equal(out["x"], x)


@gpu
def test_graph_capture_runs_nothing_and_replays(dev):
    """The three calls captured into a graph on a side stream: nothing runs during the capture (the
    launch sequence is a function of n alone and nothing synchronises), and the replay solves
    whatever the buffers hold then, to the bits of the eager run."""
    torch = dev.torch
    n, lda, ldl = 129, 132, 134
    rng = np.random.default_rng([n, 5])
    data = {"A": (_bound_matrix("gram_4n", n), rng.standard_normal(n)), "B": (_exact_factor(n)[0], _exact_rhs(n)[2])}
    eager = {k: dev.run(POSV, n, A=a, b=b, lda=lda, ldl=ldl) for k, (a, b) in data.items()}
    assert np.array_equal(eager["B"]["x"], _exact_rhs(n)[1])
    images = {k: dev.images(n, lda, ldl, A=a, b=b) for k, (a, b) in data.items()}
    srcs = {k: dev.upload(v) for k, v in images.items()}
    d = {k: torch.empty_like(v) for k, v in srcs["A"].items()}
    side = torch.cuda.Stream()

    def fill(k):
        for name in d:
            d[name].copy_(srcs[k][name], non_blocking=True)

    with torch.cuda.stream(side):
        fill("A")
        dev.enqueue(POSV, d, n, lda, ldl, side)  # eager first: also loads the code object
    side.synchronize()
    assert np.array_equal(_bits(dev.result(POSV, images["A"], d, n, lda, ldl)["x"]), _bits(eager["A"]["x"]))

    with torch.cuda.stream(side):
        fill("A")
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        dev.enqueue(POSV, d, n, lda, ldl, side)
    torch.cuda.synchronize()
    assert all(torch.equal(d[name], srcs["A"][name]) for name in d), "a kernel ran during the capture"
    gc.collect()
    for k in ("B", "A"):
        with torch.cuda.stream(side):
            fill(k)
            graph.replay()
        torch.cuda.synchronize()
        out = dev.result(POSV, images[k], d, n, lda, ldl)
        assert out["intact"] and out["flag"] == 0 and out["info"] == 0, k
        assert np.array_equal(_bits(out["L"]), _bits(eager[k]["L"])) and np.array_equal(_bits(out["x"]), _bits(eager[k]["x"])), k


# ------------------------------------------------------------------ 5. non-finite values
@gpu
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf], ids=["nan", "+inf", "-inf"])
def test_non_finite_values_run_clean(dev, value):
    """NaN or Inf in b[0], b[n-1] or l_00: the call returns 0, the stream synchronises and nothing
    outside d_b is written.  The values are unspecified and not looked at, but for one: x[n-1] is
    b[n-1] less finite terms, divided twice, and cannot come out finite."""
    for n in (1, 33, 65, 129):
        L, x, b = _exact_rhs(n)
        for where in ("b0", "b_last", "l00"):
            Lv, bv = L.copy(), b.copy()
            if where == "b0":
                bv[0] = value
            elif where == "b_last":
                bv[n - 1] = value
            else:
                Lv[0, 0] = value
            out = dev.run(("potrs",), n, L=Lv, b=bv)  # check() has raised on any return code but 0
            assert out["intact"] and out["flag"] == INFO_FILL and out["info"] == INFO_FILL, (n, where, value)
            if where == "b_last":
                assert not np.isfinite(out["x"][n - 1]), (n, value)
