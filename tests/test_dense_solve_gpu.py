"""The opt-in device solve of NewtonRaphson's Newton system (include/fedagg_dense.h,
substrafl_amd/csrc/dense.hip; ``accelerate(NewtonRaphson, solve="device")``), held to the standard
error bounds of LU with partial pivoting rather than to LAPACK's bits.

u = 2^-53, gamma_n = n u / (1 - n u).  Sizes: {1, 2, 3, 17}, then T - 1, T, T + 1 and 2 T + 1 for
every distinct blocking size T the library reports (``fedagg_dense_blocking``), and 5 max(T) + 7.
Matrix families (seeded ``default_rng``): symmetric diagonally dominant (gen_golden_nr._hessian's
recipe), standard normal, normal with an exactly zero diagonal, normal with the diagonal scaled by
1e-12, normal with rows scaled by 10^[-6, 6]; right-hand sides are fp32 values widened.

One case of that grid is singular by construction: n = 1 with an exactly zero diagonal is the
matrix [0].  There the tests assert what the contract says of a zero pivot (``info == 1``, no
fault) instead of an error bound on a solution that does not exist.

Next to the bounds stands a family whose answers are exact: ``_exact_system`` builds A = P^T L U
from factors for which every step of the elimination and of the substitutions is exact in fp64
whatever the order of the sums, so ``ipiv``, the stored factors and x have one right value each
and are compared with ``np.array_equal``, no tolerance.  It runs at every size above and at the
two sizes at which the panel kernel's strided loops first take another pass (``_large_sizes``:
search stride + 2 T + 1 and scale stride + 2 T + 1, read from dense.hip), where the five
families and their bounds run as well.
"""

import ctypes
import functools
import json
import re
import shutil
import subprocess
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import standin_substrafl.strategies as ss
from standin_substrafl.strategies import schemas as sch

from oracle import newton_raphson_sums

gpu = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
D = ROOT / "tests" / "golden"
ETA_RECORD = ROOT / "profiles" / "dense_solve_eta.json"
U = 2.0 ** -53
FAMILIES = ("spd_dominant", "normal", "zero_diagonal", "tiny_diagonal", "row_scaled")
GUARD = 64  # elements of guard band behind every buffer


def _blocking():
    from substrafl_amd import _native_dense

    return _native_dense.blocking()


def _sizes():
    ts = sorted(set(_blocking()))
    out = {1, 2, 3, 17, 5 * max(ts) + 7}
    for t in ts:
        out |= {t - 1, t, t + 1, 2 * t + 1}
    assert max(out) <= 800
    return sorted(out)


def _gamma(n):
    return n * U / (1.0 - n * U)


def _matrix(family, n, seed=0):
    rng = np.random.default_rng([FAMILIES.index(family), n, seed])
    a = rng.standard_normal((n, n))
    if family == "spd_dominant":
        a = (a + a.T) * 0.5 + np.eye(n) * (n + 1.0)
    elif family == "zero_diagonal":
        a[np.diag_indices(n)] = 0.0
    elif family == "tiny_diagonal":
        a[np.diag_indices(n)] *= 1e-12
    elif family == "row_scaled":
        a *= 10.0 ** rng.uniform(-6, 6, (n, 1))
    g = rng.standard_normal(n).astype(np.float32).astype(np.float64)
    return np.ascontiguousarray(a), g


def _singular_by_construction(family, n):
    return family == "zero_diagonal" and n == 1


# ------------------------------------------------------------------ the panel kernel's strides
DENSE_SRC = ROOT / "substrafl_amd" / "csrc" / "dense.hip"


@functools.lru_cache(maxsize=None)
def _strides():
    """The strides of ``dense_panel_f64``'s loops over one column, read from the source so that a
    re-tune moves the sizes below (or fails here, where a define or a loop is gone):
    ``panel`` DN_NB; ``search`` rows between two visits of one thread in the column-0 pivot search
    (DN_PANEL_THREADS); ``scale`` the same for one iteration of the scale pass (its unroll factor
    times DN_PANEL_THREADS); ``track`` for the rank-1 update, which carries the search of the
    other columns (DN_RG * DN_UB)."""
    src = DENSE_SRC.read_text()

    def define(name, known=()):
        m = re.search(rf"^#define[ \t]+{name}[ \t]+(.+?)[ \t]*(?://.*)?$", src, re.M)
        assert m, f"dense.hip no longer defines {name}"
        text = m.group(1)
        for k, v in known:
            text = re.sub(rf"\b{k}\b", str(v), text)
        m = re.fullmatch(r"\(?\s*(\d+)\s*(?:/\s*(\d+))?\s*\)?", text)
        assert m, f"dense.hip: {name} is no longer an integer or a quotient of two ({text!r})"
        return int(m.group(1)) // int(m.group(2) or 1)

    threads = define("DN_PANEL_THREADS")
    out = {"panel": define("DN_NB"), "search": threads,
           "track": define("DN_RG", [("DN_PANEL_THREADS", threads)]) * define("DN_UB")}
    # the column-0 search: for (dn_u64 i = j + t; i < n; i += DN_PANEL_THREADS)
    assert len(re.findall(r"for \(dn_u64 i = j \+ t; i < n; i \+= DN_PANEL_THREADS\)", src)) == 1, "the search loop"
    # the scale pass: for (dn_u64 i0 = jc + 1 + t; i0 < n; i0 += 4 * DN_PANEL_THREADS)
    m = re.findall(r"for \(dn_u64 i0 = jc \+ 1 \+ t; i0 < n; i0 \+= (\d+) \* DN_PANEL_THREADS\)", src)
    assert len(m) == 1, "the scale loop"
    out["scale"] = int(m[0]) * threads
    return out


def _large_sizes():
    """The smallest sizes that reach the code the advertised sizes run: S + 2 T + 1 (a thread of
    the column-0 search takes a second row in the first three panels) and Q + 2 T + 1 (the scale
    pass iterates twice in the first two panels, the search's unrolled body runs), both with a
    last panel and a last trailing tile one wide."""
    s = _strides()
    T, S, Q = s["panel"], s["search"], s["scale"]
    small, large = S + 2 * T + 1, Q + 2 * T + 1
    assert small < large and large - 1 > Q and large - 1 > 3 * S  # the unrolled search body: n - j > 3 S
    return [small, large]


# ------------------------------------------------------------------ the exact-arithmetic family
def _exact_system(n, seed=0, zero_at=None, last_row_stays=False):
    """``(A, b, L, U, perm, x)`` with A = (L U)[perm] and b = A x, every value a small multiple of
    1/4, such that LU with partial pivoting is exact in fp64 at every step:
    every Schur complement is L[:, k:] @ U[k:, :], whose partial sums in any order are multiples
    of 1/4 below 4 n + 4 in magnitude; each multiplier is (l_ij u_jj) / u_jj, an exact quotient; and
    |l_ij| <= 1/2 < 1 makes the pivot of step j unique, the row that holds row j of L U.  The
    substitutions are exact for the same reason (y = U x are integers, x the exact quotients).
    ``zero_at``: u_jj = 0 there (the first zero pivot).  ``last_row_stays``: the last row of A is
    the last row of L U, so that no interchange before the last step touches it."""
    rng = np.random.default_rng([n, seed])
    L = np.tril(rng.choice([-0.5, -0.25, 0.0, 0.0, 0.25, 0.5], (n, n)), -1) + np.eye(n)
    U = np.triu(rng.integers(-3, 4, (n, n)).astype(np.float64), 1)
    U[np.diag_indices(n)] = rng.choice([-5., -4., -3., 3., 4., 5., 7.], n)
    perm = rng.permutation(n)
    if zero_at is not None:
        U[zero_at, zero_at] = 0.0
    if last_row_stays:
        k = int(np.flatnonzero(perm == n - 1)[0])
        perm[[k, n - 1]] = perm[[n - 1, k]]
    A = np.ascontiguousarray((L @ U)[perm])  # row r of A is row perm[r] of L U
    x = rng.integers(-8, 9, n).astype(np.float64)
    b = A @ x
    return A, b, L, U, perm, x


def _expected_ipiv(perm):
    """LAPACK's ``ipiv`` (0-based) for A = (L U)[perm] when the pivot of step j is the row that
    holds row j of L U: ``pos[k]`` is where row k of L U sits now, ``cur`` its inverse."""
    n = len(perm)
    cur = [int(p) for p in perm]
    pos = [0] * n
    for r, k in enumerate(cur):
        pos[k] = r
    ipiv = np.empty(n, np.int32)
    for j in range(n):
        p = pos[j]
        ipiv[j] = p
        k = cur[j]  # the row of L U that gives up position j
        cur[p], pos[k] = k, p
        cur[j], pos[j] = j, j
    return ipiv


def _cpu_replay(A, b):
    """``(LU, ipiv, x)`` of LU with partial pivoting (first row of largest magnitude) on the host:
    LAPACK's getrf / getrs where scipy imports, else a plain NumPy elimination up to n = 65, else
    None."""
    n = A.shape[0]
    try:
        from scipy.linalg import lu_factor, lu_solve
    except ImportError:
        if n > 65:
            return None
        W, y, ipiv = A.copy(), b.copy(), np.empty(n, np.int32)
        for j in range(n):
            p = j + int(np.argmax(np.abs(W[j:, j])))
            ipiv[j] = p
            W[[j, p]] = W[[p, j]]
            y[[j, p]] = y[[p, j]]
            if W[j, j] != 0:
                W[j + 1:, j] /= W[j, j]
                W[j + 1:, j + 1:] -= np.outer(W[j + 1:, j], W[j, j + 1:])
        for i in range(n):
            y[i] -= W[i, :i] @ y[:i]
        for i in range(n - 1, -1, -1):
            y[i] = (y[i] - W[i, i + 1:] @ y[i + 1:]) / W[i, i]
        return W, ipiv, y
    lu, piv = lu_factor(A)
    return lu, piv.astype(np.int32), lu_solve((lu, piv), b)


@functools.lru_cache(maxsize=None)
def _exact_case(n, seed=0):
    """One system of the family with what must come out (``LU`` the stored factors, ``ipiv``),
    built once per size and read-only.  The host replay is asserted here, once per size, before
    any device result is compared: the reference's own correctness is part of the record."""
    A, b, L, U, perm, x = _exact_system(n, seed)
    c = {"A": A, "b": b, "L": L, "U": U, "perm": perm, "x": x, "LU": np.tril(L, -1) + U, "ipiv": _expected_ipiv(perm)}
    replay = _cpu_replay(A, b)
    if replay is not None:
        lu, piv, xs = replay
        assert np.array_equal(piv, c["ipiv"]), (n, seed, "host replay: ipiv")
        assert np.array_equal(lu, c["LU"]), (n, seed, "host replay: factors")
        assert np.array_equal(xs, x), (n, seed, "host replay: x")
    for v in c.values():
        v.flags.writeable = False
    return c


def _exact_sizes_cpu():
    s = _strides()
    T = s["panel"]
    # (no library here, so no fedagg_dense_blocking: 10 T + 7 is _sizes()' largest, 5 max(T) + 7, for 2 T tiles)
    return [1, 2, T - 1, T + 1, 2 * T + 1, 10 * T + 7] + _large_sizes()


def test_strides_are_read_from_the_source():
    s = _strides()
    assert s["scale"] % s["search"] == 0 and s["scale"] > s["search"] > s["panel"] > 1 and s["track"] > 1
    for n in _large_sizes():
        assert n % s["panel"] == 1  # the last panel is one column wide


@pytest.mark.parametrize("n", _exact_sizes_cpu())
def test_exact_family_on_the_host(n):
    """The family's claim, without a GPU: the constructed factors, the interchanges that follow
    from ``perm`` alone and x are, bit for bit, what LU with partial pivoting gives on the host."""
    replay = _cpu_replay(*_exact_system(n)[:2])
    if replay is None:
        n = 65  # no LAPACK here: the plain elimination, at the largest size it is quick at
        replay = _cpu_replay(*_exact_system(n)[:2])
    c = _exact_case(n)  # asserts the replay as well; here each part by name
    lu, piv, xs = replay
    assert np.array_equal(piv, c["ipiv"]) and np.array_equal(lu, c["LU"]) and np.array_equal(xs, c["x"])
    # multiples of 1/4, at most 7 (one term with l = 1) + 3.5 (n - 1) in magnitude
    assert np.all(c["A"] * 4 == np.round(c["A"] * 4)) and np.abs(c["A"]).max() <= 7 + 3.5 * (n - 1)
    # the bookkeeping against the definition: the interchanges put the rows in the order of L U
    assert np.array_equal(_apply_pivots(c["A"], c["ipiv"]), c["L"] @ c["U"])


class Dev:
    """The library on torch-owned device buffers: every buffer is followed by a guard band."""

    def __init__(self):
        import torch

        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        from substrafl_amd import _native_dense

        self.torch = torch
        self.lib = _native_dense.load()
        self.check = _native_dense.check

    def run(self, A, b=None, lda=None, stream=None, fill_on_stream=False, what="solve", ipiv=None):
        """Factor (and with ``b`` solve) on the device.  Returns a dict: LU (n x n), ipiv, info, x,
        and ``intact``: whether the padding of every row and every guard band kept its bits.
        ``fill_on_stream``: A reaches its buffer by a device copy enqueued on ``stream`` directly
        before the library call (nothing synchronises in between).
        ``what="getrs"``: A holds factors and ``ipiv`` their interchanges, both made on the host;
        only ``fedagg_dense_getrs_f64`` runs, and ``intact`` then also says that the factors, the
        interchanges and the ``info`` slot kept their bits."""
        torch = self.torch
        n = A.shape[0]
        lda = n if lda is None else lda
        host = np.full((n, lda), np.nan)
        host[:, :n] = A
        guard = np.full(GUARD, -7.25)
        hA = np.concatenate([host.reshape(-1), guard])
        hb = np.concatenate([b if b is not None else np.zeros(n), guard])
        dA_src = torch.from_numpy(hA).cuda()
        db = torch.from_numpy(hb).cuda()
        di = torch.full((n + 1 + GUARD,), -77, dtype=torch.int32, device="cuda")  # ipiv, info, guard
        ws = int(self.lib.fedagg_dense_ws_bytes(n))
        dws = torch.full((ws // 8 + GUARD,), -7.25, dtype=torch.float64, device="cuda")
        assert (what == "getrs") == (ipiv is not None)
        if ipiv is not None:
            di[:n] = torch.from_numpy(np.array(ipiv, np.int32)).cuda()
        torch.cuda.synchronize()
        st = stream if stream is not None else torch.cuda.current_stream()
        if fill_on_stream:
            dA = torch.full_like(dA_src, 3.0)  # what a solve that ran ahead of the copy would factor
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                dA.copy_(dA_src, non_blocking=True)
        else:
            dA = dA_src
        vp = ctypes.c_void_p
        sp = vp(st.cuda_stream)
        p_i, p_info = vp(di.data_ptr()), vp(di.data_ptr() + 4 * n)
        if what == "solve":
            self.check(self.lib.fedagg_dense_solve_f64(vp(dA.data_ptr()), n, lda, p_i, p_info, vp(db.data_ptr()),
                                                       vp(dws.data_ptr()), sp), "solve")
        elif what == "getrs":
            self.check(self.lib.fedagg_dense_getrs_f64(vp(dA.data_ptr()), n, lda, p_i, vp(db.data_ptr()), sp), "getrs")
        else:
            self.check(self.lib.fedagg_dense_getrf_f64(vp(dA.data_ptr()), n, lda, p_i, p_info, vp(dws.data_ptr()), sp),
                       "getrf")
            if b is not None:
                self.check(self.lib.fedagg_dense_getrs_f64(vp(dA.data_ptr()), n, lda, p_i, vp(db.data_ptr()), sp), "getrs")
        st.synchronize()
        torch.cuda.synchronize()
        oA, ob, oi, ows = dA.cpu().numpy(), db.cpu().numpy(), di.cpu().numpy(), dws.cpu().numpy()
        full = oA[: n * lda].reshape(n, lda)
        same = lambda a, r: np.array_equal(np.asarray(a).view(np.uint8), np.asarray(r).view(np.uint8))  # noqa: E731
        intact = (same(full[:, n:], host[:, n:]) and same(oA[n * lda:], guard) and same(ob[n:], guard)
                  and same(oi[n + 1:], np.full(GUARD, -77, np.int32)) and same(ows, np.full(ws // 8 + GUARD, -7.25)))
        if what == "getrs":
            intact = (intact and same(full[:, :n], host[:, :n]) and same(oi[:n], np.asarray(ipiv, np.int32))
                      and int(oi[n]) == -77)
        return {"LU": full[:, :n].copy(), "ipiv": oi[:n].copy(), "info": int(oi[n]), "x": ob[:n].copy(),
                "intact": intact}


@pytest.fixture(scope="module")
def dev():
    return Dev()


def _bits(a):
    a = np.asarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _apply_pivots(A, ipiv):
    PA = A.copy()
    for j, p in enumerate(ipiv):
        if p != j:
            PA[[j, p]] = PA[[p, j]]
    return PA


# ------------------------------------------------------------------ exact residual
def _scaled_ints(a):
    """``(ints, e)`` with ``a[k] == ints[k] * 2**e`` exactly (every double is a dyadic rational)."""
    a = np.asarray(a, np.float64).reshape(-1)
    m, e = np.frexp(a)
    mi = np.ldexp(m, 53).astype(np.int64)  # exact: 53 significant bits
    e = e.astype(np.int64) - 53
    nz = mi != 0
    emin = int(e[nz].min()) if nz.any() else 0
    return [int(v) << int(s - emin) if v else 0 for v, s in zip(mi.tolist(), e.tolist())], emin


def backward_error(H, x, g):
    """eta(x) = ||g - H x||inf / (||H||inf ||x||inf + ||g||inf), the residual computed exactly
    (integers scaled by powers of two, combined as ``fractions.Fraction``) and rounded once."""
    n = H.shape[0]
    hi, he = _scaled_ints(H)
    xi, xe = _scaled_ints(x)
    gi, ge = _scaled_ints(g)
    two = Fraction(2)
    sh, sg = two ** (he + xe), two ** ge
    r = 0.0
    for i in range(n):
        row = hi[i * n:(i + 1) * n]
        r = max(r, float(abs(Fraction(gi[i]) * sg - Fraction(sum(a * b for a, b in zip(row, xi))) * sh)))
    den = np.abs(H).sum(axis=1).max() * np.abs(x).max() + np.abs(g).max()
    return r / den


def test_backward_error_helper_is_exact():
    H = np.array([[1.0, 2.0 ** -60], [3.0, 1e-300]])
    x = np.array([1.0, 2.0 ** 60])
    g = np.array([2.0, 3.0])  # row 0: residual exactly 0 (float64 would round 1 + 1 - 2 fine, but row 1 not)
    r1 = Fraction(3) - Fraction(3) - Fraction(1e-300) * Fraction(2.0 ** 60)
    den = max(1.0 + 2.0 ** -60, 3.0 + 1e-300) * 2.0 ** 60 + 3.0
    assert backward_error(H, x, g) == float(abs(r1)) / den


# ------------------------------------------------------------------ 1. factorisation
def _check_factorisation(dev, family, n):
    """The header's gates on one factorisation: ``info``, ``ipiv`` in range, multipliers <= 1,
    |P A - L U| <= 3 gamma_n |L| |U|, and up to n = 65 the first row of largest magnitude."""
    A, _ = _matrix(family, n)
    out = dev.run(A, what="getrf")
    LU, ipiv = out["LU"], out["ipiv"]
    assert out["intact"], (family, n)
    assert out["info"] == (1 if _singular_by_construction(family, n) else 0), (family, n, out["info"])
    assert all(j <= int(p) < n for j, p in enumerate(ipiv)), (family, n)
    L = np.tril(LU, -1) + np.eye(n)
    Uf = np.triu(LU)
    assert np.all(np.abs(np.tril(LU, -1)) <= 1.0), (family, n, "a multiplier above 1: no pivoting")
    PA = _apply_pivots(A, ipiv)
    err = np.abs(PA - L @ Uf)
    bound = 3.0 * _gamma(n) * (np.abs(L) @ np.abs(Uf))
    worst = float((err - bound).max())
    assert np.all(err <= bound), (family, n, worst, np.unravel_index(np.argmax(err - bound), err.shape))
    # the pivot is the FIRST row of largest magnitude: replay the elimination on the host
    if n <= 65:
        W = A.copy()
        for j in range(n):
            p = j + int(np.argmax(np.abs(W[j:, j])))  # argmax returns the first maximum
            col = np.abs(W[j:, j])
            # the device's column differs from this replay by rounding only: accept any row that
            # is a maximum to within that rounding, and require the first one on exact ties
            if col.max() > 0 and np.sum(col >= col.max() * (1 - 1e-9)) == 1:
                assert int(ipiv[j]) == p, (family, n, j)
            q = int(ipiv[j])
            W[[j, q]] = W[[q, j]]
            if W[j, j] != 0:
                W[j + 1:, j] /= W[j, j]
                W[j + 1:, j + 1:] -= np.outer(W[j + 1:, j], W[j, j + 1:])


@gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_factorisation_bounds(dev, family):
    for n in _sizes():
        _check_factorisation(dev, family, n)


@gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_factorisation_bounds_at_the_stride_sizes(dev, family):
    """The same gates, unchanged, where the panel kernel's strided loops take further passes."""
    for n in _large_sizes():
        _check_factorisation(dev, family, n)


@gpu
def test_first_of_equal_pivots_is_taken(dev):
    """Exact ties in every column: a unit diagonal and one more +-1 further down, 1 to 300 rows
    away.  In the rank-1 update, which carries the search of a panel's columns 1 to 31 (a thread
    comes back every DN_RG * DN_UB = 128 rows), that is the same wave, another wave and another
    pass of the same thread.  In the column-0 search and in the scale pass (strides 512 and 2048)
    every thread makes one pass at this size: ``test_first_of_equal_pivots_far_apart`` reaches
    their further passes.  No row has an entry right of its diagonal, so nothing fills in: the
    first row of largest magnitude is the diagonal at every step, no rows move, and the factors
    are the matrix itself, exactly."""
    n = 5 * max(_blocking()) + 7
    assert 129 > _strides()["track"] and n <= _strides()["search"]
    _check_ties(dev, n, [1, 2, 70, 129, 300])


def _check_ties(dev, n, distances, shift_per_panel=0):
    """Column j takes ``distances[(j + shift_per_panel * panel index) % len]``: with a list whose
    length divides the panel width, a shift of 1 gives the panels' first columns every distance
    in turn instead of the first one always."""
    T = _strides()["panel"]
    A = np.eye(n)
    for j in range(n):
        d = distances[(j + shift_per_panel * (j // T)) % len(distances)]
        if j + d < n:
            A[j + d, j] = -1.0 if j % 2 else 1.0
    out = dev.run(A, what="getrf")
    assert out["info"] == 0 and out["intact"]
    assert np.array_equal(out["ipiv"], np.arange(n))
    assert np.array_equal(out["LU"], A)


@gpu
def test_first_of_equal_pivots_far_apart(dev):
    """The same construction at the larger stride size, the equal candidate up to one scale
    stride + 1 rows below the diagonal: a search thread meets it in its second or third pass
    (S + 1, 2 S + 6), and it lies beyond the first iteration of the scale pass (Q + 1; every
    pivot is 1 here, so that pass is run but cannot show: the exact family holds it).  The list
    has 8 entries and a panel 32 columns, so the distances shift by one per panel: column 0 of a
    panel, the only one the search of its own visits, then sees each of them.  A second run puts
    the equal candidate a whole number of search strides away, where the very thread that holds
    the diagonal comes back to it (a search that kept the last of two equal values shows here)."""
    s = _strides()
    T, S, Q = s["panel"], s["search"], s["scale"]
    n = _large_sizes()[-1]
    assert Q + 1 < n and T % 8 == 0 and Q % S == 0
    _check_ties(dev, n, [1, 2, 70, 129, 300, S + 1, 2 * S + 6, Q + 1], shift_per_panel=1)
    _check_ties(dev, n, [S, 2 * S, 3 * S, Q], shift_per_panel=1)


# ------------------------------------------------------------------ 2. solve
_eta = {}


def _check_solve(dev, family, n):
    """The header's gate on one solve, eta <= n u with the residual computed exactly; the device's
    and NumPy's eta go into the record."""
    A, g = _matrix(family, n)
    out = dev.run(A, g)
    assert out["intact"], (family, n)
    if _singular_by_construction(family, n):
        assert out["info"] == 1
        _eta[f"{family}/{n}"] = {"n": n, "singular": True}
        return
    assert out["info"] == 0
    eta_dev = backward_error(A, out["x"], g)
    eta_np = backward_error(A, np.linalg.solve(A, g), g)
    _eta[f"{family}/{n}"] = {"n": n, "eta_device_u": eta_dev / U, "eta_numpy_u": eta_np / U, "gate_u": n}
    print(f"{family} n={n}: eta device {eta_dev / U:.2f} u, numpy {eta_np / U:.2f} u, gate {n} u")
    assert eta_dev <= n * U, (family, n, eta_dev / U)
    # getrf + getrs is the same launch sequence as solve: the same bits
    two = dev.run(A, g, what="getrf+getrs")
    assert np.array_equal(_bits(two["x"]), _bits(out["x"])) and np.array_equal(_bits(two["LU"]), _bits(out["LU"]))


@gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_solve_backward_error(dev, family):
    for n in _sizes():
        _check_solve(dev, family, n)


@gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_solve_backward_error_at_the_stride_sizes(dev, family):
    """The same gate, unchanged, where the panel kernel's strided loops take further passes."""
    for n in _large_sizes():
        _check_solve(dev, family, n)


@gpu
def test_eta_record():
    """The record of the backward errors (device and ``np.linalg.solve``) per case; no second gate."""
    want = len(FAMILIES) * (len(_sizes()) + len(_large_sizes()))
    if len(_eta) != want:
        return  # the solve cases did not all run in this session: the record is left as it is
    ETA_RECORD.write_text(json.dumps({"unit": "u = 2^-53", "blocking": list(_blocking()), "cases": _eta}, indent=1,
                                     sort_keys=True) + "\n")


# ------------------------------------------------------------------ 2b. the exact family on the device
def _assert_exact(out, c, where):
    assert out["intact"], where
    assert out["info"] == 0, (where, out["info"])
    assert np.array_equal(out["ipiv"], c["ipiv"]), (where, "ipiv", np.flatnonzero(out["ipiv"] != c["ipiv"])[:4])
    bad = np.argwhere(out["LU"] != c["LU"])
    assert bad.size == 0, (where, "LU", len(bad), bad[:4].tolist())
    assert np.array_equal(out["x"], c["x"]), (where, "x", np.flatnonzero(out["x"] != c["x"])[:4])


@gpu
def test_exact_family_solve(dev):
    """``solve`` and ``getrf + getrs`` at every size: interchanges, stored factors and solution
    equal the constructed ones, by value and with no tolerance."""
    assert all(n % t for n in _large_sizes() for t in set(_blocking()))
    assert _strides()["panel"] == _blocking()[0]
    for n in _sizes() + _large_sizes():
        c = _exact_case(n)
        _assert_exact(dev.run(c["A"], c["b"]), c, (n, "solve"))
        _assert_exact(dev.run(c["A"], c["b"], what="getrf+getrs"), c, (n, "getrf+getrs"))


def _getrs_sizes():
    T = _strides()["panel"]
    return [1, T - 1, T, T + 1, 2 * T + 1, 5 * max(_blocking()) + 7] + _large_sizes()


@gpu
def test_exact_family_getrs_on_host_built_factors(dev):
    """``fedagg_dense_getrs_f64`` alone, on factors and interchanges the device never made: a
    convention that factorisation and substitution misread alike (the order of the interchanges,
    the unit diagonal) cannot cancel here."""
    for n in _getrs_sizes():
        c = _exact_case(n)
        if n > 2 * _strides()["panel"]:  # chained interchanges: some row takes part in two of them
            moved = np.flatnonzero(c["ipiv"] != np.arange(n))
            assert np.bincount(np.concatenate([moved, c["ipiv"][moved]]), minlength=n).max() >= 2, n
        out = dev.run(c["LU"], c["b"], what="getrs", ipiv=c["ipiv"])
        assert out["intact"], n  # the factors, the interchanges and the info slot kept their bits too
        assert np.array_equal(out["x"], c["x"]), (n, np.flatnonzero(out["x"] != c["x"])[:4])


@gpu
def test_exact_family_padded_and_on_a_side_stream(dev):
    for n in (5 * max(_blocking()) + 7, _large_sizes()[-1]):
        c = _exact_case(n)
        _assert_exact(dev.run(c["A"], c["b"], lda=n + 3), c, (n, "lda = n + 3"))
        _assert_exact(dev.run(c["A"], c["b"], stream=dev.torch.cuda.Stream(), fill_on_stream=True), c, (n, "side stream"))
        _assert_exact(dev.run(c["A"], c["b"], lda=n + 3, stream=dev.torch.cuda.Stream(), fill_on_stream=True), c,
                      (n, "lda = n + 3 on a side stream"))


@gpu
def test_exact_family_zero_pivot_keeps_the_finished_rows(dev):
    """u_jj = 0 in the constructed U: column j of the Schur complement is exactly zero at step j,
    so ``info == j + 1``, and the steps before j ran as they do without the zero: their
    interchanges and rows < j of the stored factors (finished, and touched by no later step) keep
    their exact values.  What lies from step j on is unspecified and not asserted."""
    T = _strides()["panel"]
    big = _large_sizes()[-1]
    for n, j in [(5 * max(_blocking()) + 7, T + 5), (big, (big // T - 1) * T + 5)]:  # (.., in the last full panel)
        assert T < j < n - 1
        A, b, L, Uc, perm, _ = _exact_system(n, 0, zero_at=j)
        assert Uc[j, j] == 0.0
        out = dev.run(A, b)
        assert out["intact"], (n, j)
        assert out["info"] == j + 1, (n, j, out["info"])
        assert np.array_equal(out["ipiv"][:j], _expected_ipiv(perm)[:j]), (n, j)
        assert np.array_equal(np.triu(out["LU"])[:j], Uc[:j]), (n, j, "rows < j of U")
        assert np.array_equal(np.tril(out["LU"], -1)[:j], np.tril(L, -1)[:j]), (n, j, "rows < j of L")


@gpu
def test_deterministic_at_the_larger_stride_size(dev):
    n = _large_sizes()[-1]
    A, g = _matrix("normal", n)
    first, again = dev.run(A, g), dev.run(A, g)
    for k in ("LU", "ipiv", "x"):
        assert np.array_equal(_bits(again[k]), _bits(first[k])), k
    assert first["info"] == again["info"] == 0 and first["intact"] and again["intact"]


# ------------------------------------------------------------------ 3. the reference's own outputs
class _Algo:
    pass


def _states(grads, hess, ns):
    return [sch.NewtonRaphsonSharedState(gradients=g, hessian=h, n_samples=n) for g, h, n in zip(grads, hess, ns)]


@gpu
def test_golden_updates_within_conditioning(dev):
    from substrafl_amd.engine import engine_for
    from substrafl_amd.integration import accelerate
    from substrafl_amd.integration import newton_raphson_sums as engine_sums

    NR = accelerate(ss.NewtonRaphson, solve="device")
    arrays = np.load(D / "golden_newton_raphson.npz", allow_pickle=False)
    meta = json.loads((D / "golden_newton_raphson_meta.json").read_text())
    for c in meta["cases"]:
        key, K, L = c["key"], c["K"], c["layers"]
        grads = [[arrays[f"{key}/k{k}/g{li}"] for li in range(L)] for k in range(K)]
        hess = [arrays[f"{key}/k{k}/h"] for k in range(K)]
        ns = [int(v) for v in arrays[f"{key}/n_samples"]]
        res = NR(algo=_Algo(), damping_factor=c["damping_factor"]).compute_averaged_states(
            shared_states=_states(grads, hess, ns), _skip=True)
        assert engine_for(None).last_timing["solve"] == "device", key
        ref = [arrays[f"{key}/out{i}"] for i in range(c["outputs"])]
        got = res.parameters_update
        assert len(got) == len(ref)
        for gi, ri in zip(got, ref):
            assert np.asarray(gi).dtype == ri.dtype and np.asarray(gi).shape == ri.shape, key
        H, G = engine_sums(_states(grads, hess, ns))
        Hr, Gr = newton_raphson_sums(grads, hess, ns)
        for a, r in ((H, Hr), (G, Gr)):  # the sums, through the refactored device-resident body
            assert a.dtype == r.dtype and np.array_equal(_bits(a), _bits(r)), key
        n = Hr.shape[0]
        gf = np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in got])
        rf = np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in ref])
        rel = np.abs(gf - rf).max() / np.abs(rf).max()
        gate = 4.0 * np.linalg.cond(Hr.astype(np.float64), np.inf) * n * U
        print(f"{key}: n={n} rel {rel:.3e} gate {gate:.3e}")
        assert rel <= gate, (key, rel, gate)


@gpu
def test_environment_override_and_host_fall_through(dev, monkeypatch):
    from substrafl_amd.engine import engine_for
    from substrafl_amd.integration import accelerate, newton_raphson_update

    rng = np.random.default_rng(5)
    P, K = 19, 3
    hess = [_matrix("spd_dominant", P, k)[0] for k in range(K)]
    grads = [[rng.standard_normal(P).astype(np.float32)] for _ in range(K)]
    st = _states(grads, hess, [3, 1, 4])
    host = newton_raphson_update(st, 0.5, solve="host")
    assert engine_for(None).last_timing["solve"] == "host"
    devu = newton_raphson_update(st, 0.5)
    assert engine_for(None).last_timing["solve"] == "device"
    assert devu.dtype == host.dtype and devu.shape == host.shape
    Hr, _ = newton_raphson_sums(grads, hess, [3, 1, 4])
    assert np.abs(devu - host).max() <= 4 * np.linalg.cond(Hr, np.inf) * P * U * np.abs(host).max()
    monkeypatch.setenv("FEDAGG_NR_SOLVE", "device")
    NR = accelerate(ss.NewtonRaphson)  # the default option, overridden by the environment
    res = NR(algo=_Algo(), damping_factor=0.5).compute_averaged_states(shared_states=st, _skip=True)
    assert engine_for(None).last_timing["solve"] == "device"
    assert np.array_equal(_bits(np.asarray(res.parameters_update[0]).reshape(-1)), _bits(devu))
    monkeypatch.setenv("FEDAGG_NR_SOLVE", "host")
    assert np.array_equal(_bits(newton_raphson_update(st, 0.5, solve="device")), _bits(host))
    monkeypatch.delenv("FEDAGG_NR_SOLVE")
    # an fp32 Hessian: NumPy solves it in single precision, so the host does, and says why
    st32 = _states(grads, [h.astype(np.float32) for h in hess], [3, 1, 4])
    u32 = newton_raphson_update(st32, 0.5, solve="device")
    reason = engine_for(None).last_timing["solve"]
    assert reason.startswith("host") and "float32" in reason
    H32, G32 = newton_raphson_sums(grads, [h.astype(np.float32) for h in hess], [3, 1, 4])
    ref32 = -0.5 * np.linalg.solve(H32, G32)
    assert u32.dtype == ref32.dtype and np.array_equal(_bits(u32), _bits(ref32))


# ------------------------------------------------------------------ 4. singular
@gpu
def test_zero_column_reports_its_pivot(dev):
    T = _blocking()
    for n, j in [(1, 0), (3, 1)] + [(t + 1, t) for t in sorted(set(T))] + [(max(T) + 1, 5)]:
        A, g = _matrix("normal", n, seed=9)
        A[:, j] = 0.0
        out = dev.run(A, g)
        assert out["info"] == j + 1, (n, j, out["info"])
        assert out["intact"]


@gpu
def test_singular_system_raises_linalgerror_on_both_routes(dev):
    from substrafl_amd.integration import accelerate

    P = 6
    hess = [_matrix("normal", P, k)[0] for k in range(2)]
    for h in hess:
        h[:, 2] = 0.0
    grads = [[np.ones(P, np.float32)] for _ in range(2)]
    for mode in ("device", "host"):
        NR = accelerate(ss.NewtonRaphson, solve=mode)
        with pytest.raises(np.linalg.LinAlgError, match="Singular matrix"):
            NR(algo=_Algo(), damping_factor=1.0).compute_averaged_states(shared_states=_states(grads, hess, [1, 2]),
                                                                          _skip=True)


# ------------------------------------------------------------------ 5. bounds
@gpu
def test_padding_and_guard_bands_untouched(dev):
    T = _blocking()
    for n in (T[0] + 1, 2 * max(T) + 2):
        A, g = _matrix("normal", n, seed=3)
        tight = dev.run(A, g)
        padded = dev.run(A, g, lda=n + 3)
        assert tight["intact"] and padded["intact"], n
        for k in ("LU", "ipiv", "x"):
            assert np.array_equal(_bits(padded[k]), _bits(tight[k])), (n, k)
        assert padded["info"] == tight["info"] == 0


# ------------------------------------------------------------------ 6. determinism and stream order
@gpu
def test_deterministic_and_ordered_by_the_stream(dev):
    n = 5 * max(_blocking()) + 7
    A, g = _matrix("normal", n, seed=4)
    first = dev.run(A, g)
    again = dev.run(A, g)
    side = dev.run(A, g, stream=dev.torch.cuda.Stream(), fill_on_stream=True)
    for other in (again, side):
        for k in ("LU", "ipiv", "x"):
            assert np.array_equal(_bits(other[k]), _bits(first[k])), k
        assert other["info"] == 0 and other["intact"]


# ------------------------------------------------------------------ 6b. the strategy route, exact
@gpu
@pytest.mark.parametrize("gdtype", [np.float64, np.float32], ids=["f64_gradients", "f32_gradients"])
def test_strategy_route_exact_above_the_search_stride(dev, gdtype):
    """``newton_raphson_update`` and the accelerated strategy on a system of the exact family, at
    the smaller stride size: two clients of equal weight with H_0 = A + D, H_1 = A - D (D multiples
    of 1/4 in [-2, 2]) and g_0 = g_1 = b, so both sums are exact and the update is -x, exactly.
    fp32 gradients (b fits fp32 exactly) go through the ``fedagg_cast`` widening ahead of the solve."""
    from substrafl_amd.engine import engine_for
    from substrafl_amd.integration import accelerate, newton_raphson_update

    P = _large_sizes()[0]
    c = _exact_case(P)
    A, b, x = c["A"], c["b"], c["x"]
    Dm = np.random.default_rng([P, 1]).integers(-8, 9, (P, P)).astype(np.float64) / 4.0
    hess = [A + Dm, A - Dm]
    assert np.array_equal(b.astype(gdtype).astype(np.float64), b)
    shapes = [(P - 77,), (7, 11)]
    split = lambda v: [v[:P - 77].reshape(shapes[0]).copy(), v[P - 77:].reshape(shapes[1]).copy()]  # noqa: E731
    grads = [split(b.astype(gdtype)) for _ in range(2)]
    Hs, Gs = newton_raphson_sums(grads, hess, [1, 1])
    assert np.array_equal(Hs, A) and Gs.dtype == gdtype and np.array_equal(Gs.astype(np.float64), b)
    st = _states(grads, hess, [1, 1])
    update = newton_raphson_update(st, 1.0, solve="device")
    tm = engine_for(None).last_timing
    assert tm["solve"] == "device" and tm["P"] == P
    assert update.dtype == np.float64 and np.array_equal(update, -x), np.flatnonzero(update != -x)[:4]
    NR = accelerate(ss.NewtonRaphson, solve="device")
    res = NR(algo=_Algo(), damping_factor=1.0).compute_averaged_states(shared_states=st, _skip=True)
    assert engine_for(None).last_timing["solve"] == "device"
    got = res.parameters_update
    assert len(got) == 2
    for gi, ri, shp in zip(got, split(-x), shapes):
        assert np.asarray(gi).shape == shp and np.array_equal(np.asarray(gi), ri)


# ------------------------------------------------------------------ 6c. non-finite inputs
NON_FINITE = [np.nan, np.inf, -np.inf]
_finite_runs = {}


@gpu
@pytest.mark.parametrize("value", NON_FINITE, ids=["nan", "+inf", "-inf"])
def test_non_finite_last_diagonal_entry_feeds_nothing_else(dev, value):
    """"Inputs with NaN or Inf raise nothing and fault nothing."  The last row of A is the last
    row of L U here, so no interchange moves it before the last step and a[n-1][n-1] feeds no
    entry but itself: the interchanges and every other entry of the factors are, bit for bit,
    those of the same matrix with a finite value there (and the constructed ones)."""
    T = _strides()["panel"]
    for n in (T + 1, 2 * T + 1):
        A, b, L, Uc, perm, _ = _exact_system(n, 0, last_row_stays=True)
        assert perm[n - 1] == n - 1
        if n not in _finite_runs:  # shared by the three values, and left unchanged
            A[n - 1, n - 1] = 9.0
            _finite_runs[n] = dev.run(A, b)
        fin = _finite_runs[n]
        A[n - 1, n - 1] = value
        out = dev.run(A, b)  # check() has raised on any return code but 0; run() synchronised the stream
        assert fin["intact"] and out["intact"] and fin["info"] == 0, (n, value)
        assert np.array_equal(out["ipiv"], fin["ipiv"]) and np.array_equal(fin["ipiv"], _expected_ipiv(perm)), (n, value)
        mask = np.ones((n, n), bool)
        mask[n - 1, n - 1] = False
        assert np.array_equal(_bits(out["LU"])[mask], _bits(fin["LU"])[mask]), (n, value)
        assert np.array_equal(fin["LU"][mask], (np.tril(L, -1) + Uc)[mask]), (n, value)


@gpu
@pytest.mark.parametrize("value", NON_FINITE + ["nan_column"], ids=["nan", "+inf", "-inf", "nan_column"])
def test_non_finite_first_entry_or_column_runs_clean(dev, value):
    """The value at a[0][0], or a whole column of NaN: the calls return 0, the stream
    synchronises, every interchange stays inside [j, n) and nothing outside the outputs is
    written.  The values are unspecified and not looked at."""
    T = _strides()["panel"]
    for n in (T + 1, 2 * T + 1):
        A, g = _matrix("normal", n, seed=11)
        if isinstance(value, str):
            A[:, T // 2] = np.nan
        else:
            A[0, 0] = value
        out = dev.run(A, g)
        assert out["intact"], (n, value)
        ipiv = out["ipiv"].astype(np.int64)
        assert np.all((np.arange(n) <= ipiv) & (ipiv < n)), (n, value, ipiv)


# ------------------------------------------------------------------ 7. the default is unchanged
@gpu
def test_default_is_the_host_solve_and_never_loads_the_dense_library():
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import numpy as np\n"
            "import standin_substrafl.strategies as ss\n"
            "from standin_substrafl.strategies import schemas as sch\n"
            "from substrafl_amd.integration import accelerate\n"
            "from substrafl_amd.engine import engine_for\n"
            "class A: pass\n"
            "H = np.array([[4.0, 1.0], [1.0, 3.0]]); g = [np.array([1.0, 2.0], np.float32)]\n"
            "st = [sch.NewtonRaphsonSharedState(gradients=g, hessian=H, n_samples=2) for _ in range(2)]\n"
            "r = accelerate(ss.NewtonRaphson)(algo=A(), damping_factor=1.0).compute_averaged_states(shared_states=st, _skip=True)\n"
            "ref = -1.0 * np.linalg.solve(H * 0.5 + H * 0.5, (g[0] * 0.5 + g[0] * 0.5))\n"
            "assert np.array_equal(np.asarray(r.parameters_update[0]).reshape(-1), ref)\n"
            "assert engine_for(None).last_timing['solve'] == 'host'\n"
            "assert 'substrafl_amd._native_dense' not in sys.modules\n"
            "assert 'libfedagg_dense' not in open('/proc/self/maps').read()\n" % (str(ROOT), str(ROOT / "tests")))
    subprocess.run([sys.executable or shutil.which("python3"), "-c", code], check=True, timeout=120)
