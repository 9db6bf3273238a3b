"""The dense fp64 Cholesky of libfedagg_dense.so (include/fedagg_dense.h, ``fedagg_dense_potrf_f64``;
substrafl_amd/csrc/dense_potrf.hip), the certificate behind the opt-in device Hessian check of
NewtonRaphson's clients.

u = 2^-53, gamma_n = n u / (1 - n u).  Sizes: those of the LU tests ({1, 2, 3, 17}, T - 1, T, T + 1
and 2 T + 1 for every blocking size T the library reports, 5 max(T) + 7) and 577 = 9 * 64 + 1: nine
tile rows below the first panel, the last tile one row high and the last block one column wide.

Three kinds of input:
  * an exact family, ``_exact_factor``: an integer L (strictly lower entries in [-2, 2], diagonal in
    {1, 2, 4}) and A = L L^T.  Every partial sum a_ik - sum l_im l_km is an integer below 2^40 in
    any order, every pivot is l_kk^2 and every quotient l_ik l_kk / l_kk, so the factor has one
    right value per entry and is compared with ``np.array_equal``;
  * the same with a_pp lowered by l_pp^2: pivot p is exactly 0, ``info == p + 1``, and the leading
    p x p triangle is still L's;
  * bound families (``spd_dominant`` of the LU tests; Gram matrices X^T D X / m + l2 I of
    fp32-valued X, the shape of a logistic regression's Hessian) held to Higham's thm 10.3,
    |A - L L^T| <= gamma_{n+1} |L| |L^T| on the lower triangle, with the LU tests' factor 3 for
    the fp64 products of the test itself.

Every run pre-fills the strict upper triangle, the padding of the rows and guard bands before and
behind the buffers with a NaN bit pattern and checks that they come back bit for bit.
"""

import ctypes
import functools
import gc

import numpy as np
import pytest

from test_dense_solve_gpu import _blocking, _gamma, _matrix, _sizes

gpu = pytest.mark.gpu

GUARD = 64  # elements of guard band before and behind every buffer
NAN_BITS = np.uint64(0x7FF8DEADBEEF0001)  # a quiet NaN no arithmetic produces
INFO_FILL = -77
LARGE = 577


def _potrf_sizes():
    out = sorted(set(_sizes()) | {LARGE})
    assert LARGE % max(_blocking()) == 1 and LARGE // max(_blocking()) >= 5
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _exact_factor(n, seed=0):
    """``(A, L)`` of the exact family, built once per size and read-only."""
    rng = np.random.default_rng([n, seed])
    L = np.tril(rng.integers(-2, 3, (n, n)).astype(np.float64), -1)
    L[np.diag_indices(n)] = rng.choice([1.0, 2.0, 4.0], n)
    A = L @ L.T  # integers below 4 n + 16: exact in any order
    assert np.abs(A).max() <= 4 * n + 16 and np.array_equal(A, A.T)
    A.flags.writeable = L.flags.writeable = False
    return A, L


def _symmetric(G):
    """G's lower triangle mirrored: exactly symmetric whatever the BLAS made of the product."""
    return np.ascontiguousarray(np.tril(G) + np.tril(G, -1).T)


def _gram(n, m, l2, seed=0):
    """X^T D X / m + l2 I: X (m x n) standard normal rounded to fp32, D = p (1 - p) of a logistic
    model's predictions; rank min(m, n) before the l2 term."""
    rng = np.random.default_rng([n, m, seed])
    X = rng.standard_normal((m, n)).astype(np.float32).astype(np.float64)
    p = 1.0 / (1.0 + np.exp(-rng.standard_normal(m)))
    return _symmetric((X.T * (p * (1.0 - p))) @ X / m + l2 * np.eye(n))


BOUND_FAMILIES = ("spd_dominant", "gram_4n", "gram_half_l2")


def _bound_matrix(family, n):
    if family == "spd_dominant":
        return _symmetric(_matrix("spd_dominant", n)[0])
    if family == "gram_4n":
        return _gram(n, 4 * n, 0.0)
    return _gram(n, max(1, n // 2), 1e-3)


class Dev:
    """``fedagg_dense_potrf_f64`` on torch-owned device buffers with guard bands on both sides."""

    def __init__(self):
        import torch

        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        from substrafl_amd import _native_dense

        self.torch = torch
        self.lib = _native_dense.load()
        self.check = _native_dense.check

    def host_image(self, A, lda, true_upper=False):
        """[guard | n rows of lda | guard] as uint64 bits: A's lower triangle, the NaN pattern
        everywhere else (``true_upper``: A's strict upper triangle in place)."""
        n = A.shape[0]
        body = np.full((n, lda), NAN_BITS, np.uint64)
        keep = np.ones((n, n), bool) if true_upper else np.tril(np.ones((n, n), bool))
        body[:, :n][keep] = _bits(A)[keep]
        guard = np.full(GUARD, NAN_BITS, np.uint64)
        return np.concatenate([guard, body.reshape(-1), guard])

    def call(self, d_buf, n, lda, d_info, stream):
        vp = ctypes.c_void_p
        self.check(self.lib.fedagg_dense_potrf_f64(vp(d_buf.data_ptr() + 8 * GUARD), n, lda,
                                                   vp(d_info.data_ptr() + 4 * GUARD), vp(stream.cuda_stream)), "potrf")

    def result(self, image, d_buf, d_info, n, lda):
        """``L`` (lower triangle, zeros above), ``info``, and ``intact``: every bit outside the
        lower triangle and the info word is what it was."""
        out = d_buf.cpu().numpy().view(np.uint64)
        oi = d_info.cpu().numpy()
        body, was = out[GUARD:GUARD + n * lda].reshape(n, lda), image[GUARD:GUARD + n * lda].reshape(n, lda)
        outside = np.ones((n, lda), bool)
        outside[:, :n] = ~np.tril(np.ones((n, n), bool))
        intact = (np.array_equal(body[outside], was[outside]) and np.array_equal(out[:GUARD], image[:GUARD])
                  and np.array_equal(out[GUARD + n * lda:], image[GUARD + n * lda:])
                  and bool(np.all(oi[:GUARD] == INFO_FILL)) and bool(np.all(oi[GUARD + 1:] == INFO_FILL)))
        return {"L": np.tril(body[:, :n].view(np.float64)), "info": int(oi[GUARD]), "intact": intact}

    def run(self, A, lda=None, stream=None, fill_on_stream=False, true_upper=False):
        """Factor on the device.  ``fill_on_stream``: A reaches its buffer by a device copy
        enqueued on ``stream`` directly before the library call (nothing synchronises between)."""
        torch = self.torch
        n = A.shape[0]
        lda = n if lda is None else lda
        image = self.host_image(A, lda, true_upper)
        src = torch.from_numpy(image.view(np.int64)).cuda()
        d_info = torch.full((2 * GUARD + 1,), INFO_FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        st = stream if stream is not None else torch.cuda.current_stream()
        if fill_on_stream:
            d_buf = torch.zeros_like(src)  # what a factorisation that ran ahead of the copy would read
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                d_buf.copy_(src, non_blocking=True)
        else:
            d_buf = src
        self.call(d_buf, n, lda, d_info, st)
        st.synchronize()
        torch.cuda.synchronize()
        return self.result(image, d_buf, d_info, n, lda)


@pytest.fixture(scope="module")
def dev():
    return Dev()


def _assert_exact(out, L, where):
    assert out["intact"], where
    assert out["info"] == 0, (where, out["info"])
    bad = np.argwhere(out["L"] != L)
    assert bad.size == 0, (where, len(bad), bad[:4].tolist())


# ------------------------------------------------------------------ 1. the exact family
@gpu
def test_exact_family(dev):
    for n in _potrf_sizes():
        A, L = _exact_factor(n)
        _assert_exact(dev.run(A), L, n)


@gpu
def test_failed_pivot_reports_itself_and_keeps_the_leading_triangle(dev):
    """a_pp lowered by l_pp^2: d = 0 at pivot p exactly.  ``info == p + 1``, rows and columns
    [0, p) of L are the factor's, and the launches after it run clean on what is there."""
    for n in _potrf_sizes():
        A, L = _exact_factor(n)
        for p in sorted({0, 31, 32, 33, n - 1}):
            if p >= n:
                continue
            B = A.copy()
            B[p, p] -= L[p, p] ** 2
            out = dev.run(B)
            assert out["intact"], (n, p)
            assert out["info"] == p + 1, (n, p, out["info"])
            assert np.array_equal(out["L"][:p, :p], L[:p, :p]), (n, p)


# ------------------------------------------------------------------ 2. the bound
@gpu
@pytest.mark.parametrize("family", BOUND_FAMILIES)
def test_factorisation_bound(dev, family):
    for n in _potrf_sizes():
        A = _bound_matrix(family, n)
        assert np.array_equal(A, A.T)
        out = dev.run(A)
        L = out["L"]
        assert out["intact"] and out["info"] == 0, (family, n, out["info"])
        assert np.all(np.diag(L) > 0), (family, n)
        low = np.tril(np.ones((n, n), bool))
        err = np.abs(A - L @ L.T)[low]
        bound = (3.0 * _gamma(n + 1) * (np.abs(L) @ np.abs(L).T))[low]
        print(f"{family} n={n}: max err / bound {float((err / bound).max()):.3f}")
        assert np.all(err <= bound), (family, n, float((err - bound).max()))


# ------------------------------------------------------------------ 3. what is never touched
@gpu
def test_upper_triangle_padding_and_guard_bands_untouched(dev):
    """The NaN pattern in the strict upper triangle, in a padded ``lda = n + 5`` band and in the
    guard bands comes back bit for bit (``intact``), and it feeds nothing: L is, bit for bit, the
    L of the run with the true upper triangle in place."""
    for n in (3, 33, 65, 129, 327, LARGE):
        A = _bound_matrix("gram_half_l2", n)
        tight, padded, full = dev.run(A), dev.run(A, lda=n + 5), dev.run(A, lda=n + 5, true_upper=True)
        for out in (tight, padded, full):
            assert out["intact"] and out["info"] == 0, n
        assert np.array_equal(_bits(padded["L"]), _bits(tight["L"])), n
        assert np.array_equal(_bits(full["L"]), _bits(tight["L"])), n
        E, L = _exact_factor(n)
        _assert_exact(dev.run(E, lda=n + 5), L, (n, "lda = n + 5"))


# ------------------------------------------------------------------ 4. non-finite input
NON_FINITE = [np.nan, np.inf, -np.inf]


@gpu
@pytest.mark.parametrize("value", NON_FINITE, ids=["nan", "+inf", "-inf"])
def test_non_finite_first_entry_fails_the_first_pivot(dev, value):
    for n in (1, 33, 65, 129):
        A = _exact_factor(n)[0].copy()
        A[0, 0] = value
        out = dev.run(A)  # check() has raised on any return code but 0; run() synchronised the stream
        assert out["intact"], (n, value)
        assert out["info"] != 0 and out["info"] == 1, (n, value, out["info"])


@gpu
@pytest.mark.parametrize("value", NON_FINITE, ids=["nan", "+inf", "-inf"])
def test_non_finite_last_entry_feeds_nothing_else(dev, value):
    """a[n-1][n-1] is read by the last pivot alone: every other entry of L is the exact family's,
    and the last pivot fails."""
    for n in (1, 33, 65, 129):
        A, L = _exact_factor(n)
        B = A.copy()
        B[n - 1, n - 1] = value
        out = dev.run(B)
        assert out["intact"], (n, value)
        assert out["info"] == n, (n, value, out["info"])
        mask = np.ones((n, n), bool)
        mask[n - 1, n - 1] = False
        assert np.array_equal(out["L"][mask], L[mask]), (n, value)


# ------------------------------------------------------------------ 5. determinism and stream order
@gpu
def test_deterministic_and_ordered_by_the_stream(dev):
    A = _bound_matrix("gram_4n", LARGE)
    first, again = dev.run(A), dev.run(A)
    side = dev.run(A, stream=dev.torch.cuda.Stream(), fill_on_stream=True)
    padded_side = dev.run(A, lda=LARGE + 5, stream=dev.torch.cuda.Stream(), fill_on_stream=True)
    for other in (again, side, padded_side):
        assert other["info"] == first["info"] == 0 and other["intact"] and first["intact"]
        assert np.array_equal(_bits(other["L"]), _bits(first["L"]))
    E, L = _exact_factor(LARGE)
    _assert_exact(dev.run(E, stream=dev.torch.cuda.Stream(), fill_on_stream=True), L, "exact, side stream")


@gpu
def test_graph_capture_runs_nothing_and_replays(dev):
    """The call captured into a graph on a side stream: nothing runs during the capture (the
    launch sequence is a function of n alone and nothing synchronises), and the replay factors
    whatever the buffer holds then, to the bits of the eager run."""
    torch = dev.torch
    n, lda = 129, 134
    data = {"A": _bound_matrix("gram_4n", n), "B": _exact_factor(n)[0]}
    eager = {k: dev.run(v, lda=lda) for k, v in data.items()}
    images = {k: dev.host_image(v, lda) for k, v in data.items()}
    srcs = {k: torch.from_numpy(v.view(np.int64)).cuda() for k, v in images.items()}
    d_buf = torch.empty_like(srcs["A"])
    d_info = torch.full((2 * GUARD + 1,), INFO_FILL, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_buf.copy_(srcs["A"], non_blocking=True)
        dev.call(d_buf, n, lda, d_info, side)  # eager first: also loads the code object
    side.synchronize()
    assert np.array_equal(_bits(dev.result(images["A"], d_buf, d_info, n, lda)["L"]), _bits(eager["A"]["L"]))

    with torch.cuda.stream(side):
        d_buf.copy_(srcs["A"], non_blocking=True)
        d_info.fill_(INFO_FILL)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        dev.call(d_buf, n, lda, d_info, side)
    torch.cuda.synchronize()
    assert torch.equal(d_buf, srcs["A"]) and bool((d_info == INFO_FILL).all()), "a kernel ran during the capture"
    gc.collect()
    for k in ("B", "A"):
        with torch.cuda.stream(side):
            d_buf.copy_(srcs[k], non_blocking=True)
            d_info.fill_(INFO_FILL)
            graph.replay()
        torch.cuda.synchronize()
        out = dev.result(images[k], d_buf, d_info, n, lda)
        assert out["intact"] and out["info"] == eager[k]["info"] == 0, k
        assert np.array_equal(_bits(out["L"]), _bits(eager[k]["L"])), k
