"""The dense fp64 Householder LQ of libfedagg_dense.so (include/fedagg_dense.h, ``fedagg_dense_gelqf_f64``
and ``fedagg_dense_orglq_f64``; substrafl_amd/csrc/dense_lq.hip): ``A = L Q`` of a row-major n x m
matrix, n <= m, and the explicit ``Q == np.linalg.qr(A.T)[0].T`` behind the opt-in device
orthonormalisation of FedPCA's averaged state.

u = 2^-53.  Sizes come from ``lq_blocking()``, B = max(panel, tile_m, tile_n):
n in {1, 2, 3, 17, panel - 1, panel, panel + 1, 2 panel + 1, B + 1, 2 B + 33} and
m in {n, n + 1, B - 1, B + 1, k_chunk - 1, k_chunk + 1, 3 k_chunk + 7}, each where m >= n; every
shape runs with tight and with padded ``lda`` / ``ldq``.

Inputs:
  * an exact family, ``_exact_case``: signed, scaled partial permutations (row i is d_i e_p(i), d_i in
    +-{1/2, 1, 2, 4}, distinct p(i)): every norm, beta, tau in {0, 1} and product is exact, so L, tau
    and Q are compared with ``np.array_equal`` against ``np.linalg.qr(A.T)``'s factors transposed;
  * bound families (standard normal; the same rounded to fp32; a "subspace-iteration" state
    G (X^T X) with X's columns scaled over three decades) against ``np.linalg.qr`` in fp64 on the same
    input: the relative residual eps = ||A - L Q||_F / ||A||_2 and the loss of orthogonality
    o = ||Q Q^T - I||_F must each be <= max(4 x LAPACK's value, 8 u sqrt(n)) and <= m n u sqrt(n)
    (Higham thm 19.4 / 19.13 with constant 1; the factor 4 is a margin, not a measurement);
  * closeness to LAPACK's Q where kappa_2(A) <= 10^3 (by SVD): ||Q_dev - Q_ref||_F <= 2 (sqrt(2) kappa_2
    (eps_dev + eps_ref) + o_dev + o_ref), the first-order perturbation bound of the Q factor doubled
    for the higher-order terms;
  * rank deficiency (a zero row, a duplicated row, a zero matrix): no fault, both bounds on o and eps
    hold against LAPACK's eps and o on the same input; only LAPACK's Q is not compared.

Every run fills the row padding and guard bands before and behind every buffer (A, tau, Q, the
workspace) with a NaN bit pattern and checks that they come back bit for bit, and that orglq leaves
d_A and d_tau as gelqf wrote them; between the two calls the workspace is overwritten with the same
pattern on the stream, so orglq can depend on nothing gelqf left there.

Worst ratios one run on an MI355X showed (profiles/dense_lq_accuracy.txt), per family as
(eps / LAPACK's, o / LAPACK's, eps / m n u sqrt(n), o / m n u sqrt(n), distance / its bound):
normal (2.08, 2.00, 0.60, 0.50, 0.15), normal_fp32 (2.05, 4.00, 0.23, 1.00, 0.15), subspace (2.91, 2.97, 0.69,
1.00, 0.16).  The 4.00 is 2 x 63 (four units of u against one, under the floor 8 u sqrt(n)); from n = 17
up the worst ratio to LAPACK is 2.97.  The 1.00 is the 1 x 2 shape, o = 2 u: the bound itself and LAPACK's
own value there; every other shape stays below 0.38 of m n u sqrt(n).  Rank-deficient inputs, worst
(eps / LAPACK's, o / LAPACK's): zero row (1.60, 1.81), duplicated row (1.63, 1.62); the zero matrix gives
eps = o = 0, as LAPACK does.
"""

import ctypes
import functools

import numpy as np
import pytest

gpu = pytest.mark.gpu

U = 2.0 ** -53
GUARD = 64  # elements of guard band before and behind every buffer
NAN_BITS = np.uint64(0x7FF8DEADBEEF0001)  # the quiet NaN of tests/test_dense_potrf_gpu.py: no arithmetic produces it
PAD = 5
BOUND_FAMILIES = ("normal", "normal_fp32", "subspace")
MAX_ELEMENTS = 2 * 10 ** 6
KAPPA_MAX = 1e3


def _lq_blocking():
    from substrafl_amd import _native_dense

    return _native_dense.lq_blocking()


def _shapes(blocking=None):
    panel, tm, tn, kc = blocking or _lq_blocking()
    B = max(panel, tm, tn)
    out = []
    for n in sorted({1, 2, 3, 17, panel - 1, panel, panel + 1, 2 * panel + 1, B + 1, 2 * B + 33}):
        for m in sorted({n, n + 1, B - 1, B + 1, kc - 1, kc + 1, 3 * kc + 7}):
            if m >= n:
                out.append((n, m))
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ------------------------------------------------------------------ inputs and the reference
@functools.lru_cache(maxsize=None)
def _exact_case(n, m, seed=0):
    """``(A, L, tau, Q)`` of the exact family with LAPACK's factors, built once and read-only."""
    rng = np.random.default_rng([n, m, seed, 1])
    A = np.zeros((n, m))
    A[np.arange(n), rng.permutation(m)[:n]] = rng.choice([0.5, 1.0, 2.0, 4.0], n) * rng.choice([-1.0, 1.0], n)
    _, tau = np.linalg.qr(A.T, mode="raw")
    q, r = np.linalg.qr(A.T)
    out = (A, np.ascontiguousarray(r.T), tau, np.ascontiguousarray(q.T))
    for a in out:
        a.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def _covariance(m):
    """X^T X of a 2 m x m standard-normal X whose columns are scaled over three decades."""
    X = np.random.default_rng([m, 7]).standard_normal((2 * m, m)) * np.logspace(0, -3, m)
    return X.T @ X


@functools.lru_cache(maxsize=None)
def _bound_case(family, n, m, seed=0):
    """``(A, reference)`` of a bound family; the reference (LAPACK's eps and o, its Q, kappa_2) is
    computed once per case and shared by the tests that need it."""
    rng = np.random.default_rng([n, m, seed, 2])
    A = rng.standard_normal((n, m))
    if family == "normal_fp32":
        A = A.astype(np.float32).astype(np.float64)
    elif family == "subspace":
        A = A @ _covariance(m)
    A = np.ascontiguousarray(A)
    A.flags.writeable = False
    return A, _reference(A)


def _measures(A, L, Q):
    """``(eps, o)``: ||A - L Q||_F / ||A||_2 (0 for a zero matrix that is reproduced exactly) and
    ||Q Q^T - I||_F, in fp64 on the host."""
    n = A.shape[0]
    norm2 = float(np.linalg.norm(A, 2))
    res = float(np.linalg.norm(A - L @ Q))
    return (res / norm2 if norm2 > 0 else res), float(np.linalg.norm(Q @ Q.T - np.eye(n)))


def _reference(A):
    q, r = np.linalg.qr(A.T)
    Q, L = np.ascontiguousarray(q.T), np.ascontiguousarray(r.T)
    eps, o = _measures(A, L, Q)
    sv = np.linalg.svd(A, compute_uv=False)
    kappa = float(sv[0] / sv[-1]) if sv[-1] > 0 else np.inf
    return {"Q": Q, "L": L, "eps": eps, "o": o, "kappa": kappa}


def _check_bounds(A, out, ref, where, worst=None):
    """The two bounds of the module docstring on eps and o of a device result against ``ref``
    (``_reference(A)``: LAPACK's eps and o on the same input).  Returns ``(eps, o)``."""
    n, m = A.shape
    eps, o = _measures(A, out["L"], out["Q"])
    householder = m * n * U * np.sqrt(n)
    for name, value in (("eps", eps), ("o", o)):
        print(f"{where}: {name} {value:.3e}  LAPACK {ref[name]:.3e}  m n u sqrt(n) {householder:.3e}")
        assert np.isfinite(value), (where, name, value)
        # The constant 1 has no slack at n = 1: at 1 x 2 the measured o is 2 u, the bound itself and
        # LAPACK's own value there (on other 1 x 2 inputs LAPACK exceeds it about one time in four,
        # profiles/dense_lq_accuracy.txt), so a change of the inputs' seed or of the order of the
        # panel's sum of squares can flip this assertion at that shape.
        assert value <= householder, (where, name, value, householder)
        assert value <= max(4.0 * ref[name], 8.0 * U * np.sqrt(n)), (where, name, value, ref[name])
        if worst is not None and ref[name] > 0:
            worst[name] = max(worst.get(name, 0.0), value / ref[name])
    if worst is not None:
        worst["eps_over_householder"] = max(worst.get("eps_over_householder", 0.0), eps / householder)
        worst["o_over_householder"] = max(worst.get("o_over_householder", 0.0), o / householder)
    return eps, o


def _closeness_bound(kappa, eps_dev, eps_ref, o_dev, o_ref):
    return 2.0 * (np.sqrt(2.0) * kappa * (eps_dev + eps_ref) + o_dev + o_ref)


# ------------------------------------------------------------------ the device
class Dev:
    """``fedagg_dense_gelqf_f64`` + ``fedagg_dense_orglq_f64`` on torch-owned device buffers, each
    with guard bands on both sides."""

    def __init__(self):
        import torch

        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        from substrafl_amd import _native_dense

        self.torch = torch
        self.lib = _native_dense.load()
        self.check = _native_dense.check

    @staticmethod
    def image(body):
        """[guard | body | guard] as uint64 bits."""
        guard = np.full(GUARD, NAN_BITS, np.uint64)
        return np.concatenate([guard, np.ascontiguousarray(body).reshape(-1).view(np.uint64), guard])

    def run(self, A, lda=None, ldq=None, stream=None, busy_between=False):
        """Factor and form Q on the device, nothing synchronising between the two calls.  Between
        them, on the same stream: snapshots of d_A and d_tau, the workspace overwritten with the NaN
        pattern, and with ``busy_between`` unrelated work (a matrix product) as well."""
        torch, vp = self.torch, ctypes.c_void_p
        n, m = A.shape
        lda = m if lda is None else lda
        ldq = m if ldq is None else ldq
        body = np.full((n, lda), NAN_BITS, np.uint64)
        body[:, :m] = _bits(A)
        ws_elems = int(self.lib.fedagg_dense_lq_ws_bytes(n, m)) // 8
        assert ws_elems > 0
        images = {"A": self.image(body), "tau": self.image(np.full(n, NAN_BITS, np.uint64)),
                  "Q": self.image(np.full((n, ldq), NAN_BITS, np.uint64)),
                  "ws": self.image(np.full(ws_elems, NAN_BITS, np.uint64))}
        d = {k: torch.from_numpy(v.view(np.int64)).cuda() for k, v in images.items()}
        ws_fill = d["ws"].clone()
        other = torch.ones((128, 128), dtype=torch.float64, device="cuda") if busy_between else None
        torch.cuda.synchronize()
        st = stream if stream is not None else torch.cuda.current_stream()
        p = {k: vp(v.data_ptr() + 8 * GUARD) for k, v in d.items()}
        with torch.cuda.stream(st):
            self.check(self.lib.fedagg_dense_gelqf_f64(p["A"], n, m, lda, p["tau"], p["ws"], vp(st.cuda_stream)), "gelqf")
            a_after, tau_after = d["A"].clone(), d["tau"].clone()
            d["ws"].copy_(ws_fill)
            if busy_between:
                for _ in range(4):
                    other = other @ other * (1.0 / 128.0)
            self.check(self.lib.fedagg_dense_orglq_f64(p["A"], n, m, lda, p["tau"], p["Q"], ldq, p["ws"],
                                                       vp(st.cuda_stream)), "orglq")
        st.synchronize()
        torch.cuda.synchronize()
        host = {k: v.cpu().numpy().view(np.uint64) for k, v in d.items()}
        fa = host["A"][GUARD:GUARD + n * lda].reshape(n, lda)
        fq = host["Q"][GUARD:GUARD + n * ldq].reshape(n, ldq)
        intact = (np.array_equal(host["A"], a_after.cpu().numpy().view(np.uint64))  # orglq only reads d_A
                  and np.array_equal(host["tau"], tau_after.cpu().numpy().view(np.uint64))  # ... and d_tau
                  and bool(np.all(fa[:, m:] == NAN_BITS)) and bool(np.all(fq[:, m:] == NAN_BITS)))
        for k, img in images.items():
            intact = intact and np.array_equal(host[k][:GUARD], img[:GUARD]) and np.array_equal(host[k][-GUARD:], img[-GUARD:])
        F = fa[:, :m].view(np.float64)
        return {"F": F, "L": np.tril(F[:, :n]), "tau": host["tau"][GUARD:GUARD + n].view(np.float64),
                "Q": np.ascontiguousarray(fq[:, :m]).view(np.float64), "intact": intact}

    def run_both_layouts(self, A):
        """Tight and padded leading dimensions: the same bits, returned once."""
        n, m = A.shape
        tight, padded = self.run(A), self.run(A, lda=m + PAD, ldq=m + PAD + 2)
        assert tight["intact"] and padded["intact"], (n, m)
        for k in ("F", "tau", "Q"):
            assert np.array_equal(_bits(tight[k]), _bits(padded[k])), (n, m, k)
        return tight


@pytest.fixture(scope="module")
def dev():
    return Dev()


# (tests/test_dense_lq_abi.py asserts, without a GPU, that the largest shape stays under MAX_ELEMENTS)


# ------------------------------------------------------------------ 1. the exact family
@gpu
def test_exact_family(dev):
    for n, m in _shapes():
        for seed in (0, 1):
            A, L, tau, Q = _exact_case(n, m, seed)
            out = dev.run_both_layouts(A)
            where = (n, m, seed)
            assert set(np.unique(tau)) <= {0.0, 1.0}, where
            assert np.array_equal(out["tau"], tau), (where, "tau")
            assert np.array_equal(out["L"], L), (where, "L")
            assert np.array_equal(out["Q"], Q), (where, "Q")


# ------------------------------------------------------------------ 2. the bounds and the closeness
@gpu
@pytest.mark.parametrize("family", BOUND_FAMILIES)
def test_residual_orthogonality_and_closeness(dev, family):
    worst, closeness_cases = {}, 0
    for n, m in _shapes():
        A, ref = _bound_case(family, n, m)
        out = dev.run_both_layouts(A)
        eps, o = _check_bounds(A, out, ref, (family, n, m), worst)
        if ref["kappa"] <= KAPPA_MAX:
            closeness_cases += 1
            dist = float(np.linalg.norm(out["Q"] - ref["Q"]))
            bound = _closeness_bound(ref["kappa"], eps, ref["eps"], o, ref["o"])
            print(f"{(family, n, m)}: kappa {ref['kappa']:.3g}  |Q - Qref|_F {dist:.3e}  bound {bound:.3e}")
            assert dist <= bound, (family, n, m, dist, bound, ref["kappa"])
            if bound > 0:
                worst["closeness"] = max(worst.get("closeness", 0.0), dist / bound)
    assert closeness_cases >= len(_shapes()) // 2, closeness_cases
    print(f"WORST {family}: " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


# ------------------------------------------------------------------ 3. rank deficiency, non-finite input
@gpu
@pytest.mark.parametrize("kind", ["zero_row", "duplicated_row", "zero_matrix"])
def test_rank_deficient_input_still_gives_orthonormal_rows(dev, kind):
    """Both gates on eps and o, against LAPACK's eps and o on the same rank-deficient input; only its
    Q is not compared (the null-space rows of a rank-deficient Q are not determined by A)."""
    worst = {}
    for n, m in [(1, 1), (3, 4), (33, 33), (33, 65), (65, 511), (161, 513)]:
        A = _bound_case("normal", n, m)[0].copy()
        if kind == "zero_row":
            A[n // 2] = 0.0
        elif kind == "duplicated_row":
            A[n - 1] = A[0]
        else:
            A[:] = 0.0
        out = dev.run_both_layouts(A)
        _check_bounds(A, out, _reference(A), (kind, n, m), worst)
    print(f"WORST {kind}: " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


@gpu
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf], ids=["nan", "+inf", "-inf"])
def test_non_finite_input_faults_nothing(dev, value):
    for n, m in [(1, 2), (33, 65), (65, 513)]:
        for at in [(0, 0), (n - 1, m - 1), (n // 2, m // 2)]:
            A = _bound_case("normal", n, m)[0].copy()
            A[at] = value
            out = dev.run(A, lda=m + PAD, ldq=m + PAD)  # check() has raised on any return code but 0
            assert out["intact"], (n, m, at, value)


# ------------------------------------------------------------------ 4. determinism and stream order
@gpu
def test_deterministic_and_ordered_by_the_stream(dev):
    n, m = _shapes()[-1]
    A = _bound_case("subspace", n, m)[0]
    first = dev.run(A)
    side = dev.run(A, stream=dev.torch.cuda.Stream())
    other_side = dev.run(A, stream=dev.torch.cuda.Stream(), lda=m + PAD, ldq=m + PAD)
    busy = dev.run(A, busy_between=True)
    busy_side = dev.run(A, stream=dev.torch.cuda.Stream(), busy_between=True)
    for other in (side, other_side, busy, busy_side):
        assert first["intact"] and other["intact"]
        for k in ("F", "tau", "Q"):
            assert np.array_equal(_bits(other[k]), _bits(first[k])), k
    E, L, tau, Q = _exact_case(n, m)
    out = dev.run(E, stream=dev.torch.cuda.Stream(), busy_between=True)
    assert out["intact"] and np.array_equal(out["L"], L) and np.array_equal(out["Q"], Q) and np.array_equal(out["tau"], tau)
