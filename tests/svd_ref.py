"""Shared helpers of the SVD tests (tests/test_svd_cpu.py, tests/test_gpu_svd.py): the float64 CPU restatement of the
device algorithm of src/ml/svd.py (numpy and scipy only) and the fixture of tests/golden/make_svd_fixture.py.

The algorithm is scikit-learn's randomized TruncatedSVD (n_components = k, n_oversamples = 10, n_iter = 5,
random_state = 42) with two exchanges that leave the spanned subspace, and so the scores, unchanged in exact
arithmetic: CholeskyQR2 for the LU and QR normalisers, and an eigendecomposition of the W x W Gram matrix of B^T
for LAPACK's SVD of B (W = k + 10)."""
from __future__ import annotations

import functools
import json
from pathlib import Path

import numpy as np
from scipy.sparse import csr_matrix

import lightgcn_ref as LR

GOLDEN = Path(__file__).resolve().parent / "golden"
SEED, OVERSAMPLES, N_ITER, LD = 42, 10, 5, 64
BAR_FACTOR = 16                       # golden bar = BAR_FACTOR * noise, the LightGCN fixture's factor
CASES = (("150x97", 50), ("150x97", 8), ("97x150", 50), ("97x150", 8))   # (matrix, n_components)
RANKS_CASE = ("150x97", 50)           # the case whose 99-negative ranks are stored
PIVOT_FLOOR = LD * 2.0 ** -53         # a pivot at or below PIVOT_FLOOR * G[k, k] is rounding noise: not positive


def case_key(name: str, k: int) -> str:
    return f"{name}_k{k}"


@functools.lru_cache(maxsize=None)
def case_matrix(name: str) -> csr_matrix:
    """The fixture's matrices: the LightGCN fixture graph (150 x 97, M = A) and its transpose (97 x 150, M = A^T)."""
    m = LR.fixture_graph_unchecked()
    return m if name == "150x97" else csr_matrix(m.T)


def matrix_digest(matrix: csr_matrix) -> str:
    from gen import digest
    m = matrix.tocsr().copy()
    m.sum_duplicates()
    m.sort_indices()
    return digest(np.array(m.shape, np.int64), m.indptr.astype(np.int64), m.indices.astype(np.int32),
                  m.data.astype(np.float64))


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(GOLDEN / "svd.npz", allow_pickle=False))


@functools.lru_cache(maxsize=None)
def fixture_meta():
    return json.loads((GOLDEN / "svd_meta.json").read_text())


def sketch(n: int, W: int) -> np.ndarray:
    """The reference's starting matrix Omega [n, W], draw for draw, from a RandomState of its own."""
    return np.random.RandomState(SEED).normal(size=(n, W))


def chol_inv(G: np.ndarray, W: int):
    """(R^-1 upper triangular [W, W], flag) with G[:W, :W] = R^T R; flag = 1 where a pivot is not positive (at or
    below PIVOT_FLOOR times its diagonal entry) or NaN, as hvae_svd_chol_inv sets it."""
    a = np.array(G[:W, :W], np.float64)
    diag = a.diagonal().copy()
    flag = 0
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(W):
            piv = a[k, k]
            if not piv > PIVOT_FLOOR * diag[k]:
                flag = 1
            d = np.sqrt(piv)
            a[k, k] = d
            a[k + 1:, k] /= d
            a[k + 1:, k + 1:] -= np.outer(a[k + 1:, k], a[k + 1:, k])
        L = np.tril(a)
        Linv = np.zeros_like(L)
        for j in range(W):
            Linv[j, j] = 1.0 / L[j, j]
            for i in range(j + 1, W):
                Linv[i, j] = -(L[i, j:i] @ Linv[j:i, j]) / L[i, i]
    return Linv.T.copy(), flag


def cholqr2(Y: np.ndarray):
    """(Q, flag): Y's columns orthonormalised by two passes of Gram -> Cholesky -> Y R^-1."""
    W = Y.shape[1]
    flag = 0
    for _ in range(2):
        Rinv, f = chol_inv(Y.T @ Y, W)
        flag |= f
        Y = Y @ Rinv
    return Y, flag


def components_from(Bt: np.ndarray, Q: np.ndarray, transposed: bool, k: int):
    """(components [k, n_items], singular values [k], T) from B^T = M^T Q [n, W]: the eigenpairs of its Gram matrix,
    descending; T is the [W, k] matrix src/ml/svd.py hands to svd_apply."""
    w, E = np.linalg.eigh(Bt.T @ Bt)
    order = np.argsort(w)[::-1]
    w, E = w[order], E[:, order]
    with np.errstate(invalid="ignore"):
        s = np.sqrt(w)
    T = (E if transposed else E / s)[:, :k]
    comps = ((Q if transposed else Bt) @ T).T
    return flip_signs(comps), s[:k], T


def flip_signs(comps: np.ndarray) -> np.ndarray:
    """svd_flip(u_based_decision=False): each component's largest-magnitude entry (the first of equals) positive."""
    big = np.abs(comps).argmax(axis=1)
    return comps * np.sign(comps[np.arange(len(comps)), big])[:, None]


def explained_variance_ratio(matrix: csr_matrix, user_factors: np.ndarray) -> np.ndarray:
    """TruncatedSVD's: var(X V, axis=0) over the summed per-column variance of X."""
    a = matrix.tocsr().astype(np.float64)
    n = a.shape[0]
    mean = np.asarray(a.sum(axis=0)).ravel() / n
    full_var = (np.asarray(a.multiply(a).sum(axis=0)).ravel() / n - mean ** 2).sum()
    return np.var(user_factors, axis=0) / full_var


def fit(matrix: csr_matrix, k: int) -> dict:
    """The device algorithm of SVDRecommender.fit in float64 on the host."""
    a = matrix.tocsr().astype(np.float64)
    a.sum_duplicates()
    n_users, n_items = a.shape
    W = k + OVERSAMPLES
    transposed = n_users < n_items
    M = csr_matrix(a.T) if transposed else a
    Mt = csr_matrix(M.T)
    Q, flag = sketch(M.shape[1], W), 0
    for _ in range(N_ITER):
        Q, f1 = cholqr2(M @ Q)
        Q, f2 = cholqr2(Mt @ Q)
        flag |= f1 | f2
    Q, f = cholqr2(M @ Q)
    flag |= f
    Bt = Mt @ Q
    if flag or not np.isfinite(Bt).all():  # SVDRecommender.fit raises here
        return {"flag": 1, "transposed": transposed}
    comps, s, _ = components_from(Bt, Q, transposed, k)
    uf = a @ comps.T
    return {"components": comps, "user_factors": uf, "singular_values": s,
            "explained_variance_ratio": explained_variance_ratio(a, uf), "scores": uf @ comps, "flag": flag,
            "transposed": transposed}


def score_bar32(user_factors: np.ndarray, components: np.ndarray, bar64: float) -> float:
    """The bar of the fp32 device scores against the reference's float64 ones: the factors rounded to fp32 once
    each (2 u per product), the product rounded (u), and a 64-term fp32 sum in any order, (64 + 5) u sum_j |u_j v_j|
    with u = 2^-24 covering all of it to first order, plus the float64 factors' own bar; the largest over the
    matrix."""
    return float((64 + 5) * 2.0 ** -24 * (np.abs(user_factors) @ np.abs(components)).max() + bar64)


def candidates(matrix: csr_matrix, u: int, t: int) -> np.ndarray:
    """Every item the user has not seen, the test item left out: the 99-negative protocol's candidates where fewer
    than 99 exist."""
    return np.setdiff1d(np.arange(matrix.shape[1]), np.append(matrix[u].indices, t))


def ref_bracket(scores: np.ndarray, cand: np.ndarray, t: int, tol: float):
    """[#{ref > s_t + tol}, #{ref >= s_t - tol}]: the ranks the test item can take when every score moves by at
    most tol / 2."""
    return int((scores[cand] > scores[t] + tol).sum()), int((scores[cand] >= scores[t] - tol).sum())


def sketch_is_full_rank(matrix: csr_matrix, k: int) -> bool:
    return fit(matrix, k)["flag"] == 0


def rank_deficient_rows(seed: int = 4) -> np.ndarray:
    """40 distinct rows of 60 columns stacked three times: a [120, 60] matrix of rank 40 (fp32-exact values, so it
    is also an interaction matrix whose sketch at k = 50, W = 60 has rank 40)."""
    rows = np.random.Generator(np.random.PCG64(seed)).standard_normal((40, 60)).astype(np.float32).astype(np.float64)
    return np.concatenate([rows, rows, rows])
