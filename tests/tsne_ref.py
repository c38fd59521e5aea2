"""Float64 restatement of the latent-space projections (csrc/hvae_tsne.hip, src/ml/visualize.py): dense, O(n^2),
numpy only. The oracle of tests/test_gpu_tsne.py, and itself checked against scikit-learn's recorded outputs
(tests/golden/tsne.npz) by tests/test_visualize_cpu.py.

The algorithm is scikit-learn 1.7's TSNE(method="barnes_hut", init="pca", learning_rate="auto") with the exact
repulsion (angle = 0) and float64 throughout. `reverse=True` takes every sum in the opposite order: the difference
between the two runs is the restatement's own rounding noise, which the trajectory test's bar is a multiple of.
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
EPS = float(np.finfo(np.float64).eps)
FLT_MIN = float(np.finfo(np.float32).tiny)
U = 2.0 ** -53
BAR_FACTOR = 16
EXPLORATION_ITER, N_ITER_CHECK, EARLY_EXAGGERATION = 250, 50, 12.0
PERPLEXITY_TOL, PERPLEXITY_STEPS = 1e-5, 100
# name -> (n, L, perplexity); "dup" holds three exactly duplicated rows; the inputs are in the fixture (<name>_X)
CASES = {"c300": (300, 16, 30.0), "c120": (120, 5, 10.0), "dup": (193, 33, 30.0)}


def fixture():
    return np.load(GOLDEN / "tsne.npz")


def fixture_meta():
    return json.loads((GOLDEN / "tsne_meta.json").read_text())


def clustered(n: int, L: int, seed: int, n_clusters: int = 5, dup: int = 0) -> np.ndarray:
    """n float32 rows around n_clusters centres; with dup, rows 7, 70 and n - 1 copy rows 3, 3 and 11 exactly."""
    rng = np.random.RandomState(seed)
    centres = rng.normal(size=(n_clusters, L)) * 2.0
    x = (centres[rng.randint(n_clusters, size=n)] + rng.normal(size=(n, L)) * 0.7).astype(np.float32)
    if dup:
        x[7], x[70], x[n - 1] = x[3], x[3], x[11]
    return x


def neighbour_count(n: int, perplexity: float) -> int:
    return min(n - 1, int(3.0 * perplexity + 1))


def _sum(a, axis=None, reverse=False):
    a = np.asarray(a)
    if reverse:  # a copy: numpy walks a negative stride in memory order
        a = np.ascontiguousarray(a.ravel()[::-1] if axis is None else np.flip(a, axis=axis))
    return a.sum(axis=axis)


# ------------------------------------------------------------------------------------------------ neighbours ----
def sq_distances(X32: np.ndarray) -> np.ndarray:
    """[n, n] sum_l (double(x_il) - double(x_jl))^2, the difference form; the diagonal is +inf."""
    X = X32.astype(np.float64)
    n = len(X)
    D = np.empty((n, n))
    for a in range(0, n, 64):
        D[a:a + 64] = ((X[a:a + 64, None, :] - X[None, :, :]) ** 2).sum(-1)
    D[np.arange(n), np.arange(n)] = np.inf
    return D


def neighbours(X32: np.ndarray, k: int, D: np.ndarray | None = None):
    """The k nearest other rows, ascending by (distance, index): idx int32 [n, k], d2 float64 [n, k]."""
    D = sq_distances(X32) if D is None else D
    idx = np.argsort(D, axis=1, kind="stable")[:, :k]  # stable: equal distances stay in index order
    return idx.astype(np.int32), np.take_along_axis(D, idx, axis=1)


# ------------------------------------------------------------------------------------------------ perplexity ----
def perplexity_row(d: np.ndarray, perplexity: float, reverse=False, trace: list | None = None,
                   betas: list | None = None) -> np.ndarray:
    """scikit-learn's _binary_search_perplexity for one row of squared distances; trace collects every step's
    |H - log perplexity|, betas the row's final beta."""
    target = np.log(perplexity)
    beta, lo, hi = 1.0, -np.inf, np.inf
    for _ in range(PERPLEXITY_STEPS):
        p = np.exp(-d * beta)
        s = _sum(p, reverse=reverse)
        if s == 0.0:
            s = 1e-8
        p = p / s
        diff = np.log(s) + beta * _sum(d * p, reverse=reverse) - target
        if trace is not None:
            trace.append(abs(diff))
        if abs(diff) <= PERPLEXITY_TOL:
            break
        if diff > 0.0:
            lo = beta
            beta = beta * 2.0 if hi == np.inf else (beta + hi) / 2.0
        else:
            hi = beta
            beta = beta / 2.0 if lo == -np.inf else (beta + lo) / 2.0
    if betas is not None:
        betas.append(beta)
    return p


def conditional_p(d2: np.ndarray, perplexity: float, reverse=False, trace: list | None = None,
                  betas: list | None = None) -> np.ndarray:
    return np.stack([perplexity_row(d, perplexity, reverse, trace, betas) for d in d2])


def row_perplexity(p: np.ndarray) -> np.ndarray:
    """2^H of each row of a conditional P (rows sum to 1)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        h = -np.where(p > 0, p * np.log2(p), 0.0).sum(axis=1)
    return 2.0 ** h


def joint_p(idx: np.ndarray, cond: np.ndarray, reverse=False) -> np.ndarray:
    """Dense symmetric P = (C + C^T) / max(sum, eps)."""
    n = len(idx)
    C = np.zeros((n, n))
    C[np.arange(n)[:, None], idx] = cond
    P = C + C.T
    return P / max(_sum(P, reverse=reverse), EPS)


# ---------------------------------------------------------------------------------------------------- forces ----
def forces(Y: np.ndarray, P: np.ndarray, reverse=False):
    """attr [n, 2], rep [n, 2], z [n] and q [n, n] (zero diagonal) of one evaluation."""
    diff = Y[:, None, :] - Y[None, :, :]
    q = 1.0 / (1.0 + (diff ** 2).sum(-1))
    np.fill_diagonal(q, 0.0)
    z = _sum(q, axis=1, reverse=reverse)
    rep = _sum((q * q)[:, :, None] * diff, axis=1, reverse=reverse)
    attr = _sum((P * q)[:, :, None] * diff, axis=1, reverse=reverse)
    return attr, rep, z, q


def kl_error(P: np.ndarray, q: np.ndarray, Z: float, exaggeration: float, reverse=False) -> float:
    p = exaggeration * P
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = np.where(p > 0, p * np.log(np.maximum(p, FLT_MIN) / np.maximum(q / Z, FLT_MIN)), 0.0)
    return float(_sum(_sum(terms, axis=1, reverse=reverse), reverse=reverse))


def step(Y, gains, upd, P, exaggeration, momentum, lr, reverse=False, want_stats=True):
    """One force evaluation and scikit-learn's _gradient_descent step -> a dict of everything the device exposes;
    Y, gains and upd are replaced, not written in place."""
    attr, rep, z, q = forces(Y, P, reverse)
    Z = max(float(_sum(z, reverse=reverse)), EPS)
    grad = 4.0 * (exaggeration * attr - rep / Z)
    inc = upd * grad < 0.0
    gains = np.maximum(np.where(inc, gains + 0.2, gains * 0.8), 0.01)
    g = grad * gains
    upd = momentum * upd - lr * g
    out = {"attr": attr, "rep": rep, "z": z, "Z": Z, "grad": grad, "gains": gains, "upd": upd, "Y": Y + upd}
    if want_stats:
        out["error"] = kl_error(P, q, Z, exaggeration, reverse)
        out["grad_norm"] = float(np.sqrt(_sum(g * g, reverse=reverse)))
    return out


def descend(state: dict, P, it, max_iter, momentum, exaggeration, n_iter_without_progress, lr, reverse=False,
            min_grad_norm=1e-7):
    """scikit-learn's _gradient_descent over state = {Y, gains, upd}: the error and the gradient norm are looked at
    every N_ITER_CHECK-th iteration and on the last one. -> (error, last iteration)."""
    error = best_error = np.finfo(float).max
    best_iter = i = it
    for i in range(it, max_iter):
        check = (i + 1) % N_ITER_CHECK == 0
        want = check or i == max_iter - 1
        s = step(state["Y"], state["gains"], state["upd"], P, exaggeration, momentum, lr, reverse, want)
        state.update(Y=s["Y"], gains=s["gains"], upd=s["upd"])
        if want:
            error = s["error"]
        if check:
            if error < best_error:
                best_error, best_iter = error, i
            elif i - best_iter > n_iter_without_progress:
                break
            if s["grad_norm"] <= min_grad_norm:
                break
    return error, i


def learning_rate(n: int) -> float:
    return max(n / EARLY_EXAGGERATION / 4.0, 50.0)


def new_state(init: np.ndarray) -> dict:
    return {"Y": np.array(init, np.float64), "gains": np.ones_like(init, dtype=np.float64),
            "upd": np.zeros_like(init, dtype=np.float64)}


def embed(P: np.ndarray, init: np.ndarray, max_iter: int = 1000, reverse=False):
    """The two-stage loop -> (Y, kl_divergence, n_iter)."""
    lr, state = learning_rate(len(P)), new_state(init)
    kl, it = descend(state, P, 0, EXPLORATION_ITER, 0.5, EARLY_EXAGGERATION, EXPLORATION_ITER, lr, reverse)
    if it < EXPLORATION_ITER or max_iter - EXPLORATION_ITER > 0:
        kl, it = descend(state, P, it + 1, max_iter, 0.8, 1.0, 300, lr, reverse)
    return state["Y"], kl, it


# ------------------------------------------------------------------------------------------------------- PCA ----
def pca2(X32: np.ndarray, reverse=False):
    """The two leading principal components, exactly (covariance with divisor n - 1, eigh), with the sign rule of
    svd_flip(u_based_decision=False): each component's largest-magnitude entry is positive.
    -> (projection [n, 2], explained_variance_ratio [2], components [2, L])."""
    X = X32.astype(np.float64)
    n = len(X)
    Xc = X - _sum(X, axis=0, reverse=reverse) / n
    cov = _sum(Xc[:, :, None] * Xc[:, None, :], axis=0, reverse=reverse) / (n - 1)
    w, v = np.linalg.eigh(cov)
    comps = v[:, ::-1][:, :2].T.copy()
    big = np.abs(comps).argmax(axis=1)
    comps *= np.sign(comps[np.arange(2), big])[:, None]
    return Xc @ comps.T, w[::-1][:2] / w.sum(), comps


def tsne_init(proj: np.ndarray) -> np.ndarray:
    """scikit-learn's init="pca": float32 storage, then PC1 scaled to a standard deviation of 1e-4."""
    y = proj.astype(np.float32).astype(np.float64)
    return y / np.std(y[:, 0]) * 1e-4


def fit(X32: np.ndarray, perplexity: float, max_iter: int = 1000, reverse=False) -> dict:
    k = neighbour_count(len(X32), perplexity)
    idx, d2 = neighbours(X32, k)
    cond = conditional_p(d2, perplexity, reverse)
    P = joint_p(idx, cond, reverse)
    proj, evr, _ = pca2(X32, reverse)
    init = tsne_init(proj)
    Y, kl, it = embed(P, init, max_iter, reverse)
    return {"idx": idx, "d2": d2, "cond": cond, "P": P, "pca": proj, "explained_variance_ratio": evr, "init": init,
            "tsne": Y, "kl_divergence": kl, "n_iter": it}
