"""Shared helpers of the LightGCN tests (tests/test_lightgcn_cpu.py, tests/test_gpu_lightgcn.py): the fixture of
tests/golden/make_lightgcn_fixture.py, its graph rebuilt from a seed and checked against the fixture's digest, the
kernel-test graphs, and the float64 restatements the kernels are compared with."""
from __future__ import annotations

import functools
import json
from pathlib import Path

import numpy as np
from scipy.sparse import csr_matrix

GOLDEN = Path(__file__).resolve().parent / "golden"
SEED_TORCH, SEED_NUMPY = 5, 11       # torch.manual_seed / np.random.seed before every reference fit
N_USERS, N_ITEMS, DIM, LAYERS = 150, 97, 64, 3
EMPTY_USER, EMPTY_ITEM, HOT_ITEM = 17, 40, 5
N_NEG = 99                           # more than 97 items hold: every row's candidates are all its unseen items
BAR_FACTOR = 16                      # golden bar = BAR_FACTOR * max|fp32 - fp64| of the reference's own two runs


def random_graph(n_users: int, n_items: int, p: float, seed: int, empty_user: int, empty_item: int,
                 hot_item: int | None = None, hot_users: int = 0, hot_user: int | None = None, hot_items: int = 0,
                 twos: int = 7) -> csr_matrix:
    """A seeded Bernoulli(p) interaction matrix with one empty row, one empty column, optionally an item with
    exactly hot_users users and a user with exactly hot_items items, and `twos` entries of 2.0 (a duplicate pair
    summed)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    dense = rng.random((n_users, n_items)) < p
    dense[empty_user, :] = False
    dense[:, empty_item] = False
    if hot_user is not None:
        dense[hot_user, :] = False
        pool = np.setdiff1d(np.arange(n_items), [empty_item] + ([] if hot_item is None else [hot_item]))
        dense[hot_user, rng.choice(pool, hot_items, replace=False)] = True
    if hot_item is not None:
        dense[:, hot_item] = False
        pool = np.setdiff1d(np.arange(n_users), [empty_user] + ([] if hot_user is None else [hot_user]))
        dense[rng.choice(pool, hot_users, replace=False), hot_item] = True
    rows, cols = np.nonzero(dense)
    data = np.ones(len(rows))
    data[rng.choice(len(rows), min(twos, len(rows)), replace=False)] = 2.0
    return csr_matrix((data, (rows, cols)), shape=(n_users, n_items))


@functools.lru_cache(maxsize=None)
def fixture_graph_unchecked() -> csr_matrix:
    return random_graph(N_USERS, N_ITEMS, 0.085, 2025, EMPTY_USER, EMPTY_ITEM, HOT_ITEM, 124)


def fixture_tests(matrix: csr_matrix):
    """(users, test items) of the fixture's evaluation: every user, one seeded item outside the user's row."""
    rng = np.random.Generator(np.random.PCG64(77))
    users = np.arange(matrix.shape[0], dtype=np.int64)
    tests = np.empty(len(users), np.int64)
    for u in users:
        seen = matrix.indices[matrix.indptr[u]:matrix.indptr[u + 1]]
        tests[u] = rng.choice(np.setdiff1d(np.arange(matrix.shape[1]), seen))
    return users, tests


def graph_digest(matrix: csr_matrix, users, tests) -> str:
    from gen import digest
    m = matrix.tocsr().copy()
    m.sum_duplicates()
    m.sort_indices()
    return digest(m.indptr.astype(np.int64), m.indices.astype(np.int32), m.data.astype(np.float64),
                  np.asarray(users, np.int64), np.asarray(tests, np.int64))


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(GOLDEN / "lightgcn.npz", allow_pickle=False))


@functools.lru_cache(maxsize=None)
def fixture_meta():
    return json.loads((GOLDEN / "lightgcn_meta.json").read_text())


@functools.lru_cache(maxsize=None)
def fixture_graph():
    """(matrix, test users, test items) of the fixture, checked against its digest."""
    m = fixture_graph_unchecked()
    users, tests = fixture_tests(m)
    assert graph_digest(m, users, tests) == fixture_meta()["data_digest"], "the rebuilt graph differs from the fixture's"
    return m, users, tests


def state_digest(state=None) -> str:
    """A digest of numpy's global MT19937 state (key and position)."""
    from gen import digest
    st = np.random.get_state() if state is None else state
    return digest(np.asarray(st[1], np.uint32), np.array([st[2]], np.int64))


KERNEL_GRAPHS = {  # name -> random_graph arguments (tests/test_gpu_lightgcn.py)
    "37x23": dict(n_users=37, n_items=23, p=0.2, seed=1, empty_user=3, empty_item=7),
    "300x257": dict(n_users=300, n_items=257, p=0.03, seed=2, empty_user=11, empty_item=100, hot_item=9,
                    hot_users=290),
    "2100x130": dict(n_users=2100, n_items=130, p=0.02, seed=3, empty_user=5, empty_item=64, hot_item=2,
                     hot_users=1500, hot_user=8, hot_items=120),
}


@functools.lru_cache(maxsize=None)
def kernel_graph(name: str) -> csr_matrix:
    return random_graph(**KERNEL_GRAPHS[name])


def structure(matrix: csr_matrix) -> csr_matrix:
    """The 0/1 structure of a matrix (matrix.nonzero()), float64."""
    m = matrix.tocsr().copy()
    m.sum_duplicates()
    m.eliminate_zeros()
    m.data[:] = 1.0
    return m.astype(np.float64)


def adjacency(matrix: csr_matrix):
    """(A_w float64 CSR [n, n] holding the fp32-rounded edge weights, deg^-1/2 float64 [n], degrees) of the
    bipartite graph, users first; the weight of (u, i) is fp32(s_u * s_i) as the kernels and the reference form it."""
    s = structure(matrix)
    n_users, n_items = s.shape
    deg = np.concatenate([np.asarray(s.sum(axis=1)).ravel(), np.asarray(s.sum(axis=0)).ravel()])
    with np.errstate(divide="ignore"):
        scale = np.where(deg > 0, np.power(np.where(deg > 0, deg, 1.0), -0.5), 0.0)
    r, c = s.nonzero()
    w = (scale[r] * scale[n_users + c]).astype(np.float32).astype(np.float64)
    n = n_users + n_items
    a = csr_matrix((np.concatenate([w, w]), (np.concatenate([r, c + n_users]), np.concatenate([c + n_users, r]))),
                   shape=(n, n))
    return a, scale, deg


def propagate_oracle(a: csr_matrix, x: np.ndarray, add: np.ndarray | None, alpha: float):
    """(alpha * (add + A x), the absolute sum alpha * (|add| + |A| |x|)) in float64 from fp32 inputs."""
    x = x.astype(np.float64)
    ad = np.zeros_like(x) if add is None else add.astype(np.float64)
    return alpha * (ad + a @ x), alpha * (np.abs(ad) + abs(a) @ np.abs(x))


def bpr_oracle(F: np.ndarray, n_users: int, users, pos, neg, reg: float):
    """(loss, g [n, d]) of the reference's BPR loss (baseline.py:354-367) in float64 from the fp32 table F."""
    F = F.astype(np.float64)
    users, pos, neg = (np.asarray(a, np.int64) for a in (users, pos, neg))
    nb = len(users)
    fu, fp, fn = F[users], F[n_users + pos], F[n_users + neg]
    x = (fu * fp).sum(1) - (fu * fn).sum(1)
    loss = np.mean(np.maximum(-x, 0) + np.log1p(np.exp(-np.abs(x)))) + reg * ((fu ** 2).sum() + (fp ** 2).sum()
                                                                              + (fn ** 2).sum()) / nb
    c = (-1.0 / (1.0 + np.exp(x)) / nb)[:, None]
    g = np.zeros_like(F)
    np.add.at(g, users, c * (fp - fn) + 2 * reg / nb * fu)
    np.add.at(g, n_users + pos, c * fu + 2 * reg / nb * fp)
    np.add.at(g, n_users + neg, -c * fu + 2 * reg / nb * fn)
    return float(loss), g
