"""Shared helpers of the baseline tests (tests/test_baselines_cpu.py, tests/test_gpu_baselines.py): the fixture of
tests/golden/make_baseline_fixture.py, its planted datasets rebuilt from tests/golden/gen.py, the scipy float64
restatement of Item-KNN, and the rank brackets."""
from __future__ import annotations

import functools
import json
from pathlib import Path

import numpy as np
from scipy.sparse import csr_matrix, diags

GOLDEN = Path(__file__).resolve().parent / "golden"
CONFIGS = {  # tests/golden/make_baseline_fixture.py CONFIGS
    "small": dict(n_users=400, n_items=300, n_clusters=8, lam=6),
    "large": dict(n_users=600, n_items=10050, n_clusters=32, lam=6),
}
SEED, N_NEG = 7, 99
BAR = 2.0 ** -23  # one fp32 rounding of a double sum of non-negative terms, with a factor 2 of headroom


def bar(ref):
    """|got - ref| <= 2^-23 max(|ref|, 1); the 1 covers the diagonal subtraction."""
    return BAR * np.maximum(np.abs(ref), 1.0)


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(GOLDEN / "baselines.npz", allow_pickle=False))


@functools.lru_cache(maxsize=None)
def fixture_meta():
    return json.loads((GOLDEN / "baselines_meta.json").read_text())


@functools.lru_cache(maxsize=None)
def planted(cfg_name: str):
    """(train+val matrix, test users, test items, the three frames, ids) of a fixture config, checked against the
    fixture's data digest."""
    from gen import PLANTED_CONFIG, digest, synth_planted
    import pandas as pd
    tr, va, te, _, uid, iid = synth_planted(**dict(PLANTED_CONFIG, **CONFIGS[cfg_name]))
    both = pd.concat([tr, va])
    rows = both["user_id"].str[1:].astype(np.int64).values
    cols = both["asin"].str[1:].astype(np.int64).values
    matrix = csr_matrix((np.ones(len(both)), (rows, cols)), shape=(len(uid), len(iid)))
    users = te["user_id"].str[1:].astype(np.int64).values
    tests = te["asin"].str[1:].astype(np.int64).values
    m = matrix.copy()
    m.sum_duplicates()
    m.sort_indices()
    got = digest(m.indptr.astype(np.int64), m.indices.astype(np.int32), m.data.astype(np.float64), users, tests)
    assert got == fixture_meta()["configs"][cfg_name]["data_digest"], "planted data differ from the fixture's"
    fx = fixture()
    assert np.array_equal(fx[f"{cfg_name}_users"], users) and np.array_equal(fx[f"{cfg_name}_tests"], tests)
    return matrix, users, tests


def knn_oracle(matrix: csr_matrix, rows: np.ndarray, zero_diag: bool) -> np.ndarray:
    """float64 [len(rows), N]: sum over the nonzero structure I_u of cosine(c_j, c_i), the i = j term removed when
    zero_diag. Sparse products: (B_ind Nn^T) Nn with Nn = M diag(1 / ||c||)."""
    m = csr_matrix(matrix, dtype=np.float64)
    m.sum_duplicates()
    m.eliminate_zeros()
    sq = np.asarray(m.multiply(m).sum(axis=0)).ravel()
    inv = np.where(sq > 0, 1.0 / np.sqrt(np.where(sq > 0, sq, 1.0)), 0.0)
    nn = (m @ diags(inv)).tocsr()
    ind = m[np.asarray(rows)].copy()
    ind.data[:] = 1.0
    s = np.asarray(((ind @ nn.T) @ nn).todense())
    if zero_diag:
        s = s - np.asarray(ind.todense())  # j in I_u implies a non-empty column: its own term is exactly 1
    return s


def candidates(tests, neg):
    return np.concatenate([np.asarray(tests)[:, None], neg], axis=1).astype(np.int64)


def exact_bracket(cs: np.ndarray):
    """(#greater, #equal) of candidate 0 per row of candidate scores cs [R, C]."""
    return (cs[:, 1:] > cs[:, :1]).sum(1), (cs[:, 1:] == cs[:, :1]).sum(1)


def tol_bracket(cs: np.ndarray):
    """[#{ref > s_t + tol}, #{ref >= s_t - tol}] per row, tol the score bar at the test item's score."""
    tol = bar(cs[:, :1])
    return (cs[:, 1:] > cs[:, :1] + tol).sum(1), (cs[:, 1:] >= cs[:, :1] - tol).sum(1)


def replay_choice_stream(matrix: csr_matrix, users, tests, passes: int):
    """numpy's global state after `passes` runs of the reference's per-row np.random.choice loop from SEED."""
    m = matrix.tocsr()
    n_items = m.shape[1]
    np.random.seed(SEED)
    for _ in range(passes):
        for u, t in zip(users, tests):
            mask = np.ones(n_items, dtype=bool)
            mask[m.indices[m.indptr[u]:m.indptr[u + 1]]] = False
            mask[t] = False
            np.random.choice(np.flatnonzero(mask), N_NEG, replace=False)
    return np.random.get_state()


def same_state(a, b) -> bool:
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
