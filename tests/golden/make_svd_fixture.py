"""G10: SVD fixture from the reference's own src/ml/baseline.py (SVDRecommender, :102-118).

Run in the build container (where the reference checkout and scikit-learn exist; a few seconds):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_svd_fixture.py

The matrices are tests/svd_ref.py's: the LightGCN fixture graph, 150 users x 97 items (scikit-learn iterates over
M = A), and its transpose, 97 x 150 (M = A^T), each at n_components = 50 and 8. The reference is observed, outputs
only, per case <matrix>_k<k>:
  _components         model.components_ = item_factors [k, n_items]
  _user_factors       fit_transform's result [n_users, k]
  _singular_values    model.singular_values_ [k]
  _evr_sum            model.explained_variance_ratio_.sum(), the figure the reference logs
  _scores             predict() of every user [n_users, n_items]
and for 150x97_k50 the reference's rank of each test item under the 99-negative protocol (`ranks`; 97 items hold
fewer than 99 negatives, so every row's candidates are all its unseen items and nothing is drawn).
meta: the scikit-learn version, the data digests, and per stored array
  noise = the larger of two float64 differences from the reference: its own run with the QR normaliser
          (randomized_svd(..., power_iteration_normalizer="QR") inside TruncatedSVD.fit_transform's own steps),
          and tests/svd_ref.py's restatement of the device algorithm (CholeskyQR2, Gram eigendecomposition);
  bar   = 16 * noise, the golden bar of the GPU tests.
The generator asserts that another rank-k SVD is no such neighbour -- the exact SVD's scores miss the fixture's by
more than 1e6 bars -- and that the rank brackets the GPU test checks are sharp: the share of rows whose bracket
[lo, hi] at the test's tolerance has hi - lo <= 1 is recorded (`tight_bracket_share`) and at least 0.9.
"""
from __future__ import annotations

import importlib
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE), str(HERE.parent)]
from make_golden import import_reference  # noqa: E402
import lightgcn_ref as LR  # noqa: E402
import svd_ref as SR  # noqa: E402

ARRAYS = ("components", "user_factors", "singular_values", "evr_sum", "scores")


def observe(rec, matrix) -> dict:
    """A fitted reference recommender's outputs."""
    return {"components": np.array(rec.item_factors), "user_factors": np.array(rec.user_factors),
            "singular_values": np.array(rec.model.singular_values_),
            "evr_sum": np.array(rec.model.explained_variance_ratio_.sum()),
            "scores": np.stack([rec.predict(u) for u in range(matrix.shape[0])])}


def qr_run(matrix, k: int) -> dict:
    """TruncatedSVD.fit_transform's steps around randomized_svd with the QR normaliser (the estimator's own
    parameter check refuses "QR", so the function is called as the estimator calls it)."""
    from sklearn.utils.extmath import randomized_svd, svd_flip
    from sklearn.utils.sparsefuncs import mean_variance_axis
    u, s, vt = randomized_svd(matrix, k, n_iter=SR.N_ITER, n_oversamples=SR.OVERSAMPLES,
                              power_iteration_normalizer="QR", random_state=SR.SEED, flip_sign=False)
    u, vt = svd_flip(u, vt, u_based_decision=False)
    uf = matrix @ vt.T
    evr = np.var(uf, axis=0) / mean_variance_axis(matrix.tocsr().astype(np.float64), axis=0)[1].sum()
    return {"components": vt, "user_factors": uf, "singular_values": s, "evr_sum": np.array(evr.sum()),
            "scores": uf @ vt}


def main():
    import pandas as pd
    import scipy.linalg
    import sklearn
    import_reference()
    b = importlib.import_module("src.ml.baseline")
    out, meta = {}, {"sklearn": sklearn.__version__, "numpy": np.__version__, "random_state": SR.SEED,
                     "bar_factor": SR.BAR_FACTOR, "data_digest": {}, "noise": {}, "bar": {}, "exact_svd_miss": {}}
    fitted = {}
    for name, k in SR.CASES:
        matrix, key = SR.case_matrix(name), SR.case_key(name, k)
        meta["data_digest"][name] = SR.matrix_digest(matrix)
        state = LR.state_digest()
        rec = b.SVDRecommender(n_components=k)
        assert rec.model.random_state == SR.SEED and rec.model.algorithm == "randomized"
        assert (rec.model.n_iter, rec.model.n_oversamples) == (SR.N_ITER, SR.OVERSAMPLES)
        rec.fit(matrix)
        assert LR.state_digest() == state, "the reference's fit drew from numpy's global stream"
        fitted[key] = rec
        ref = observe(rec, matrix)
        qr = qr_run(matrix, k)
        mine = SR.fit(matrix, k)
        assert mine["flag"] == 0 and mine["transposed"] == (name == "97x150")
        mine["evr_sum"] = mine["explained_variance_ratio"].sum()
        for a in ARRAYS:
            assert ref[a].dtype == np.float64
            out[f"{key}_{a}"] = ref[a]
            noise = max(float(np.abs(ref[a] - qr[a]).max()), float(np.abs(ref[a] - mine[a]).max()))
            assert 0 < noise < 1e-11, (key, a, noise)
            meta["noise"][f"{key}_{a}"] = noise
            meta["bar"][f"{key}_{a}"] = SR.BAR_FACTOR * noise
        # some other rank-k SVD is not the reference's run
        u, s, vt = scipy.linalg.svd(matrix.toarray())
        exact = matrix.toarray() @ vt[:k].T @ vt[:k]
        miss = float(np.abs(exact - ref["scores"]).max())
        meta["exact_svd_miss"][key] = miss
        assert miss > 1e6 * meta["bar"][f"{key}_scores"], (key, miss)

    # the reference's ranks under the 99-negative protocol
    name, k = SR.RANKS_CASE
    matrix, key = SR.case_matrix(name), SR.case_key(name, k)
    users, tests = LR.fixture_tests(matrix)
    uid = [f"U{u}" for u in range(matrix.shape[0])]
    iid = [f"I{i}" for i in range(matrix.shape[1])]
    test_df = pd.DataFrame({"user_id": [uid[u] for u in users], "asin": [iid[i] for i in tests]})
    u2i, i2i = {u: n for n, u in enumerate(uid)}, {i: n for n, i in enumerate(iid)}
    ranks, ndcg, K_ALL = [], b.ndcg_at_k, matrix.shape[1]

    def ndcg_rec(top_k, relevant, kk):
        if kk == K_ALL:
            ranks.append(int(np.flatnonzero(np.asarray(top_k) == relevant[0])[0]))
        return ndcg(top_k, relevant, kk)

    b.ndcg_at_k = ndcg_rec
    try:
        state = LR.state_digest()
        metrics = b.evaluate_model(fitted[key], "SVD", matrix, test_df, u2i, i2i, [5, 10, 20, K_ALL], LR.N_NEG)
        assert LR.state_digest() == state, "evaluate_model drew from numpy"
    finally:
        b.ndcg_at_k = ndcg
    assert len(ranks) == len(users)
    out["ranks"] = np.array(ranks, np.int32)
    meta["metrics"] = {str(kk): v for kk, v in metrics.items() if kk != K_ALL}
    scores = out[f"{key}_scores"]
    tol = 2 * SR.score_bar32(out[f"{key}_user_factors"], out[f"{key}_components"], meta["bar"][f"{key}_scores"])
    tight = 0
    for u, t, rank in zip(users, tests, ranks):
        lo, hi = SR.ref_bracket(scores[u], SR.candidates(matrix, u, t), t, tol)
        assert lo <= rank <= hi
        tight += hi - lo <= 1
    meta["rank_tol"] = tol
    meta["tight_bracket_share"] = tight / len(users)
    assert meta["tight_bracket_share"] >= 0.9

    np.savez_compressed(HERE / "svd.npz", **out)
    (HERE / "svd_meta.json").write_text(json.dumps(meta, indent=1))
    print(json.dumps({k: meta[k] for k in ("noise", "exact_svd_miss", "tight_bracket_share", "rank_tol")}, indent=1))
    size = (HERE / "svd.npz").stat().st_size
    print("svd.npz", size, "bytes")
    assert size < 1_000_000


if __name__ == "__main__":
    main()
