"""G8: Popularity / Item-KNN fixture from the reference's own src/ml/baseline.py.

Run in the build container (where the reference checkout exists; a few seconds):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_baseline_fixture.py

Two planted datasets (gen.synth_planted, written in the reference's on-disk layout): "small", 400 users x 300
items (the reference's dense-similarity path, diagonal zeroed) and "large", 600 users x 10,050 items (its
on-the-fly path above 10,000 items, diagonal kept). For each, the reference's PopularityRecommender and
ItemKNNRecommender are fitted on its train+val matrix and its evaluate_model runs the 99-negative protocol with
np.random.seed(7) set right before. The run is observed, not restated: every predict() result, every
np.random.choice draw and every ranked list evaluate_model hands to its metric functions is recorded. Stored
(tests/golden/baselines.npz + baselines_meta.json), inputs -> outputs only:
  <cfg>_users / _tests          the test rows, in evaluation order
  <cfg>_neg                     the 99 negatives per row (both models draw the same ones: same seed, same rows)
  <cfg>_pop                     Popularity's float64 scores (one row: the same for every user)
  small_knn                     Item-KNN's float64 predict rows, whole
  large_knn / large_items       Item-KNN's scores at each row's 100 candidates followed by 200 fixed items
  <cfg>_<model>_rank            the reference's rank of the test item per row
  meta: the data digest and the reference's aggregated metrics (for information: its ranks inside score ties
        depend on numpy's unstable argsort, so the metrics are not a target)
The generator asserts that every reference rank lies in [#greater, #greater + #equal] of its own scores.
"""
from __future__ import annotations

import importlib
import json
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
from gen import digest, write_planted_artifacts  # noqa: E402
from make_golden import import_reference  # noqa: E402

CONFIGS = {
    "small": dict(n_users=400, n_items=300, n_clusters=8, lam=6),
    "large": dict(n_users=600, n_items=10050, n_clusters=32, lam=6),
}
SEED = 7
N_NEG = 99
K_ALL = 100          # a k that keeps the whole ranked candidate list
N_FIXED = 200        # extra fixed items scored per row of the large config
MODELS = (("pop", "PopularityRecommender"), ("knn", "ItemKNNRecommender"))


def matrix_digest(matrix, users, tests) -> str:
    m = matrix.tocsr()
    m.sum_duplicates()
    m.sort_indices()
    return digest(m.indptr.astype(np.int64), m.indices.astype(np.int32), m.data.astype(np.float64),
                  np.asarray(users, np.int64), np.asarray(tests, np.int64))


def observe(b, model, name, matrix, test_df, u2i, i2i):
    """One evaluate_model run of the reference with its predict / choice / ranked lists recorded."""
    scores, draws, ranks = [], [], []
    predict = model.predict
    choice = np.random.choice
    ndcg = b.ndcg_at_k

    def predict_rec(u):
        s = predict(u)
        scores.append(np.array(s, dtype=np.float64, copy=True))
        return s

    def choice_rec(*a, **k):
        d = choice(*a, **k)
        draws.append(np.array(d, dtype=np.int32))
        return d

    def ndcg_rec(top_k, relevant, k):
        if k == K_ALL:
            ranks.append(int(np.flatnonzero(np.asarray(top_k) == relevant[0])[0]))
        return ndcg(top_k, relevant, k)

    model.predict = predict_rec
    np.random.choice = choice_rec
    b.ndcg_at_k = ndcg_rec
    try:
        np.random.seed(SEED)
        metrics = b.evaluate_model(model, name, matrix, test_df, u2i, i2i, [5, 10, 20, K_ALL], N_NEG)
    finally:
        model.predict = predict
        np.random.choice = choice
        b.ndcg_at_k = ndcg
    del metrics[K_ALL]
    return np.stack(scores), np.stack(draws), np.array(ranks, np.int32), metrics


def main():
    import pandas as pd
    import_reference()
    b = importlib.import_module("src.ml.baseline")
    out, meta = {}, {"seed": SEED, "n_negatives": N_NEG, "numpy": np.__version__, "configs": {}}
    for cfg_name, cfg in CONFIGS.items():
        with tempfile.TemporaryDirectory() as td:
            data, _ = write_planted_artifacts(td, cfg)
            full, train_df, val_df, maps = b.load_training_data(str(data))
            u2i, i2i = maps["user_to_idx"], maps["item_to_idx"]
            matrix, _ = b._build_input_matrix(train_df, val_df, u2i, i2i, full.shape)
            test_df = pd.read_csv(Path(data) / "test.csv")
        users = np.array([u2i[u] for u in test_df["user_id"]], np.int32)
        tests = np.array([i2i[i] for i in test_df["asin"]], np.int32)
        n_items = matrix.shape[1]
        fixed = np.random.Generator(np.random.PCG64(5)).choice(n_items, N_FIXED, replace=False)
        fixed = np.sort(fixed).astype(np.int32)
        out[f"{cfg_name}_users"], out[f"{cfg_name}_tests"] = users, tests
        m = {"config": cfg, "shape": list(matrix.shape), "zero_diag": bool(n_items <= 10000),
             "data_digest": matrix_digest(matrix, users, tests), "metrics": {}, "tie_rows": {}, "pessimistic_rows": {}}
        for key, cls in MODELS:
            model = getattr(b, cls)()
            model.fit(matrix)
            scores, neg, rank, metrics = observe(b, model, key, matrix, test_df, u2i, i2i)
            assert scores.shape == (len(users), n_items) and neg.shape == (len(users), N_NEG)
            if f"{cfg_name}_neg" in out:
                assert np.array_equal(out[f"{cfg_name}_neg"], neg), "the two models drew different negatives"
            out[f"{cfg_name}_neg"] = neg
            cand = np.concatenate([tests[:, None], neg], axis=1)
            cs = np.take_along_axis(scores, cand.astype(np.int64), axis=1)
            gt = (cs[:, 1:] > cs[:, :1]).sum(1)
            eq = (cs[:, 1:] == cs[:, :1]).sum(1)
            assert ((rank >= gt) & (rank <= gt + eq)).all(), f"{cfg_name}/{key}: a reference rank outside its bracket"
            m["tie_rows"][key] = float((eq > 0).mean())
            m["pessimistic_rows"][key] = float(((eq > 0) & (rank == gt + eq)).sum() / max((eq > 0).sum(), 1))
            m["metrics"][key] = {str(k): v for k, v in metrics.items()}
            out[f"{cfg_name}_{key}_rank"] = rank
            if key == "pop":
                assert (scores == scores[0]).all()
                out[f"{cfg_name}_pop"] = scores[0]
            elif cfg_name == "small":
                out["small_knn"] = scores
            else:
                out["large_items"] = fixed
                out["large_knn"] = np.concatenate([cs, scores[:, fixed.astype(np.int64)]], axis=1)
        meta["configs"][cfg_name] = m
        print(cfg_name, json.dumps({k: m[k] for k in ("shape", "data_digest", "tie_rows", "pessimistic_rows")}))
    np.savez_compressed(HERE / "baselines.npz", **out)
    (HERE / "baselines_meta.json").write_text(json.dumps(meta, indent=1))
    size = (HERE / "baselines.npz").stat().st_size
    print("baselines.npz", size, "bytes")
    assert size < 1_000_000, "fixture too large"


if __name__ == "__main__":
    main()
