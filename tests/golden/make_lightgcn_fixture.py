"""G9: LightGCN fixture from the reference's own src/ml/baseline.py (LightGCNRecommender, :239-385).

Run in the build container (where the reference checkout exists; a few seconds):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_lightgcn_fixture.py

The graph is tests/lightgcn_ref.py's: 150 users x 97 items, more than 1024 and fewer than 2048 interactions (an
epoch is two batches, the second ragged), one empty user row, one empty item column (still drawn as a negative),
one item with at least 120 users, a few entries of 2.0. With torch.manual_seed and np.random.seed fixed before
every fit, the reference is observed, outputs only:
  init                     the initial [247, 64] table (user rows, then item rows)
  batch_users / _pos / _neg  the first epoch's triples in step order (batch k = [1024 k, 1024 (k + 1)))
  user_e1, item_e1, user_e5, item_e5   the final embeddings after epochs = 1 and epochs = 5
  scores, ranks            after epochs = 5: predict() of every user (evaluate_model's scores, fp32) and the
                           reference's rank of each test item under the 99-negative protocol (97 items hold fewer
                           than 99 negatives, so every row's candidates are all its unseen items and nothing is drawn)
  meta: the data digest, a digest of numpy's state after each fit, the losses, and per stored array
        noise = max|fp32 - fp64| against the same reference code run in float64 from the same draws (the fp32
        initial table cast up, float64 edge weights) and bar = 16 * noise, the golden bar of the GPU tests.
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


def fit(b, matrix, epochs: int, double: bool, record: dict | None = None):
    """One seeded fit of the reference's LightGCNRecommender; in float64 when `double` (the model built in fp32
    from the same draws, then cast; the adjacency with unrounded float64 weights)."""
    import torch
    rec = b.LightGCNRecommender(embedding_dim=LR.DIM, n_layers=LR.LAYERS, epochs=epochs)
    rec.device = torch.device("cpu")
    model_cls, perm, randint = b.LightGCNModel, np.random.permutation, np.random.randint
    if double:
        b.LightGCNModel = lambda *a, **k: model_cls(*a, **k).double()
        a64, _, _ = adjacency64(matrix)
        rec._build_adj_matrix = lambda m: a64
    draws = {"perm": [], "neg": []}
    np.random.permutation = lambda n: draws["perm"].append(perm(n)) or draws["perm"][-1]
    np.random.randint = lambda lo, hi, size: draws["neg"].append(randint(lo, hi, size)) or draws["neg"][-1]
    try:
        torch.manual_seed(LR.SEED_TORCH)
        np.random.seed(LR.SEED_NUMPY)
        rec.fit(matrix)
    finally:
        b.LightGCNModel, np.random.permutation, np.random.randint = model_cls, perm, randint
    if record is not None:
        record.update(draws)
    return rec


def adjacency64(matrix):
    """The normalised adjacency as a float64 torch sparse tensor with unrounded weights s_u * s_i."""
    import torch
    s = LR.structure(matrix).tocoo()
    n_users, n_items = s.shape
    a, scale, _ = LR.adjacency(matrix)
    r = np.concatenate([s.row, s.col + n_users])
    c = np.concatenate([s.col + n_users, s.row])
    vals = torch.tensor(scale[r] * scale[c], dtype=torch.float64)
    return torch.sparse_coo_tensor(torch.tensor(np.stack([r, c])), vals, a.shape), scale, None


def main():
    import pandas as pd
    import torch
    import_reference()
    b = importlib.import_module("src.ml.baseline")
    matrix = LR.fixture_graph_unchecked()
    users, tests = LR.fixture_tests(matrix)
    nnz = LR.structure(matrix).nnz
    assert 1024 < nnz < 2048 and matrix.shape == (LR.N_USERS, LR.N_ITEMS)
    assert matrix[LR.EMPTY_USER].nnz == 0 and matrix[:, LR.EMPTY_ITEM].nnz == 0
    assert matrix[:, LR.HOT_ITEM].nnz >= 120 and (matrix.data == 2.0).any()
    out, meta = {}, {"seed_torch": LR.SEED_TORCH, "seed_numpy": LR.SEED_NUMPY, "numpy": np.__version__,
                     "torch": torch.__version__, "shape": list(matrix.shape), "nnz": int(nnz),
                     "embedding_dim": LR.DIM, "n_layers": LR.LAYERS, "bar_factor": LR.BAR_FACTOR,
                     "data_digest": LR.graph_digest(matrix, users, tests), "state_digest": {}, "noise": {}, "bar": {}}

    torch.manual_seed(LR.SEED_TORCH)
    m0 = b.LightGCNModel(LR.N_USERS, LR.N_ITEMS, LR.DIM, LR.LAYERS)
    out["init"] = torch.cat([m0.user_embedding.weight, m0.item_embedding.weight]).detach().numpy().copy()

    pos_users, pos_items = matrix.nonzero()
    runs = {}
    for epochs in (1, 5):
        draws = {}
        r32 = fit(b, matrix, epochs, False, draws)
        meta["state_digest"][str(epochs)] = LR.state_digest()
        r64 = fit(b, matrix, epochs, True)
        assert LR.state_digest() == meta["state_digest"][str(epochs)]
        runs[epochs] = (r32, r64)
        if epochs == 1:
            perm = draws["perm"][0]
            out["batch_users"] = pos_users[perm].astype(np.int32)
            out["batch_pos"] = pos_items[perm].astype(np.int32)
            out["batch_neg"] = np.concatenate(draws["neg"]).astype(np.int32)
            assert [len(d) for d in draws["neg"]] == [1024, nnz - 1024]
            assert (out["batch_neg"] == LR.EMPTY_ITEM).any(), "the empty column is never drawn as a negative"
        for key, a32, a64 in ((f"user_e{epochs}", r32.user_final_emb, r64.user_final_emb),
                              (f"item_e{epochs}", r32.item_final_emb, r64.item_final_emb)):
            assert a32.dtype == torch.float32 and a64.dtype == torch.float64
            out[key] = a32.numpy().copy()
            meta["noise"][key] = float((a32.double() - a64).abs().max())

    r32, r64 = runs[5]
    uid = [f"U{u}" for u in range(LR.N_USERS)]
    iid = [f"I{i}" for i in range(LR.N_ITEMS)]
    test_df = pd.DataFrame({"user_id": [uid[u] for u in users], "asin": [iid[i] for i in tests]})
    u2i, i2i = {u: k for k, u in enumerate(uid)}, {i: k for k, i in enumerate(iid)}
    ranks, ndcg, K_ALL = [], b.ndcg_at_k, LR.N_ITEMS

    def ndcg_rec(top_k, relevant, k):
        if k == K_ALL:
            ranks.append(int(np.flatnonzero(np.asarray(top_k) == relevant[0])[0]))
        return ndcg(top_k, relevant, k)

    b.ndcg_at_k = ndcg_rec
    try:
        state = np.random.get_state()
        metrics = b.evaluate_model(r32, "LightGCN", matrix, test_df, u2i, i2i, [5, 10, 20, K_ALL], LR.N_NEG)
        assert LR.state_digest() == LR.state_digest(state), "evaluate_model drew from numpy"
    finally:
        b.ndcg_at_k = ndcg
    out["scores"] = np.stack([r32.predict(int(u)) for u in users]).astype(np.float32)
    s64 = np.stack([r64.predict(int(u)) for u in users])
    meta["noise"]["scores"] = float(np.abs(out["scores"].astype(np.float64) - s64).max())
    out["ranks"] = np.array(ranks, np.int32)
    assert len(ranks) == len(users)
    meta["metrics"] = {str(k): v for k, v in metrics.items() if k != K_ALL}
    meta["bar"] = {k: LR.BAR_FACTOR * v for k, v in meta["noise"].items()}

    np.savez_compressed(HERE / "lightgcn.npz", **out)
    (HERE / "lightgcn_meta.json").write_text(json.dumps(meta, indent=1))
    print(json.dumps({k: meta[k] for k in ("nnz", "data_digest", "state_digest", "noise", "bar")}, indent=1))
    print("lightgcn.npz", (HERE / "lightgcn.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
