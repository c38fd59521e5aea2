"""G10: Mult-VAE fixture from the reference's own src/ml/baseline.py (MultVAE / MultVAERecommender, :126-231).

Run where the reference checkout exists (about a minute on the CPU):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_multvae_fixture.py

The graph is tests/multvae_ref.py's g_small(): 600 users x 97 items (an epoch is 512 + 88), an empty user row, a
single-item user, an 85-item user, a few entries of 2.0, an item nobody has. With torch.manual_seed(SEED_TORCH) before
every fit the reference is observed on the CPU, outputs only. torch.nn.functional.dropout and torch.randn_like are
wrapped for the length of the fit so that the multipliers and eps of every step are multvae_ref.draws(step): a pure
function of (SEED_DEV, step), which is also what the device's Philox streams draw, so no mask has to be stored. They
do not touch torch's global generator, exactly as on a device run of the reference, where the masks come from the
device's generator: the global stream is consumed by the initial parameters and the loader's shuffles only.

Recorded (multvae.npz): the epoch orders (orders [3, 600]), the per-step losses (losses [6], the reference's own
loss tensor through a forward hook and its formula), predict() of every user after epochs = 1 and epochs = 3
(scores_e1, scores_e3), the reference's 0-based rank of every user's test item under the 99-negative protocol
after 3 epochs (ranks; 97 items hold fewer than 99 negatives, so the candidates are all unseen items and nothing is
drawn), slices of the initial parameters (init_w1 = encoder.0.weight[:4], init_bd2 = decoder.2.bias).
multvae_meta.json: digests of the graph and of the initial parameters, and per stored array noise = max |fp32 - fp64|
against the same reference code run in float64 from the same draws (parameters cast up) and bar = 16 * noise, the
golden bar of the tests. The script asserts bar <= 1e-3 * max |scores|, so the golden test cannot be vacuous.

Quality (meta["quality"]): NDCG@10 under the 99-negative protocol of 8 seeded fits of the reference, with its own
torch dropout, on tests/golden/gen.py's planted set QUALITY_CFG (400 users: one batch per epoch), QUALITY_EPOCHS
epochs each, with the sample mean and standard deviation: the reference's own spread.
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
import multvae_ref as MR  # noqa: E402


def fit(b, matrix, epochs: int, double: bool, record: dict):
    """One seeded fit of the reference's MultVAERecommender with multvae_ref.draws() handed to it; in float64 when
    `double` (the model built in fp32 from the same draws, then cast)."""
    import torch
    import torch.nn.functional as F
    from torch.utils.data import DataLoader, TensorDataset
    N = matrix.shape[1]
    state = {"step": 0, "calls": 0, "cur": None}
    record.update(orders=[], losses=[])
    model_cls, loader_cls, dropout, randn_like = b.MultVAE, b.DataLoader, F.dropout, torch.randn_like

    class Observed(model_cls):
        def forward(self, x):
            if self.training:
                state["cur"] = MR.draws(state["step"], x.shape[0], N)
                state["calls"] = 0
            out = super().forward(x.to(self.mu_layer.weight.dtype))
            if self.training:
                recon, mu, logvar = out
                xx = x.to(recon.dtype)
                loss = -torch.mean(torch.sum(F.log_softmax(recon, dim=1) * xx, dim=1)) \
                    + 0.2 * (-0.5 * torch.mean(torch.sum(1 + logvar - mu.pow(2) - logvar.exp(), dim=1)))
                record["losses"].append(float(loss.detach()))
                assert state["calls"] == 3
                state["step"] += 1
            return out

    def make_model(*a, **k):
        m = Observed(*a, **k)
        return m.double() if double else m

    class Loader:  # the real DataLoader over (row, index): its use of the global generator does not depend on the data
        def __init__(self, ds, **kw):
            self.inner = loader_cls(TensorDataset(ds.tensors[0], torch.arange(len(ds))), **kw)

        def __iter__(self):
            order = []
            for x, idx in self.inner:
                order.append(idx.numpy())
                yield (x,)
            record["orders"].append(np.concatenate(order))

        def __len__(self):
            return len(self.inner)

    def drop(x, p=0.5, training=True, inplace=False):
        if not training:
            return x
        assert p == MR.P_DROP
        m = state["cur"][state["calls"]]
        state["calls"] += 1
        assert m.shape == tuple(x.shape)
        return x * torch.as_tensor(m).to(x.dtype)

    def eps_like(t, **kw):
        e = state["cur"][3]
        assert e.shape == tuple(t.shape)
        return torch.as_tensor(e).to(t.dtype)

    rec = b.MultVAERecommender(hidden_dim=MR.HIDDEN, latent_dim=MR.LATENT, epochs=epochs)
    rec.device = torch.device("cpu")
    b.MultVAE, b.DataLoader, F.dropout, torch.randn_like = make_model, Loader, drop, eps_like
    try:
        torch.manual_seed(MR.SEED_TORCH)
        rec.fit(matrix)
    finally:
        b.MultVAE, b.DataLoader, F.dropout, torch.randn_like = model_cls, loader_cls, dropout, randn_like
    return rec


QUALITY_CFG = dict(n_users=400, n_items=200, d=4, n_clusters=8)
QUALITY_EPOCHS = 150
QUALITY_SEEDS = list(range(8))


def quality(b):
    """NDCG@10 of 8 seeded fits of the unmodified reference on the planted set."""
    import tempfile
    import pandas as pd
    import torch
    from gen import write_planted_artifacts
    train_m = importlib.import_module("src.ml.train")
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        data, _ = write_planted_artifacts(Path(tmp), QUALITY_CFG)
        full, train_df, val_df, maps = train_m.load_training_data(str(data))
        matrix, _ = b._build_input_matrix(train_df, val_df, maps["user_to_idx"], maps["item_to_idx"], full.shape)
        test_df = pd.read_csv(Path(data) / "test.csv")
        for seed in QUALITY_SEEDS:
            torch.manual_seed(seed)
            np.random.seed(seed)
            rec = b.MultVAERecommender(epochs=QUALITY_EPOCHS)
            rec.device = torch.device("cpu")
            rec.fit(matrix)
            res = b.evaluate_model(rec, "Mult-VAE", matrix, test_df, maps["user_to_idx"], maps["item_to_idx"], [10], 99)
            out.append(res[10]["ndcg"])
    return out


def main():
    import pandas as pd
    import torch
    import_reference()
    b = importlib.import_module("src.ml.baseline")
    matrix = MR.g_small()
    users, tests = MR.fixture_tests(matrix)
    N = matrix.shape[1]
    out, meta = {}, {"seed_torch": MR.SEED_TORCH, "seed_dev": MR.SEED_DEV, "torch": torch.__version__,
                     "numpy": np.__version__, "shape": list(matrix.shape), "nnz": int(matrix.nnz),
                     "hidden": MR.HIDDEN, "latent": MR.LATENT, "epochs": list(MR.FIX_EPOCHS),
                     "bar_factor": MR.BAR_FACTOR, "data_digest": MR.graph_digest(matrix), "noise": {}, "bar": {}}

    torch.manual_seed(MR.SEED_TORCH)
    m0 = b.MultVAE(N, MR.HIDDEN, MR.LATENT)
    init = {k: v.detach().clone() for k, v in m0.state_dict().items()}
    meta["init_digest"] = MR.params_digest(init)
    out["init_w1"] = init["encoder.0.weight"][:4].numpy().copy()
    out["init_bd2"] = init["decoder.2.bias"].numpy().copy()

    runs = {}
    for epochs in MR.FIX_EPOCHS:
        r32d, r64d = {}, {}
        r32, r64 = fit(b, matrix, epochs, False, r32d), fit(b, matrix, epochs, True, r64d)
        assert all(np.array_equal(a, c) for a, c in zip(r32d["orders"], r64d["orders"]))
        s32 = np.stack([r32.predict(int(u)) for u in users]).astype(np.float32)
        s64 = np.stack([r64.predict(int(u)) for u in users])
        assert s64.dtype == np.float64
        out[f"scores_e{epochs}"] = s32
        meta["noise"][f"scores_e{epochs}"] = float(np.abs(s32.astype(np.float64) - s64).max())
        meta[f"max_abs_scores_e{epochs}"] = float(np.abs(s64).max())
        runs[epochs] = (r32, r32d, r64d)
    r32, r32d, r64d = runs[MR.FIX_EPOCHS[-1]]
    assert np.array_equal(runs[1][1]["orders"][0], r32d["orders"][0]) and runs[1][1]["losses"] == r32d["losses"][:2]
    out["orders"] = np.stack(r32d["orders"]).astype(np.int32)
    out["losses"] = np.array(r32d["losses"], np.float32)
    meta["noise"]["losses"] = float(np.abs(np.array(r32d["losses"]) - np.array(r64d["losses"])).max())

    uid, iid = [f"U{u}" for u in range(matrix.shape[0])], [f"I{i}" for i in range(N)]
    test_df = pd.DataFrame({"user_id": [uid[u] for u in users], "asin": [iid[i] for i in tests]})
    u2i, i2i = {u: k for k, u in enumerate(uid)}, {i: k for k, i in enumerate(iid)}
    ranks, ndcg = [], b.ndcg_at_k

    def ndcg_rec(top_k, relevant, k):
        if k == N:
            ranks.append(int(np.flatnonzero(np.asarray(top_k) == relevant[0])[0]))
        return ndcg(top_k, relevant, k)

    b.ndcg_at_k = ndcg_rec
    try:
        metrics = b.evaluate_model(r32, "Mult-VAE", matrix, test_df, u2i, i2i, [5, 10, 20, N], 99)
    finally:
        b.ndcg_at_k = ndcg
    assert len(ranks) == len(users)
    out["ranks"] = np.array(ranks, np.int32)
    meta["metrics"] = {str(k): v for k, v in metrics.items() if k != N}
    meta["bar"] = {k: MR.BAR_FACTOR * v for k, v in meta["noise"].items()}
    for e in MR.FIX_EPOCHS:
        assert meta["bar"][f"scores_e{e}"] <= 1e-3 * meta[f"max_abs_scores_e{e}"], (e, meta["bar"])

    q = quality(b)
    meta["quality"] = {"cfg": QUALITY_CFG, "epochs": QUALITY_EPOCHS, "seeds": QUALITY_SEEDS, "k": 10, "n_negatives": 99,
                       "ndcg": q, "mean": float(np.mean(q)), "std": float(np.std(q, ddof=1))}

    np.savez_compressed(HERE / "multvae.npz", **out)
    (HERE / "multvae_meta.json").write_text(json.dumps(meta, indent=1))
    print(json.dumps({k: meta[k] for k in ("data_digest", "init_digest", "noise", "bar", "quality")}, indent=1))
    print("multvae.npz", (HERE / "multvae.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
