"""`make baseline-lightgcn` without a GPU: the fixture's own consistency, the host half of LightGCNRecommender.fit
(the init draws, the epoch stream and its summation plan) against the reference's recorded draws, the command
line, both Makefile targets, the refused shapes and run_lightgcn through the shared runner."""
import argparse
import json
import subprocess
import sys
from pathlib import Path
from unittest import mock

import numpy as np
import pytest

import lightgcn_ref as LR

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "recommendation-system_amd"


def test_fixture_graph_is_the_rebuilt_one_and_has_its_edge_cases():
    matrix, users, tests = LR.fixture_graph()  # asserts the digest
    meta, fx = LR.fixture_meta(), LR.fixture()
    s = LR.structure(matrix)
    assert list(matrix.shape) == meta["shape"] == [LR.N_USERS, LR.N_ITEMS] and s.nnz == meta["nnz"]
    assert 1024 < s.nnz < 2048
    assert s[LR.EMPTY_USER].nnz == 0 and s[:, LR.EMPTY_ITEM].nnz == 0 and s[:, LR.HOT_ITEM].nnz >= 120
    assert (matrix.data == 2.0).any()
    assert (fx["batch_neg"] == LR.EMPTY_ITEM).any()
    for u, t in zip(users, tests):
        assert matrix[u, t] == 0


def test_fixture_is_internally_consistent():
    matrix, users, tests = LR.fixture_graph()
    meta, fx = LR.fixture_meta(), LR.fixture()
    n, nnz = LR.N_USERS + LR.N_ITEMS, meta["nnz"]
    assert fx["init"].shape == (n, LR.DIM) and fx["init"].dtype == np.float32
    for e in (1, 5):
        assert fx[f"user_e{e}"].shape == (LR.N_USERS, LR.DIM) and fx[f"item_e{e}"].shape == (LR.N_ITEMS, LR.DIM)
    assert fx["batch_users"].shape == fx["batch_pos"].shape == fx["batch_neg"].shape == (nnz,)
    # the positives are a permutation of the matrix's nonzero pairs; the negatives lie in the catalogue
    pu, pi = matrix.nonzero()
    assert sorted(zip(fx["batch_users"].tolist(), fx["batch_pos"].tolist())) == sorted(zip(pu.tolist(), pi.tolist()))
    assert fx["batch_neg"].min() >= 0 and fx["batch_neg"].max() < LR.N_ITEMS
    # the stored scores are the stored embeddings' products, and the stored ranks lie in their own brackets
    want = fx["user_e5"].astype(np.float64) @ fx["item_e5"].astype(np.float64).T
    assert np.abs(fx["scores"] - want).max() < 1e-6
    for u, t, rank in zip(users, tests, fx["ranks"]):
        cand = np.setdiff1d(np.arange(LR.N_ITEMS), np.append(matrix[u].indices, t))
        gt, eq = (fx["scores"][u, cand] > fx["scores"][u, t]).sum(), (fx["scores"][u, cand] == fx["scores"][u, t]).sum()
        assert gt <= rank <= gt + eq
    for key, noise in meta["noise"].items():
        assert 0 < noise < 1e-6 and meta["bar"][key] == pytest.approx(LR.BAR_FACTOR * noise)
    assert set(meta["bar"]) == {"user_e1", "item_e1", "user_e5", "item_e5", "scores"}


def test_init_draws_equal_the_reference_table_bit_for_bit():
    import torch
    import src.ml.lightgcn as lg
    torch.manual_seed(LR.SEED_TORCH)
    table = lg.init_table(LR.N_USERS, LR.N_ITEMS, LR.DIM)
    assert table.dtype == torch.float32 and table.is_contiguous()
    assert np.array_equal(table.numpy().view(np.uint32), LR.fixture()["init"].view(np.uint32))


def test_epoch_stream_equals_the_reference_batches_and_leaves_numpy_where_it_does():
    import src.ml.lightgcn as lg
    matrix, _, _ = LR.fixture_graph()
    fx, meta = LR.fixture(), LR.fixture_meta()
    pu, pi = matrix.nonzero()
    for epochs in (1, 5):
        np.random.seed(LR.SEED_NUMPY)
        for e in range(epochs):
            users, pos, neg = lg.epoch_batches(pu, pi, LR.N_ITEMS)
            assert users.dtype == pos.dtype == neg.dtype == np.int32
            if e == 0:
                assert np.array_equal(users, fx["batch_users"]) and np.array_equal(pos, fx["batch_pos"])
                assert np.array_equal(neg, fx["batch_neg"])
        assert LR.state_digest() == meta["state_digest"][str(epochs)]


@pytest.mark.parametrize("n,batch", [(1, 4), (4, 4), (9, 4), (1290, 1024)])
def test_epoch_plan_is_the_per_batch_plan(n, batch):
    """One sort for the epoch gives every batch ops.lgcn_bpr_plan's stable sort by node, and each group holds one
    node's occurrences in ascending slot order."""
    import src.ml.lightgcn as lg
    from hvae import ops
    rng = np.random.Generator(np.random.PCG64(n))
    n_users, n_items = 7, 5
    users = rng.integers(0, n_users, n).astype(np.int32)
    pos = rng.integers(0, n_items, n).astype(np.int32)
    neg = rng.integers(0, n_items, n).astype(np.int32)
    slots, seg_off, seg_base, n_seg = lg.epoch_plan(users, pos, neg, n_users, n_items, batch)
    assert slots.dtype == seg_off.dtype == np.int32 and len(slots) == 3 * n
    for k, s in enumerate(range(0, n, batch)):
        e = min(s + batch, n)
        want_slots, want_off = ops.lgcn_bpr_plan(users[s:e], pos[s:e], neg[s:e], n_users)
        assert np.array_equal(slots[3 * s:3 * e], want_slots)
        assert np.array_equal(seg_off[seg_base[k]:seg_base[k] + n_seg[k] + 1], want_off) and n_seg[k] == len(want_off) - 1
        nb = e - s
        node = np.concatenate([users[s:e], pos[s:e] + n_users, neg[s:e] + n_users])
        assert want_off[0] == 0 and want_off[-1] == 3 * nb and sorted(want_slots.tolist()) == list(range(3 * nb))
        seen = set()
        for a, b in zip(want_off[:-1], want_off[1:]):
            grp = want_slots[a:b]
            assert b > a and (np.diff(grp) > 0).all() and len(set(node[grp].tolist())) == 1
            assert int(node[grp[0]]) not in seen
            seen.add(int(node[grp[0]]))


def test_cli_flags_and_defaults(monkeypatch):
    import src.ml.lightgcn as lg
    seen = {}

    class _Stop(Exception):
        pass

    def fake_parse(self, args=None, namespace=None):
        seen["parser"] = self
        raise _Stop

    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", fake_parse)
    monkeypatch.setattr(sys, "argv", ["prog"])
    with pytest.raises(_Stop):
        lg.main()
    by_flag = {o: a for a in seen["parser"]._actions for o in a.option_strings}
    assert "--data" in by_flag
    assert by_flag["--n-negatives"].default == 99 and by_flag["--n-negatives"].type is int
    assert by_flag["--k-values"].default == [5, 10, 20] and by_flag["--k-values"].nargs == "+"
    for flag, default, typ in (("--epochs", 50, int), ("--embedding-dim", 64, int), ("--n-layers", 3, int),
                               ("--lr", 1e-3, float), ("--reg", 1e-4, float)):
        assert by_flag[flag].default == default and by_flag[flag].type is typ


def test_cli_passes_its_arguments():
    import src.ml.lightgcn as lg
    argv = ["--data", "d/", "--n-negatives", "0", "--k-values", "3", "7", "--epochs", "2", "--embedding-dim", "128",
            "--n-layers", "2", "--lr", "0.01", "--reg", "0.5"]
    with mock.patch.object(lg, "run_lightgcn") as run, mock.patch.object(sys, "argv", ["lightgcn"] + argv):
        lg.main()
    args, kw = run.call_args
    assert args == ("d/", [3, 7], None)
    assert kw == dict(embedding_dim=128, n_layers=2, epochs=2, lr=0.01, reg=0.5)


def test_recommender_keeps_the_reference_api_and_defaults():
    import src.ml.baseline as b
    import src.ml.lightgcn as lg
    assert issubclass(lg.LightGCNRecommender, b.BaseRecommender)
    m = lg.LightGCNRecommender()
    assert (m.embedding_dim, m.n_layers, m.epochs, m.lr, m.reg) == (64, 3, 50, 1e-3, 1e-4)
    assert m.user_final_emb is None and m.item_final_emb is None
    for meth in ("fit", "predict", "score_candidates", "score_all"):
        assert callable(getattr(m, meth))


@pytest.mark.parametrize("dim", [0, 32, 63, 96, 256])
def test_refused_embedding_dim_names_the_served_ones(dim):
    import src.ml.lightgcn as lg
    with pytest.raises(ValueError) as e:
        lg.LightGCNRecommender(embedding_dim=dim)
    assert "64" in str(e.value) and "128" in str(e.value) and str(dim) in str(e.value)
    assert lg.LightGCNRecommender(embedding_dim=128).embedding_dim == 128


@pytest.mark.parametrize("layers", [0, -1, 9])
def test_refused_n_layers_names_the_served_range(layers):
    import src.ml.lightgcn as lg
    with pytest.raises(ValueError, match="1 to 8"):
        lg.LightGCNRecommender(n_layers=layers)
    for ok in (1, 8):
        assert lg.LightGCNRecommender(n_layers=ok).n_layers == ok


def test_cli_refuses_an_unserved_dim_before_reading_data(tmp_path):
    import src.ml.lightgcn as lg
    with mock.patch.object(sys, "argv", ["lightgcn", "--data", str(tmp_path / "none"), "--embedding-dim", "100"]):
        with pytest.raises(ValueError, match="64 and 128"):
            lg.main()


def test_run_lightgcn_fits_evaluates_and_merges(tmp_path, monkeypatch):
    """run_lightgcn with the device work stubbed out: the train + val matrix, the test frame, the timing entry."""
    import src.ml.baseline as b
    import src.ml.lightgcn as lg
    from gen import write_planted_artifacts
    data, _ = write_planted_artifacts(tmp_path, dict(n_users=30, n_items=40, d=4, n_clusters=2))
    calls = []

    def fake_fit(self, m):
        self.device = None
        calls.append(("fit", m.shape, self.embedding_dim, self.n_layers, self.epochs))

    def fake_eval(model, name, matrix, test_df, u2i, i2i, k_values, n_negatives):
        calls.append((name, matrix.shape, len(test_df), tuple(k_values), n_negatives))
        return {k: {"recall": 0.5, "ndcg": 0.25, "hit_ratio": 0.5} for k in k_values}

    monkeypatch.setattr(lg.LightGCNRecommender, "fit", fake_fit)
    monkeypatch.setattr(b, "evaluate_model", fake_eval)
    res = lg.run_lightgcn(str(data), [5, 10], None, embedding_dim=128, n_layers=2, epochs=3)
    assert calls == [("fit", (30, 40), 128, 2, 3), ("LightGCN", (30, 40), 30, (5, 10), None)]
    out = json.loads((tmp_path / "models" / "figures" / "baseline_results.json").read_text())
    assert list(out) == ["LightGCN"] and list(out["LightGCN"]) == ["5", "10", "training_time_seconds"]
    assert isinstance(out["LightGCN"]["training_time_seconds"], float) and set(res) == {5, 10, "training_time_seconds"}


@pytest.mark.parametrize("target,n_neg", [("baseline-lightgcn", "99"), ("baseline-lightgcn-full", "0")])
def test_makefile_targets(target, n_neg):
    r = subprocess.run(["make", "-n", "-C", str(PKG), target, "PYTHON=python", "DATA_DIR=data"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"python -m src.ml.lightgcn --data data/ --n-negatives {n_neg}" in r.stdout.splitlines()


def test_baseline_module_still_refuses_lightgcn_and_points_here(tmp_path):
    import src.ml.baseline as b
    assert b.SERVED_MODELS == ("Popularity", "Item-KNN")
    with mock.patch.object(sys, "argv", ["baseline", "--data", str(tmp_path / "none"), "--models", "LightGCN"]):
        with pytest.raises(ValueError) as e:
            b.main()
    assert "Popularity" in str(e.value) and "Item-KNN" in str(e.value) and "src.ml.lightgcn" in str(e.value)


def test_abi_declares_binds_and_wraps_the_entry_points():
    from hvae import _lib, ops
    header = (ROOT / "include" / "hvae.h").read_text()
    for name in ("hvae_lgcn_norm", "hvae_lgcn_propagate", "hvae_lgcn_bpr", "hvae_lgcn_bpr_workspace"):
        assert f"{name}(" in header and name in _lib.SIGNATURES
    assert "#define HVAE_ABI_VERSION 6" in header and _lib.ABI_VERSION == 6
    assert f"#define HVAE_LGCN_MAX_BATCH {_lib.LGCN_MAX_BATCH}" in header
    for fn in ("lgcn_norm", "lgcn_propagate", "lgcn_bpr"):
        assert callable(getattr(ops, fn))
