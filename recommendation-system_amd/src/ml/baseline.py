"""Baselines on MI355X -- drop-in for the reference's src/ml/baseline.py (`make baseline`).

Served: the two training-free baselines, Popularity and Item-KNN (reference: baseline.py:57-99), with the
reference's recommender API (fit / predict), evaluate_model (:411-471), run_all_baselines (:474-533) and CLI
(:536-544), and the same models/figures/baseline_results.json. SVD, Mult-VAE and LightGCN are separate trained
models and are not run from here: asking for one is an error, never a silent skip. LightGCN is trained by
src/ml/lightgcn.py (`make baseline-lightgcn`), SVD fitted by src/ml/svd.py (`make baseline-svd`) and Mult-VAE trained
by src/ml/multvae.py (`make baseline-multvae`); each constructs its model and hands it to this module's run_baseline:
the data loading, timing, evaluation, table, results file and common flags are written once, below.

The reference scores one test row at a time in a Python loop; here the rows are batched on the device. Scores
come from libhvae (hvae_csc_col_stats for Popularity, the two-stage hvae_knn_* kernels for Item-KNN), the
99-negative protocol ranks with hvae_rank_first and full ranking with hvae_topk. Negatives are the reference's,
draw for draw from numpy's global stream (hvae_negatives_legacy), which is left where the reference's per-row
np.random.choice calls would leave it, so the second model's draws follow the first's as they do there.

Ties. The reference ranks with numpy's default (unstable) argsort, so where the test item's score equals other
candidates' -- most rows for Popularity, and for Item-KNN on sparse data -- its rank is some position inside
[#greater, #greater + #equal] that depends on numpy's sort internals: its metrics are not a reproducible target.
This module uses the project's convention, the order of a stable ascending argsort reversed: the test item ranks
after its equals in the 99-negative protocol (hvae_rank_first), and full ranking breaks ties by larger item index
first (hvae_topk). Scores match the reference's to one fp32 rounding, and every rank lies in the reference's
bracket.
"""
from __future__ import annotations

import argparse
import json
import logging
import time
from abc import ABC, abstractmethod
from pathlib import Path

import numpy as np
import pandas as pd
import torch
from scipy.sparse import csr_matrix

from hvae import ops

from ..config import config
from .evaluate import RecommendationEvaluator, _get_device, metrics_from_rank
from .train import load_training_data

logging.basicConfig(level=logging.INFO)
logger = logging.getLogger(__name__)

SERVED_MODELS = ("Popularity", "Item-KNN")
REFERENCE_ONLY_MODELS = ("SVD", "Mult-VAE", "LightGCN")
TOPK_MAX = 64                 # hvae_topk (include/hvae.h)
KNN_T_BUDGET = 1 << 30        # bytes of the Item-KNN stage-1 matrix T [n_users, batch] fp64
MAX_BATCH = 4096
_METRICS = ("recall", "ndcg", "hit_ratio")


# =============================================================================
# Recommenders (reference: baseline.py:38-99)
# =============================================================================


class BaseRecommender(ABC):
    """The reference's recommender API plus the batched device methods the evaluation uses."""

    device: torch.device | None = None

    @abstractmethod
    def fit(self, interaction_matrix: csr_matrix) -> None:
        """Fit the model."""

    @abstractmethod
    def predict(self, user_idx: int) -> np.ndarray:
        """Predict scores for all items for a user."""

    @abstractmethod
    def score_candidates(self, users: np.ndarray, cand: torch.Tensor) -> torch.Tensor:
        """fp32 [B, C] device scores of cand [B, C] (int32, device) for the users [B]."""

    @abstractmethod
    def score_all(self, users: np.ndarray) -> torch.Tensor:
        """fp32 [B, N] device scores of every item for the users [B]; the caller may overwrite the result."""

    max_batch = MAX_BATCH


def _resolve_device(device) -> torch.device:
    dev = _get_device(str(device) if device is not None else None)
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


class PopularityRecommender(BaseRecommender):
    """Non-personalised: score[j] = sum_v M[v, j] for every user (reference: baseline.py:57-68)."""

    def __init__(self, device=None):
        self.scores = None
        self._device_arg = device

    def fit(self, interaction_matrix: csr_matrix) -> None:
        logger.info("Fitting Popularity baseline...")
        self.device = _resolve_device(self._device_arg)
        csc = ops.csc_from_scipy(interaction_matrix, self.device)
        self._scores_dev, _ = ops.csc_col_stats(csc)
        self.scores = self._scores_dev.cpu().numpy().astype(np.float64)

    def predict(self, user_idx: int) -> np.ndarray:
        return self.scores.copy()

    def score_candidates(self, users: np.ndarray, cand: torch.Tensor) -> torch.Tensor:
        return self._scores_dev[cand.long()]

    def score_all(self, users: np.ndarray) -> torch.Tensor:
        return self._scores_dev.unsqueeze(0).expand(len(users), -1).contiguous()


class ItemKNNRecommender(BaseRecommender):
    """Item-based collaborative filtering with cosine similarity (reference: baseline.py:71-99). As there, k is
    stored and never used: every interacted item's similarity counts. The dense path's zeroed diagonal
    (n_items <= 10000, :84-87) and the on-the-fly path's kept one (:97-99) are both reproduced (zero_diag)."""

    def __init__(self, k: int = 50, device=None):
        self.k = k
        self.similarity = None  # the reference's dense N x N matrix is never formed here
        self.matrix = None
        self._device_arg = device
        self._T = None

    def fit(self, interaction_matrix: csr_matrix) -> None:
        logger.info(f"Fitting Item-KNN (k={self.k})...")
        self.device = _resolve_device(self._device_arg)
        self.matrix = interaction_matrix
        self.n_users, self.n_items = interaction_matrix.shape
        self.zero_diag = self.n_items <= 10000
        self._csr = ops.csr_from_scipy(interaction_matrix, self.device)
        self._csc = ops.csc_from_scipy(interaction_matrix, self.device)
        _, self._inv_norm = ops.csc_col_stats(self._csc)
        per_row = max(ops.knn_workspace_bytes(1, self.n_users), 1)
        self.max_batch = int(max(1, min(MAX_BATCH, KNN_T_BUDGET // per_row)))
        self._T = None

    def _stage1(self, users: np.ndarray):
        rows = torch.as_tensor(np.ascontiguousarray(users, dtype=np.int32), device=self.device)
        if len(users) > self.max_batch:
            raise ValueError(f"Item-KNN: a batch of {len(users)} users exceeds max_batch {self.max_batch} "
                             f"(T stays under {KNN_T_BUDGET} bytes)")
        x = ops.Csr(self._csr.row_ptr, self._csr.col_idx, self._csr.vals, self.n_items, rows=rows)
        need = ops.knn_workspace_bytes(x.nb, self.n_users) // 8
        if self._T is None or self._T.numel() < need:
            self._T = None  # release before growing
            self._T = torch.empty(max(need, 1), dtype=torch.float64, device=self.device)
        ops.knn_user_weights(x, self._csc, self._inv_norm, self._T)
        return x

    def predict(self, user_idx: int) -> np.ndarray:
        return self.score_all(np.array([user_idx]))[0].cpu().numpy().astype(np.float64)

    def score_candidates(self, users: np.ndarray, cand: torch.Tensor) -> torch.Tensor:
        x = self._stage1(users)
        return ops.knn_score_candidates(x, self._csc, self._inv_norm, self._T, cand.contiguous(), self.zero_diag)

    def score_all(self, users: np.ndarray) -> torch.Tensor:
        x = self._stage1(users)
        return ops.knn_scores(x, self._csc, self._inv_norm, self._T, self.zero_diag)


BASELINES = {
    "Popularity": lambda: PopularityRecommender(),
    "Item-KNN": lambda: ItemKNNRecommender(k=50),
}


# =============================================================================
# Evaluation (reference: baseline.py:393-471)
# =============================================================================


def _build_input_matrix(train_df: pd.DataFrame, val_df: pd.DataFrame, user_to_idx: dict, item_to_idx: dict,
                        shape: tuple) -> tuple[csr_matrix, pd.DataFrame]:
    """Train + val positives as one matrix, duplicate pairs summed (reference: baseline.py:393-408)."""
    train_pos = train_df[train_df["binary_rating"] == 1] if "binary_rating" in train_df.columns else train_df
    val_pos = val_df[val_df["binary_rating"] == 1] if "binary_rating" in val_df.columns else val_df
    combined = pd.concat([train_pos, val_pos])
    rows = combined["user_id"].map(user_to_idx)
    cols = combined["asin"].map(item_to_idx)
    matrix = csr_matrix((np.ones(len(combined)), (rows, cols)), shape=shape)
    return matrix, combined


def rank_first_host(scores: np.ndarray, count: int | None = None) -> int:
    """0-based rank of candidate 0 among scores[:1 + count]: #greater + #equal, i.e. its position in
    candidates[np.argsort(scores, kind="stable")[::-1]] (hvae_rank_first's rule, for rows shorter than the block)."""
    row = scores if count is None else scores[:1 + int(count)]
    return int((row[1:] > row[0]).sum() + (row[1:] == row[0]).sum())


def position_in_topk(topk_idx: np.ndarray, tests: np.ndarray) -> np.ndarray:
    """Per row, the position of tests[r] in topk_idx[r] (a ranked list), or a rank past every k when absent."""
    hit = topk_idx == np.asarray(tests)[:, None]
    return np.where(hit.any(axis=1), hit.argmax(axis=1), np.iinfo(np.int32).max).astype(np.int64)


def candidate_ranks(model: BaseRecommender, users: np.ndarray, tests: np.ndarray, negatives) -> np.ndarray:
    """0-based rank of each row's test item among [test] + negatives, batched on the device; negatives as
    RecommendationEvaluator._candidates takes them."""
    R = len(users)
    cand, pad, cnt = RecommendationEvaluator._candidates(tests, negatives)
    out = np.empty(R, np.int64)
    bs = model.max_batch
    for s in range(0, R, bs):
        e = min(R, s + bs)
        sc = model.score_candidates(users[s:e], torch.as_tensor(cand[s:e], device=model.device))
        out[s:e] = ops.rank_first(sc).cpu().numpy()
        if pad[s:e].any():  # fewer available items than requested: rank over the row's own candidates only
            scn = sc.cpu().numpy()
            for r in np.nonzero(pad[s:e])[0]:
                out[s + r] = rank_first_host(scn[r], cnt[s + r])
    return out


def full_ranking_positions(model: BaseRecommender, matrix: csr_matrix, users: np.ndarray, tests: np.ndarray,
                           K: int) -> np.ndarray:
    """Position of each row's test item in the top-K of all items with the row's seen items masked
    (ties: larger item index first), or past every k when it is not among them."""
    if K > TOPK_MAX:
        raise ValueError(f"full ranking: max(k_values) = {K}, but hvae_topk serves K <= {TOPK_MAX}")
    n_items = matrix.shape[1]
    K = min(K, n_items)
    seen = ops.csr_from_scipy(matrix, model.device)
    out = np.empty(len(users), np.int64)
    bs = model.max_batch
    for s in range(0, len(users), bs):
        e = min(len(users), s + bs)
        rows = torch.as_tensor(np.ascontiguousarray(users[s:e], dtype=np.int32), device=model.device)
        excl = ops.Csr(seen.row_ptr, seen.col_idx, seen.vals, n_items, rows=rows)
        idx, _ = ops.topk(model.score_all(users[s:e]), K, exclude=excl)
        out[s:e] = position_in_topk(idx.cpu().numpy(), tests[s:e])
    return out


def evaluate_ranks(model: BaseRecommender, matrix: csr_matrix, users: np.ndarray, tests: np.ndarray,
                   k_values: list[int], n_negatives: int | None) -> np.ndarray:
    """The per-row ranks behind evaluate_model's metrics. With negatives, one hvae_negatives_legacy call draws
    every row's from numpy's global stream, in row order."""
    users = np.asarray(users, np.int64)
    tests = np.asarray(tests, np.int64)
    if len(users) == 0:
        return np.empty(0, np.int64)
    with torch.no_grad():
        if n_negatives is not None:
            m = matrix.tocsr()
            negs = ops.negatives_legacy(m.indptr, m.indices, matrix.shape[1], users, tests, n_negatives, arrays=True)
            return candidate_ranks(model, users, tests, negs)
        return full_ranking_positions(model, matrix, users, tests, max(k_values))


def evaluate_model(model: BaseRecommender, name: str, matrix: csr_matrix, test_df: pd.DataFrame, user_to_idx: dict,
                   item_to_idx: dict, k_values: list[int] | None = None,
                   n_negatives: int | None = 99) -> dict[int, dict[str, float]]:
    """Evaluate a recommender model (reference: baseline.py:411-471), every known test row, one relevant item."""
    k_values = k_values or [5, 10, 20]
    protocol = f"negative sampling ({n_negatives})" if n_negatives else "full ranking"
    logger.info(f"Evaluating {name} with {protocol}...")
    users, tests = [], []
    for user_id, item_id in zip(test_df["user_id"].tolist(), test_df["asin"].tolist()):
        if user_id not in user_to_idx or item_id not in item_to_idx:
            continue
        users.append(user_to_idx[user_id])
        tests.append(item_to_idx[item_id])
    rank = evaluate_ranks(model, matrix, users, tests, k_values, n_negatives)
    per_row = metrics_from_rank(rank, k_values)
    return {k: {m: float(np.mean(per_row[k][m])) if len(rank) else 0.0 for m in _METRICS} for k in k_values}


def _select_models(models) -> list[str]:
    names = list(models) if models else list(SERVED_MODELS)
    bad = [n for n in names if n not in SERVED_MODELS]
    if bad:
        raise ValueError(f"baseline model(s) {bad} are not served on this path: only {SERVED_MODELS[0]} and "
                         f"{SERVED_MODELS[1]} are ({', '.join(REFERENCE_ONLY_MODELS)} are separate trained models "
                         "that are not run from here; LightGCN has its own command, python -m src.ml.lightgcn, "
                         "SVD has python -m src.ml.svd, Mult-VAE has python -m src.ml.multvae)")
    return names


# =============================================================================
# The runner (reference: baseline.py:474-544): every baseline command goes through these
# =============================================================================


def load_eval_data(data_dir: str) -> tuple[csr_matrix, pd.DataFrame, dict, dict]:
    """What an evaluation reads from a data directory: (the train + val input matrix, the test frame, user_to_idx,
    item_to_idx)."""
    full_matrix, train_df, val_df, mappings = load_training_data(data_dir)
    user_to_idx, item_to_idx = mappings["user_to_idx"], mappings["item_to_idx"]
    input_matrix, _ = _build_input_matrix(train_df, val_df, user_to_idx, item_to_idx, full_matrix.shape)
    return input_matrix, pd.read_csv(Path(data_dir) / "test.csv"), user_to_idx, item_to_idx


def fit_and_evaluate(model: BaseRecommender, name: str, data: tuple, k_values: list[int],
                     n_negatives: int | None) -> dict:
    """Fit a constructed model on load_eval_data's matrix (timed to the end of its device work), evaluate it, and
    return evaluate_model's results with training_time_seconds added."""
    input_matrix, test_df, user_to_idx, item_to_idx = data
    logger.info(f"\n{'=' * 60}\nTraining {name}\n{'=' * 60}")
    start_time = time.time()
    model.fit(input_matrix)
    if model.device is not None:
        torch.cuda.synchronize(model.device)
    training_time = round(time.time() - start_time, 2)
    logger.info(f"{name} training time: {training_time:.1f}s")
    results = evaluate_model(model, name, input_matrix, test_df, user_to_idx, item_to_idx, k_values, n_negatives)
    results["training_time_seconds"] = training_time
    return results


def write_results(all_results: dict, data_dir: str, keep_existing: bool) -> Path:
    """Set the entries of all_results in <data>/../models/figures/baseline_results.json, the reference's layout
    (baseline.py:522-531). With keep_existing the file's other entries stay, in their order (a one-model command
    beside `make baseline`'s entries); without it the file is replaced, as the reference does."""
    figures_path = Path(data_dir).parent / "models" / "figures"
    figures_path.mkdir(parents=True, exist_ok=True)
    out = figures_path / "baseline_results.json"
    merged = json.loads(out.read_text()) if keep_existing and out.exists() else {}
    merged.update({m: {str(k): v for k, v in metrics.items()} for m, metrics in all_results.items()})
    with open(out, "w") as f:
        json.dump(merged, f, indent=2)
    return out


def print_table(all_results: dict, k_values: list[int]) -> None:
    cols = [(f"Recall@{k}", k, "recall") for k in k_values] + [(f"NDCG@{k}", k, "ndcg") for k in k_values]
    width = 15 + 13 * len(cols)
    print(f"\n{'-' * width}\n{'Model':<15}" + "".join(f" | {c[0]:>10}" for c in cols) + f"\n{'-' * width}")
    for name, metrics in all_results.items():
        print(f"{name:<15}" + "".join(f" | {metrics[k][m]:>10.4f}" for _, k, m in cols))
    print("-" * width)


def run_baseline(model: BaseRecommender, name: str, data_dir: str, k_values: list[int] | None,
                 n_negatives: int | None) -> dict:
    """Fit and evaluate one constructed model as run_all_baselines does, and set its entry of the results file
    beside the others."""
    k_values = k_values or [5, 10, 20]
    results = fit_and_evaluate(model, name, load_eval_data(data_dir), k_values, n_negatives)
    print_table({name: results}, k_values)
    logger.info(f"Saved to {write_results({name: results}, data_dir, keep_existing=True)}")
    return results


def run_all_baselines(data_dir: str, k_values: list[int] | None = None, n_negatives: int | None = 99,
                      models: list[str] | None = None) -> dict:
    """Run the baselines one after the other on one numpy stream (reference: baseline.py:474-533)."""
    k_values = k_values or [5, 10, 20]
    names = _select_models(models)
    data = load_eval_data(data_dir)
    all_results = {name: fit_and_evaluate(BASELINES[name](), name, data, k_values, n_negatives) for name in names}

    protocol = f"negative sampling ({n_negatives})" if n_negatives else "full ranking"
    logger.info(f"\n{'=' * 70}\nBASELINE COMPARISON ({protocol})\n{'=' * 70}")
    print_table(all_results, k_values)
    logger.info(f"Saved to {write_results(all_results, data_dir, keep_existing=False)}")
    return all_results


def parse_args(description: str, add_flags=None) -> argparse.Namespace:
    """The command line every baseline command shares (reference: baseline.py:536-544) plus the flags add_flags(parser)
    adds; --n-negatives 0 (full ranking) comes back as None."""
    parser = argparse.ArgumentParser(description=description)
    parser.add_argument("--data", default=str(config.DATA_DIR))
    parser.add_argument("--n-negatives", type=int, default=99, help="0 for full ranking")
    parser.add_argument("--k-values", type=int, nargs="+", default=[5, 10, 20])
    if add_flags is not None:
        add_flags(parser)
    args = parser.parse_args()
    args.n_negatives = args.n_negatives if args.n_negatives > 0 else None
    return args


def main() -> None:
    args = parse_args("Evaluate the training-free baselines (MI355X)", lambda p: p.add_argument(
        "--models", nargs="+", default=list(SERVED_MODELS),
        help="baselines to run, in order (served: Popularity, Item-KNN)"))
    run_all_baselines(args.data, args.k_values, args.n_negatives, models=args.models)


if __name__ == "__main__":
    main()
