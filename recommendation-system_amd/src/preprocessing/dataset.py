"""Step 2 of `make preprocess`: cleaned reviews -> train.csv / val.csv / test.csv, interaction_matrix.pkl,
mappings.pkl and dataset_stats.pkl, a drop-in for the reference's src/preprocessing/dataset.py (the same class,
functions, CLI flags, defaults and files, plus --seed).

pandas reads the file and carries every column; the index work runs on the GPU (libhvae, K23): the label encoding
of user_id and asin (hvae_prep_encode), the interaction matrix (hvae_prep_csr) and the leave-one-out split
(hvae_prep_split: one stable sort by (user, timestamp) and the membership of every sorted record). pandas then
takes the rows of each output frame once. The negatives are drawn on the host by the native sampler, draw for draw
numpy's. There is no host fallback for the device stages.

Differences from the reference, all stated in DESIGN.md 4.10: ids are strings of at most 32 bytes of UTF-8 without
NUL; timestamps are int64, datetime64 or float64; a user with fewer candidate items than draws is refused (the
reference would sample with replacement through another generator); mappings.pkl holds the four dictionaries and
not the two scikit-learn LabelEncoder objects, which nothing reads.
"""
from __future__ import annotations

import argparse
import logging
import pickle
from pathlib import Path

import numpy as np
import pandas as pd
from scipy.sparse import csr_matrix

from ..config import config
from .cleaning import encode_column

logging.basicConfig(level=logging.INFO, format="%(levelname)s:%(name)s:%(message)s")
logger = logging.getLogger(__name__)

_I64_MAX = np.iinfo(np.int64).max


def timestamp_keys(col) -> np.ndarray:
    """A timestamp column as int64 sort keys in the column's own order: int64 as it is, datetime64 by its integer
    count (NaT last), float64 by the usual order-preserving map of its bits (NaN last). Other dtypes are refused."""
    values = col.to_numpy() if hasattr(col, "to_numpy") else np.asarray(col)
    kind = values.dtype.kind
    if kind == "i" or kind == "u":
        if kind == "u" and values.dtype.itemsize == 8 and len(values) and values.max() > _I64_MAX:
            raise ValueError("timestamp: uint64 values above 2^63 - 1 are not supported")
        return values.astype(np.int64)
    if kind == "M":
        keys = values.view(np.int64).copy()
        keys[np.isnat(values)] = _I64_MAX
        return keys
    if kind == "f" and values.dtype.itemsize == 8:
        x = values + 0.0  # -0.0 -> +0.0: the two compare equal
        bits = x.view(np.int64)
        keys = bits ^ ((bits >> 63) & _I64_MAX)
        keys[np.isnan(x)] = _I64_MAX
        return keys
    raise ValueError(f"timestamp: dtype {values.dtype} is not supported (int64, datetime64 or float64)")


class DatasetBuilder:
    """Builder for recommendation datasets with train/val/test splits."""

    def __init__(self, device=None):
        import torch
        self.device = torch.device(device) if device is not None else torch.device("cuda", 0)
        self.user_to_idx: dict[str, int] = {}
        self.item_to_idx: dict[str, int] = {}
        self.idx_to_user: dict[int, str] = {}
        self.idx_to_item: dict[int, str] = {}
        self._items = np.zeros(0, dtype=object)  # classes in code order
        self._fitted = None  # (frame, user codes, item codes) of fit_encoders: device tensors

    def fit_encoders(self, df: pd.DataFrame) -> None:
        """The sorted distinct user_id and asin values, as LabelEncoder.classes_ would list them."""
        if len(df) == 0:
            raise ValueError("fit_encoders: the frame has no rows")
        ucode, users = encode_column(df["user_id"].values, "user_id", self.device)
        icode, items = encode_column(df["asin"].values, "asin", self.device)
        self.user_to_idx = {u: i for i, u in enumerate(users)}
        self.item_to_idx = {it: i for i, it in enumerate(items)}
        self.idx_to_user = {i: u for u, i in self.user_to_idx.items()}
        self.idx_to_item = {i: it for it, i in self.item_to_idx.items()}
        self._items = items
        self._fitted = (df, ucode, icode)
        logger.info(f"Encoded {len(self.user_to_idx)} users, {len(self.item_to_idx)} items")

    def _codes(self, df: pd.DataFrame):
        """(frame, user codes, item codes) on the device: the fitted frame's own codes, or a dictionary lookup for
        another frame, whose rows with an unknown user or item are dropped with a warning as in the reference."""
        import torch
        if self._fitted is not None and df is self._fitted[0]:
            return self._fitted
        user_idx = df["user_id"].map(self.user_to_idx)
        item_idx = df["asin"].map(self.item_to_idx)
        valid = (user_idx.notna() & item_idx.notna()).to_numpy()
        if not valid.all():
            logger.warning(f"Dropping {(~valid).sum()} unmapped interactions")
            df, user_idx, item_idx = df[valid], user_idx[valid], item_idx[valid]
        to_dev = lambda s: torch.from_numpy(s.to_numpy().astype(np.int32)).to(self.device)  # noqa: E731
        return df, to_dev(user_idx), to_dev(item_idx)

    def create_interaction_matrix(self, df: pd.DataFrame) -> csr_matrix:
        """The users x items matrix of binary_rating in float32: duplicate pairs summed, columns sorted, explicit
        zeros stored."""
        import torch

        from hvae import ops
        df, ucode, icode = self._codes(df)
        n_users, n_items = len(self.user_to_idx), len(self.item_to_idx)
        if len(df) == 0:
            return csr_matrix((n_users, n_items), dtype=np.float32)
        vals = torch.from_numpy(df["binary_rating"].to_numpy().astype(np.float32)).to(self.device)
        m = ops.prep_csr(ucode, icode, vals, n_users, n_items)
        matrix = csr_matrix((m.vals.cpu().numpy(), m.col_idx.cpu().numpy(), m.row_ptr.cpu().numpy()),
                            shape=(n_users, n_items), dtype=np.float32)
        logger.info(f"Matrix shape: {matrix.shape}, density: {matrix.nnz / (n_users * n_items):.6f}")
        return matrix

    def leave_one_out_split(self, df: pd.DataFrame):
        """test = each user's most recent record (users with 2 or more), val = the one before it (3 or more),
        train = the rest; every frame in (user_id, timestamp) order, ties in input order."""
        from hvae import ops
        df, ucode, _ = self._codes(df)
        if len(df) == 0:
            empty = df.reset_index(drop=True)
            return empty, empty.copy(), empty.copy()
        import torch
        ts = torch.from_numpy(timestamp_keys(df["timestamp"])).to(self.device)
        _, train, val, test = ops.prep_split(ucode, ts, len(self.user_to_idx))
        take = lambda idx: df.take(idx.cpu().numpy()).reset_index(drop=True)  # noqa: E731
        train_df, val_df, test_df = take(train), take(val), take(test)
        logger.info(f"Split: train={len(train_df)}, val={len(val_df)}, test={len(test_df)}")
        return train_df, val_df, test_df

    def create_negative_samples(self, df: pd.DataFrame, interaction_matrix: csr_matrix,
                                n_negatives_per_positive: int = 4) -> pd.DataFrame:
        """Per user of df in ascending id order, n_negatives_per_positive x (the user's rows) items the user has no
        entry for in interaction_matrix, drawn as np.random.choice(candidates, n, replace=False) would from numpy's
        global generator; appended after df with binary_rating 0, timestamp and rating 0 and '' elsewhere."""
        from hvae import ops
        n_items = len(self.item_to_idx)
        m = interaction_matrix.tocsr()
        if not m.has_canonical_format:
            m = m.copy()
            m.sum_duplicates()
        ucode = df["user_id"].map(self.user_to_idx).to_numpy()
        per_user = np.bincount(ucode.astype(np.int64), minlength=len(self.user_to_idx))
        candidates = n_items - np.diff(m.indptr)
        users = np.flatnonzero((per_user > 0) & (candidates > 0))
        n_draw = per_user[users] * int(n_negatives_per_positive)
        short = np.flatnonzero(candidates[users] < n_draw)
        if len(short):
            u = int(users[short[0]])
            raise ValueError(
                f"create_negative_samples: user {self.idx_to_user[u]!r} has {int(candidates[u])} candidate items for "
                f"{int(n_draw[short[0]])} draws; sampling with replacement is not served: lower --n-negatives or "
                "pass --no-negatives")
        if len(n_draw) and int(n_draw.max()) > 32767:
            raise ValueError(f"create_negative_samples: {int(n_draw.max())} draws for one user; at most 32767 are "
                             "served: lower --n-negatives or pass --no-negatives")
        sampled, _ = ops.negatives_legacy_rows(m.indptr, m.indices, n_items, users, n_draw)
        total = len(sampled)
        user_col = np.empty(len(users), dtype=object)
        user_col[:] = [self.idx_to_user[int(u)] for u in users]
        neg_data = {}
        for col in df.columns:
            if col == "user_id":
                neg_data[col] = np.repeat(user_col, n_draw)
            elif col == "asin":
                neg_data[col] = self._items[sampled] if total else np.zeros(0, dtype=object)
            elif col in ("binary_rating", "timestamp", "rating"):
                neg_data[col] = [0] * total
            else:
                neg_data[col] = [""] * total
        neg_df = pd.DataFrame(neg_data)
        combined = pd.concat([df, neg_df], ignore_index=True)
        logger.info(f"Added {len(neg_df)} negatives, total: {len(combined)}")
        return combined

    def save_dataset(self, train_df, val_df, test_df, interaction_matrix: csr_matrix, output_dir) -> None:
        """train.csv, val.csv, test.csv, interaction_matrix.pkl, mappings.pkl and dataset_stats.pkl under output_dir."""
        out = Path(output_dir)
        out.mkdir(parents=True, exist_ok=True)
        train_df.to_csv(out / "train.csv", index=False)
        val_df.to_csv(out / "val.csv", index=False)
        test_df.to_csv(out / "test.csv", index=False)
        with open(out / "interaction_matrix.pkl", "wb") as f:
            pickle.dump(interaction_matrix, f)
        mappings = {
            "user_to_idx": self.user_to_idx,
            "item_to_idx": self.item_to_idx,
            "idx_to_user": self.idx_to_user,
            "idx_to_item": self.idx_to_item,
        }
        with open(out / "mappings.pkl", "wb") as f:
            pickle.dump(mappings, f)
        n_users, n_items = len(self.user_to_idx), len(self.item_to_idx)
        stats = {
            "n_users": n_users,
            "n_items": n_items,
            "train_interactions": len(train_df),
            "val_interactions": len(val_df),
            "test_interactions": len(test_df),
            "matrix_density": interaction_matrix.nnz / (n_users * n_items),
        }
        with open(out / "dataset_stats.pkl", "wb") as f:
            pickle.dump(stats, f)
        logger.info(f"Saved to {out}: {stats['n_users']} users, {stats['n_items']} items")


def build_recommendation_dataset(input_path, output_dir, add_negatives: bool = True,
                                 n_negatives_per_positive: int = 4, seed: int | None = None) -> None:
    """Cleaned reviews (.csv or .jsonl) -> the dataset directory. seed (not in the reference) seeds numpy's global
    generator before the negatives are drawn; None leaves its state as it is, which is what the reference does."""
    logger.info(f"Loading data from {input_path}")
    path = str(input_path)
    if path.endswith(".csv"):
        df = pd.read_csv(path)
    elif path.endswith(".jsonl"):
        df = pd.read_json(path, lines=True)
    else:
        raise ValueError("Input must be CSV or JSONL")
    if seed is not None:
        np.random.seed(seed)

    builder = DatasetBuilder()
    builder.fit_encoders(df)
    matrix = builder.create_interaction_matrix(df)
    train_df, val_df, test_df = builder.leave_one_out_split(df)
    if add_negatives and not train_df.empty:
        train_df = builder.create_negative_samples(train_df, matrix, n_negatives_per_positive)
    builder.save_dataset(train_df, val_df, test_df, matrix, output_dir)


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Build recommendation dataset")
    parser.add_argument("--input", default=config.PROCESSED_DATA_FILE)
    parser.add_argument("--output", default=str(config.DATA_DIR / "processed_dataset"))
    parser.add_argument("--no-negatives", action="store_true")
    parser.add_argument("--n-negatives", type=int, default=4)
    parser.add_argument("--seed", type=int, default=None,
                        help="seed numpy's global generator before the negatives are drawn (default: leave it as it is)")
    return parser


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    build_recommendation_dataset(
        input_path=args.input,
        output_dir=args.output,
        add_negatives=not args.no_negatives,
        n_negatives_per_positive=args.n_negatives,
        seed=args.seed,
    )


if __name__ == "__main__":
    main()
