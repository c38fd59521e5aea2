"""Step 1 of `make preprocess`: raw Amazon Reviews JSONL -> cleaned_reviews.csv / .jsonl, a drop-in for the
reference's src/preprocessing/cleaning.py (the same functions, CLI flags, defaults and files).

pandas reads the file and carries the text columns, as in the reference. The k-core filter
(filter_by_interactions, reference cleaning.py:86-117) runs on the GPU: the ids are label-encoded by
hvae_prep_encode, every round of the filter is enqueued at once by hvae_prep_kcore, and one boolean mask comes
back for a single row selection. There is no host fallback: without the device the filter raises.
"""
from __future__ import annotations

import argparse
import json
import logging
from pathlib import Path

import numpy as np
import pandas as pd

from ..config import config

logging.basicConfig(level=logging.INFO, format="%(levelname)s:%(name)s:%(message)s")
logger = logging.getLogger(__name__)

REQUIRED_FIELDS = ["user_id", "asin", "rating", "title", "text", "timestamp"]


def load_jsonl(file_path) -> pd.DataFrame:
    """One record per line; a line that is not JSON is skipped with a warning (reference cleaning.py:24-38)."""
    logger.info(f"Loading JSONL from {file_path}")
    records = []
    with open(file_path, encoding="utf-8") as f:
        for i, line in enumerate(f):
            try:
                records.append(json.loads(line))
            except json.JSONDecodeError as e:
                logger.warning(f"Skipping malformed JSON at line {i + 1}: {e}")
    df = pd.DataFrame(records)
    logger.info(f"Loaded {len(df):,} records")
    return df


def validate_and_select_fields(df: pd.DataFrame) -> pd.DataFrame:
    """The six required columns, in the reference's order; ValueError when one is absent."""
    missing = set(REQUIRED_FIELDS) - set(df.columns)
    if missing:
        raise ValueError(f"Missing required fields: {missing}")
    logger.info("All required fields present")
    return df[REQUIRED_FIELDS].copy()


def clean_data(df: pd.DataFrame) -> pd.DataFrame:
    """Rows without user_id, asin or rating go; a missing title or text becomes ''."""
    initial_size = len(df)
    df = df.dropna(subset=["user_id", "asin", "rating"]).copy()
    df["title"] = df["title"].fillna("")
    df["text"] = df["text"].fillna("")
    logger.info(f"Cleaned: {initial_size:,} -> {len(df):,} rows ({initial_size - len(df):,} removed)")
    return df


def add_derived_fields(df: pd.DataFrame, rating_threshold: float = 4.0) -> pd.DataFrame:
    """item_text = title + ' ' + text, stripped, runs of whitespace collapsed; rows whose rating is no number go;
    binary_rating = rating >= threshold."""
    df = df.copy()
    item_text = (df["title"].astype(str) + " " + df["text"].astype(str)).str.strip()
    df["item_text"] = item_text.str.replace(r"\s+", " ", regex=True)
    df["rating"] = pd.to_numeric(df["rating"], errors="coerce")
    df = df.dropna(subset=["rating"]).copy()
    df["binary_rating"] = (df["rating"] >= rating_threshold).astype(int)
    if len(df):
        logger.info(f"Positive ratio: {df['binary_rating'].mean():.1%}")
        logger.info(f"Avg item_text length: {df['item_text'].str.len().mean():.0f} chars")
    return df


def encode_column(values, what: str, device=None):
    """LabelEncoder.fit_transform of a column of string ids on the device -> (codes int32 device tensor, the
    classes as an object array in ascending order). ValueError for an id the packing refuses (hvae.ops.prep_pack_ids)."""
    import torch

    from hvae import ops
    dev = torch.device(device) if device is not None else torch.device("cuda", 0)
    arr = np.asarray(values, dtype=object)
    words, _ = ops.prep_pack_ids(arr, what)
    keys = torch.from_numpy(words.view(np.int64)).to(dev)
    codes, first = ops.prep_encode(keys)
    return codes, arr[first.cpu().numpy()]


def filter_by_interactions(df: pd.DataFrame, min_user: int = 5, min_item: int = 5,
                           max_iterations: int = 10) -> pd.DataFrame:
    """The iterative k-core filter: users below min_user interactions go, then items below min_item, until a round
    changes nothing or max_iterations rounds have run. Row order is kept."""
    from hvae import ops
    logger.info(f"Filtering (min_user={min_user}, min_item={min_item})")
    if len(df):
        ucode, users = encode_column(df["user_id"].values, "user_id")
        icode, items = encode_column(df["asin"].values, "asin")
        alive, n_alive, rounds = ops.prep_kcore(ucode, icode, len(users), len(items), min_user, min_item,
                                                max_iterations)
        if rounds < max_iterations:
            logger.info(f"Converged after {rounds + 1} iterations")
        df = df[alive.cpu().numpy()]
        assert len(df) == n_alive
    n_users, n_items = df["user_id"].nunique(), df["asin"].nunique()
    sparsity = 1 - len(df) / (n_users * n_items) if n_users * n_items > 0 else 0
    logger.info(f"Final: {len(df):,} interactions, {n_users:,} users, {n_items:,} items")
    logger.info(f"Sparsity: {sparsity:.4f}")
    return df


def preprocess_amazon_reviews(input_path, output_path, min_user_interactions: int = 5,
                              min_item_interactions: int = 5, rating_threshold: float = 4.0) -> pd.DataFrame:
    """load -> select -> clean -> derive -> filter, then <output>.csv and <output>.jsonl (the suffix of output_path
    is replaced, as in the reference)."""
    df = load_jsonl(input_path)
    df = validate_and_select_fields(df)
    df = clean_data(df)
    df = add_derived_fields(df, rating_threshold)
    df = filter_by_interactions(df, min_user_interactions, min_item_interactions)

    output_path = Path(output_path)
    df.to_csv(output_path.with_suffix(".csv"), index=False)
    df.to_json(output_path.with_suffix(".jsonl"), orient="records", lines=True)
    logger.info(f"Saved to {output_path.with_suffix('.csv')} and {output_path.with_suffix('.jsonl')}")
    return df


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Preprocess Amazon Reviews dataset")
    parser.add_argument("--input", default=config.RAW_DATA_FILE, help="Input JSONL file")
    parser.add_argument("--output", default=config.PROCESSED_DATA_FILE, help="Output file path")
    parser.add_argument("--min-user-interactions", type=int, default=5)
    parser.add_argument("--min-item-interactions", type=int, default=5)
    parser.add_argument("--rating-threshold", type=float, default=4.0)
    return parser


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    preprocess_amazon_reviews(
        input_path=args.input,
        output_path=args.output,
        min_user_interactions=args.min_user_interactions,
        min_item_interactions=args.min_item_interactions,
        rating_threshold=args.rating_threshold,
    )


if __name__ == "__main__":
    main()
