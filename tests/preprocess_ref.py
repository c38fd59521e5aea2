"""A numpy / pandas / scipy restatement of the reference's two preprocessing scripts (src/preprocessing/cleaning.py
and src/preprocessing/dataset.py), written from their source, as the yardstick of the CPU and GPU preprocessing
tests. tests/test_preprocess_cpu.py shows that it reproduces what the reference itself produced on the raw fixture
(tests/golden/preprocess*.{jsonl.gz,npz,json}, written by tests/golden/make_preprocess_fixture.py); the device tests
then hold the kernels and the two modules to it. Nothing here imports the code under test.
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pandas as pd
import scipy.sparse as sp

GOLDEN = Path(__file__).resolve().parent / "golden"
RAW_GZ = GOLDEN / "preprocess_raw.jsonl.gz"  # the raw review file, gzipped
REQUIRED = ["user_id", "asin", "rating", "title", "text", "timestamp"]
CLEANED_COLUMNS = REQUIRED + ["item_text", "binary_rating"]
SEED = 7  # np.random.seed before the fixture's negatives


_unpacked = None


def raw_path() -> Path:
    """The raw fixture unpacked into a temporary directory (once a process, removed at exit), for code that takes
    the path of a .jsonl file."""
    global _unpacked
    if _unpacked is None:
        import atexit
        import gzip
        import shutil
        import tempfile
        d = Path(tempfile.mkdtemp(prefix="preprocess_raw_"))
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        (d / "preprocess_raw.jsonl").write_bytes(gzip.decompress(RAW_GZ.read_bytes()))
        _unpacked = d / "preprocess_raw.jsonl"
    return _unpacked


# ------------------------------------------------------------------ pieces --
def encode(values):
    """LabelEncoder.fit + transform: (classes ascending, codes, first record index of each class)."""
    arr = np.asarray(values, dtype=object)
    classes, first, codes = np.unique(arr, return_index=True, return_inverse=True)
    return classes, codes.astype(np.int64), first.astype(np.int64)


def kcore(ucode, icode, min_user=5, min_item=5, max_iterations=10):
    """filter_by_interactions over codes: (alive mask, rounds that removed a record). A round counts users over the
    live records, drops the records of users below min_user, counts items over the rest, drops the records of items
    below min_item; the loop ends after a round that changed nothing, or after max_iterations rounds."""
    ucode, icode = np.asarray(ucode, dtype=np.int64), np.asarray(icode, dtype=np.int64)
    alive = np.ones(len(ucode), dtype=bool)
    worked = 0
    for _ in range(max_iterations):
        before = int(alive.sum())
        ucnt = np.bincount(ucode[alive], minlength=int(ucode.max(initial=-1)) + 1)
        alive &= ucnt[ucode] >= min_user
        icnt = np.bincount(icode[alive], minlength=int(icode.max(initial=-1)) + 1)
        alive &= icnt[icode] >= min_item
        if int(alive.sum()) == before:
            break
        worked += 1
    return alive, worked


def split(ucode, ts_keys):
    """leave_one_out_split over (user code, int64 timestamp key): (perm, train, val, test) record indices, perm the
    stable order by (user, timestamp), the parts in that order."""
    ucode, ts_keys = np.asarray(ucode, dtype=np.int64), np.asarray(ts_keys, dtype=np.int64)
    perm = np.lexsort((ts_keys, ucode))  # stable: ties keep input order
    u = ucode[perm]
    n = len(u)
    count = np.bincount(u, minlength=int(u.max(initial=-1)) + 1)[u]
    start = np.r_[0, np.flatnonzero(u[1:] != u[:-1]) + 1] if n else np.zeros(0, dtype=np.int64)
    run_start = np.repeat(start, np.diff(np.r_[start, n]))
    rank = count - (np.arange(n) - run_start)  # 1 = the user's last record
    test = (rank == 1) & (count >= 2)
    val = (rank == 2) & (count >= 3)
    train = ~test & ~val
    return perm, perm[train], perm[val], perm[test]


def csr(ucode, icode, vals, n_users, n_items):
    """create_interaction_matrix: scipy's own construction (duplicates summed, columns sorted, explicit zeros kept)."""
    m = sp.csr_matrix((np.asarray(vals), (np.asarray(ucode), np.asarray(icode))), shape=(n_users, n_items),
                      dtype=np.float32)
    m.sum_duplicates()
    m.sort_indices()
    return m


def timestamp_keys(col) -> np.ndarray:
    """The timestamp column as int64 keys in pandas' sort order (NaT / NaN last)."""
    v = np.asarray(col)
    big = np.iinfo(np.int64).max
    if v.dtype.kind == "M":
        k = v.view(np.int64).copy()
        k[np.isnat(v)] = big
        return k
    if v.dtype.kind == "f":
        order = np.argsort(v, kind="stable")  # NaN last
        k = np.empty(len(v), dtype=np.int64)
        ranks = np.r_[0, np.cumsum(v[order][1:] != v[order][:-1])] if len(v) else np.zeros(0, np.int64)
        k[order] = ranks
        k[np.isnan(v)] = big
        return k
    return v.astype(np.int64)


def negatives(train_ucode, matrix, n_per_positive=4):
    """create_negative_samples' draws, as the reference writes them: users of the train frame ascending, each
    np.random.choice(candidates, n, replace=False) from numpy's global generator. -> (users, list of draws)."""
    n_items = matrix.shape[1]
    all_items = np.arange(n_items)
    users = np.unique(np.asarray(train_ucode))
    counts = np.bincount(np.asarray(train_ucode, dtype=np.int64), minlength=matrix.shape[0])
    kept, out = [], []
    for u in users:
        n_neg = int(counts[u]) * n_per_positive
        mask = np.ones(n_items, dtype=bool)
        mask[list(set(matrix[u].indices))] = False
        candidates = all_items[mask]
        if len(candidates) == 0:
            continue
        assert len(candidates) >= n_neg, "the replace=True path is outside the restatement"
        kept.append(int(u))
        out.append(np.random.choice(candidates, size=n_neg, replace=False))
    return kept, out


# ---------------------------------------------------------------- cleaning --
def clean(raw=None, min_user=5, min_item=5, rating_threshold=4.0, max_iterations=10):
    """preprocess_amazon_reviews up to the frame it writes: (cleaned frame with the eight columns, the 1-based raw
    line numbers of its rows, rounds of the filter that removed a record)."""
    records, lines = [], []
    with open(raw or raw_path(), encoding="utf-8") as f:
        for i, line in enumerate(f):
            try:
                records.append(json.loads(line))
                lines.append(i + 1)
            except json.JSONDecodeError:
                pass
    df = pd.DataFrame(records)
    missing = set(REQUIRED) - set(df.columns)
    if missing:
        raise ValueError(f"Missing required fields: {missing}")
    df = df[REQUIRED].copy()
    df["_line"] = lines
    df = df.dropna(subset=["user_id", "asin", "rating"]).copy()
    df["title"] = df["title"].fillna("")
    df["text"] = df["text"].fillna("")
    text = (df["title"].astype(str) + " " + df["text"].astype(str)).str.strip()
    df["item_text"] = text.str.replace(r"\s+", " ", regex=True)
    df["rating"] = pd.to_numeric(df["rating"], errors="coerce")
    df = df.dropna(subset=["rating"]).copy()
    df["binary_rating"] = (df["rating"] >= rating_threshold).astype(int)
    _, ucode, _ = encode(df["user_id"].values)
    _, icode, _ = encode(df["asin"].values)
    alive, rounds = kcore(ucode, icode, min_user, min_item, max_iterations)
    df = df[alive]
    return df[CLEANED_COLUMNS].reset_index(drop=True), df["_line"].to_numpy(), rounds


# ----------------------------------------------------------------- dataset --
def build(df, add_negatives=True, n_per_positive=4, seed=SEED):
    """build_recommendation_dataset over a cleaned frame, as arrays: the class lists, the matrix, the three splits as
    row ids into df, the negatives per user, the stats and numpy's MT19937 position afterwards."""
    users, ucode, _ = encode(df["user_id"].values)
    items, icode, _ = encode(df["asin"].values)
    m = csr(ucode, icode, df["binary_rating"].to_numpy(), len(users), len(items))
    _, train, val, test = split(ucode, timestamp_keys(df["timestamp"].to_numpy()))
    out = {"users": users, "items": items, "indptr": m.indptr.astype(np.int64), "indices": m.indices.astype(np.int32),
           "data": m.data.astype(np.float32), "train": train, "val": val, "test": test}
    if add_negatives and len(train):
        if seed is not None:
            np.random.seed(seed)
        neg_users, draws = negatives(ucode[train], m, n_per_positive)
        out["neg_users"] = np.asarray(neg_users, dtype=np.int64)
        out["neg_ptr"] = np.r_[0, np.cumsum([len(d) for d in draws])].astype(np.int64)
        out["neg_items"] = np.concatenate(draws).astype(np.int64) if draws else np.zeros(0, np.int64)
        out["mt_pos"] = int(np.random.get_state(legacy=True)[2])
        out["mt_key_head"] = np.asarray(np.random.get_state(legacy=True)[1][:8], dtype=np.uint32)
    n_train = len(train) + (len(out["neg_items"]) if "neg_items" in out else 0)
    out["stats"] = {"n_users": len(users), "n_items": len(items), "train_interactions": int(n_train),
                    "val_interactions": int(len(val)), "test_interactions": int(len(test)),
                    "matrix_density": m.nnz / (len(users) * len(items))}
    return out


def load_fixture():
    """The reference's observed results on the raw fixture: (arrays of preprocess.npz, preprocess_meta.json)."""
    arrays = dict(np.load(GOLDEN / "preprocess.npz", allow_pickle=False))
    meta = json.loads((GOLDEN / "preprocess_meta.json").read_text(encoding="utf-8"))
    return arrays, meta
