"""Writes tests/golden/preprocess_raw.jsonl.gz, preprocess.npz and preprocess_meta.json: a small raw review file and
what the reference's own src/preprocessing/cleaning.py and src/preprocessing/dataset.py make of it.

Run in the build container (where the reference checkout exists; a few seconds):
    python tests/golden/make_preprocess_fixture.py

The raw file (seeded; about 300 users x 400 items, about 4,000 lines, short texts) holds: a malformed line, null
and missing fields, a non-numeric rating, ratings on both sides of 4, repeated (user, item) pairs -- one of them
three times with ratings 5, 2, 4 --, timestamp ties inside a user, non-ASCII ids, and a planted chain of users and
items that only the second and third rounds of the k-core filter remove. The reference then runs
preprocess_amazon_reviews and, after np.random.seed(7), build_recommendation_dataset on the cleaned .jsonl (as its
Makefile does). Stored, all of it data:
  kept_lines      1-based raw line numbers of the cleaned frame's rows
  binary_rating   of the cleaned frame; item_text, users, items: newline-joined UTF-8 (uint8)
  indptr / indices / data   interaction_matrix.pkl
  train / val / test        the splits as row ids into the cleaned frame, in file order (train: the positives)
  neg_users / neg_ptr / neg_items   the appended negatives: user codes in order, offsets, item codes
  meta: the stats, the filter's iteration count, numpy's MT19937 position (and first key words) afterwards.
The generator asserts that the filter ran 3 or more removing rounds and that every user has at least as many
candidate items as draws, so the reference never took its replace=True path.
"""
import gzip
import json
import logging
import pickle
import sys
import tempfile
from pathlib import Path

import numpy as np
import pandas as pd

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

from make_golden import import_reference  # noqa: E402

N_USERS, N_ITEMS, SEED = 300, 400, 7
WORDS = "toy game fun great kids puzzle wooden train set love super little red blue box card dice ok bad broke".split()
SPECIAL_USERS = {3: "Ünï003", 17: "用户017", 41: "Zoë_041", 99: "uéser99"}
SPECIAL_ITEMS = {5: "B00Ä005", 77: "商品077", 123: "Bß0123"}


def user_id(u: int) -> str:
    return SPECIAL_USERS.get(u, f"U{u:04d}")


def item_id(i: int) -> str:
    return SPECIAL_ITEMS.get(i, f"B{i:05d}")


def raw_records():
    rng = np.random.default_rng(SEED)
    text = lambda k: " ".join(rng.choice(WORDS, size=k))  # noqa: E731
    recs = []

    def add(u, i, rating, ts, **over):
        r = {"user_id": user_id(u) if isinstance(u, int) else u, "asin": item_id(i) if isinstance(i, int) else i,
             "rating": rating, "title": text(2), "text": text(int(rng.integers(2, 5))), "timestamp": int(ts)}
        r.update(over)
        recs.append(r)

    t0 = 1_500_000_000_000
    # background: users 0 .. 279 over items 0 .. 379, item popularity skewed, 6 .. 22 interactions a user (30 for
    # user 0, the largest)
    pop = 1.0 / (np.arange(380) + 12.0)
    pop /= pop.sum()
    for u in range(280):
        k = int(rng.integers(6, 23)) if u else 30
        for i in rng.choice(380, size=k, replace=False, p=pop):
            add(u, int(i), float(rng.integers(1, 6)), t0 + int(rng.integers(0, 10**9)))
    # the planted chain (min_user = min_item = 5): user 280 has 4 rows and goes in round 1, which takes item 380
    # (5 rows, one of them user 280's) with it; user 281 (5 rows, one on item 380) then goes in round 2 and takes
    # item 381; user 282 goes in round 3 and takes item 382. Their other raters are heavy users, their other items
    # popular ones.
    heavy = list(range(1, 40))
    for step, (u, i) in enumerate([(280, 380), (281, 381), (282, 382)]):
        n_own = 4 if step == 0 else 5
        prev_item = 379 + step  # 380 for user 281, 381 for user 282
        own = [i] + ([prev_item] if step else []) + [0, 1, 2, 3][: n_own - 1 - (1 if step else 0)]
        for it in own:
            add(u, it, 5.0, t0 + step * 1000 + it)
        # the item ends with 5 rows: its own user's, the next chain user's (items 380 and 381), the rest heavy users'
        for v in heavy[step * 4: step * 4 + (4 if step == 2 else 3)]:
            add(v, i, 4.0, t0 + 5 * 10**8 + v)
    # repeated pairs: user 0 x item 0 three times with ratings on both sides, user 1 x item 1 twice, below 4 both
    for rating, dt in ((5.0, 11), (2.0, 12), (4.0, 13)):
        add(0, 0, rating, t0 + 2 * 10**9 + dt)
    add(1, 1, 1.0, t0 + 2 * 10**9)
    add(1, 1, 3.0, t0 + 2 * 10**9 + 1)
    # timestamp ties inside a user, among them the user's latest rows
    for it in (10, 11, 12):
        add(2, it, 5.0, t0 + 3 * 10**9)
    add(4, 10, 3.0, t0 + 3 * 10**9)
    add(4, 11, 4.0, t0 + 3 * 10**9)
    order = rng.permutation(len(recs))
    recs = [recs[j] for j in order]
    lines = [json.dumps(r, ensure_ascii=False) for r in recs]
    # the odd lines, spread over the file
    odd = [
        '{"user_id": "U0005", "asin": "B00001", "rating": 5.0, "title": "broken", "text": ',  # malformed
        json.dumps({"user_id": None, "asin": item_id(1), "rating": 5.0, "title": "a", "text": "b", "timestamp": t0}),
        json.dumps({"user_id": user_id(6), "rating": 4.0, "title": "no asin", "text": "b", "timestamp": t0}),
        json.dumps({"user_id": user_id(6), "asin": item_id(2), "rating": None, "title": "a", "text": "b",
                    "timestamp": t0}),
        json.dumps({"user_id": user_id(7), "asin": item_id(2), "rating": "five", "title": "a", "text": "b",
                    "timestamp": t0}),
        json.dumps({"user_id": user_id(7), "asin": item_id(3), "rating": "4.0", "title": None,
                    "text": "  spaced   out\ttext \n here ", "timestamp": t0 + 7}),
        json.dumps({"user_id": user_id(8), "asin": item_id(3), "rating": 3.5, "title": "no text field",
                    "timestamp": t0 + 8}),
        "not json at all",
    ]
    for k, line in enumerate(odd):
        lines.insert(97 + 411 * k, line)
    return lines


class _Capture(logging.Handler):
    def __init__(self):
        super().__init__()
        self.messages = []

    def emit(self, record):
        self.messages.append(record.getMessage())


def main() -> None:
    lines = raw_records()
    gz_path = HERE / "preprocess_raw.jsonl.gz"  # the raw file is committed gzipped (mtime 0: the same bytes each run)
    gz_path.write_bytes(gzip.compress(("\n".join(lines) + "\n").encode("utf-8"), 9, mtime=0))

    import_reference()
    import src.preprocessing.cleaning as cleaning
    import src.preprocessing.dataset as dataset

    cap = _Capture()
    cleaning.logger.addHandler(cap)
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        raw_path = tmp / "preprocess_raw.jsonl"
        raw_path.write_bytes(gzip.decompress(gz_path.read_bytes()))
        cleaned = cleaning.preprocess_amazon_reviews(raw_path, tmp / "cleaned_reviews.jsonl")
        converged = [m for m in cap.messages if m.startswith("Converged after")]
        assert converged, "the reference's filter did not converge within its 10 iterations"
        iterations = int(converged[0].split()[2])
        assert iterations - 1 >= 3, f"the filter removed records in {iterations - 1} rounds only"

        # the cleaned frame's rows as raw line numbers: the frame keeps the raw frame's index, which counts the
        # parsed lines
        parsed = []
        for n, line in enumerate(lines):
            try:
                json.loads(line)
                parsed.append(n + 1)
            except json.JSONDecodeError:
                pass
        kept_lines = np.asarray(parsed)[cleaned.index.to_numpy()]

        # the reference's dataset step on the cleaned .jsonl, with the row id carried as one more column
        frame = pd.read_json(tmp / "cleaned_reviews.jsonl", lines=True)
        assert len(frame) == len(cleaned)
        frame["row_id"] = np.arange(len(frame))
        frame.to_json(tmp / "with_rows.jsonl", orient="records", lines=True)
        np.random.seed(SEED)
        dataset.build_recommendation_dataset(tmp / "with_rows.jsonl", tmp / "out")
        state = np.random.get_state(legacy=True)

        with open(tmp / "out" / "interaction_matrix.pkl", "rb") as f:
            matrix = pickle.load(f)
        with open(tmp / "out" / "mappings.pkl", "rb") as f:
            mappings = pickle.load(f)
        with open(tmp / "out" / "dataset_stats.pkl", "rb") as f:
            stats = pickle.load(f)
        train = pd.read_csv(tmp / "out" / "train.csv")
        val = pd.read_csv(tmp / "out" / "val.csv")
        test = pd.read_csv(tmp / "out" / "test.csv")

    users = [mappings["idx_to_user"][i] for i in range(len(mappings["idx_to_user"]))]
    items = [mappings["idx_to_item"][i] for i in range(len(mappings["idx_to_item"]))]
    assert all(mappings["user_to_idx"][u] == i for i, u in enumerate(users))
    matrix = matrix.tocsr()
    assert matrix.has_canonical_format and matrix.dtype == np.float32
    assert (matrix.data == 0).any(), "no explicit zero is stored"

    pos = train["row_id"].notna().to_numpy()
    n_pos = int(pos.sum())
    assert pos[:n_pos].all() and not pos[n_pos:].any()
    neg = train.iloc[n_pos:]
    assert (neg["binary_rating"] == 0).all() and (neg["rating"] == 0).all()
    neg_u = neg["user_id"].map(mappings["user_to_idx"]).to_numpy()
    neg_i = neg["asin"].map(mappings["item_to_idx"]).to_numpy()
    change = np.flatnonzero(np.r_[True, neg_u[1:] != neg_u[:-1]])
    neg_users = neg_u[change]
    assert (np.diff(neg_users) > 0).all()
    neg_ptr = np.r_[change, len(neg_u)]
    # no user was short of candidates
    train_count = np.bincount(train.iloc[:n_pos]["user_id"].map(mappings["user_to_idx"]).to_numpy(),
                              minlength=len(users))
    candidates = len(items) - np.diff(matrix.indptr)
    assert (candidates >= 4 * train_count).all(), "a user took the reference's replace=True path"
    assert (np.diff(neg_ptr) == 4 * train_count[neg_users]).all()
    seen_three = frame[(frame["user_id"] == user_id(0)) & (frame["asin"] == item_id(0))]
    assert len(seen_three) >= 3 and matrix[mappings["user_to_idx"][user_id(0)], mappings["item_to_idx"][item_id(0)]] >= 2

    join = lambda xs: np.frombuffer("\n".join(xs).encode("utf-8"), dtype=np.uint8)  # noqa: E731
    assert not any("\n" in t for t in cleaned["item_text"])
    np.savez_compressed(
        HERE / "preprocess.npz",
        kept_lines=kept_lines.astype(np.int32),
        binary_rating=cleaned["binary_rating"].to_numpy().astype(np.int8),
        item_text=join(list(cleaned["item_text"])), users=join(users), items=join(items),
        indptr=matrix.indptr.astype(np.int64), indices=matrix.indices.astype(np.int32),
        data=matrix.data.astype(np.float32),
        train=train["row_id"].to_numpy()[:n_pos].astype(np.int32), val=val["row_id"].to_numpy().astype(np.int32),
        test=test["row_id"].to_numpy().astype(np.int32),
        neg_users=neg_users.astype(np.int32), neg_ptr=neg_ptr.astype(np.int64), neg_items=neg_i.astype(np.int32),
        mt_key_head=np.asarray(state[1][:8], dtype=np.uint32))
    meta = {"pandas": pd.__version__, "numpy": np.__version__, "seed": SEED, "raw_lines": len(lines),
            "cleaned_rows": int(len(cleaned)), "filter_iterations": iterations,
            "stats": {k: (float(v) if isinstance(v, float) else int(v)) for k, v in stats.items()},
            "mt_pos": int(state[2]), "columns": list(cleaned.columns)}
    (HERE / "preprocess_meta.json").write_text(json.dumps(meta, indent=1) + "\n", encoding="utf-8")
    sizes = {p.name: p.stat().st_size for p in (gz_path, HERE / "preprocess.npz", HERE / "preprocess_meta.json")}
    assert sum(sizes.values()) < (HERE / "golden.npz").stat().st_size and max(sizes.values()) < 1 << 20, sizes
    print(json.dumps({"meta": meta, "sizes": sizes}, indent=1))


if __name__ == "__main__":
    main()
