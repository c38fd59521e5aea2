"""`make preprocess` on the device (K23): hvae_prep_encode / kcore / split / csr against numpy, pandas and scipy, the
two command lines end to end against what the reference produced on the raw fixture, and the consumers of the
written directory. Every comparison is for exact equality: the outputs are integers, or fp32 sums of 0 / 1 values."""
import json
import pickle
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import preprocess_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _lines(a) -> list[str]:
    return bytes(a).decode("utf-8").split("\n")


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


# ------------------------------------------------------------------ encode --
def _check_encode(ids, dev, want_W=None):
    from hvae import ops
    words, W = ops.prep_pack_ids(ids)
    if want_W is not None:
        assert W == want_W
    codes, first = ops.prep_encode(torch.from_numpy(words.view(np.int64)).to(dev))
    classes, want_first, want_codes = np.unique(np.array(ids, dtype=object), return_index=True, return_inverse=True)
    assert codes.dtype == torch.int32 and first.dtype == torch.int32
    assert np.array_equal(codes.cpu().numpy(), want_codes)
    assert np.array_equal(first.cpu().numpy(), want_first)  # np.unique's index is the first occurrence too
    assert [ids[r] for r in first.cpu().numpy()] == list(classes)


def _random_ids(rng, n_distinct, lengths, alphabet):
    seen, attempt = {}, 0
    while len(seen) < n_distinct:
        k = int(lengths[attempt % len(lengths)])  # a short length may run out of fresh keys: move on regardless
        attempt += 1
        seen["".join(rng.choice(alphabet, size=k))] = None
    return list(seen)


ASCII = list("ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789abcxyz_")


@pytest.mark.parametrize("case", ["one", "two_equal", "lengths_1_to_32", "last_byte_of_word_4", "word_1_only",
                                  "prefix", "non_ascii", "W1", "W4", "70000"])
def test_encode_matches_numpy_unique(case, hip_device):
    rng = np.random.default_rng(11)
    want_W = None
    if case == "one":
        ids = ["B0001"]
    elif case == "two_equal":
        ids = ["same-key", "same-key"]
    elif case == "lengths_1_to_32":
        distinct = _random_ids(rng, 700, np.arange(1, 33), ASCII[:6])  # a small alphabet: many shared prefixes
        ids = [distinct[j] for j in rng.integers(0, 700, 5000)]
        assert len(set(ids)) == 700 and {len(x) for x in ids} == set(range(1, 33))
        want_W = 4
    elif case == "last_byte_of_word_4":
        ids = ["k" * 31 + c for c in "zayb"] * 3 + ["k" * 31]
        want_W = 4
    elif case == "word_1_only":
        ids = [c + "-the-same-tail-of-24-bytes-xx"[:29] for c in "qdQ0d~"] + ["\x7f" + "-the-same-tail-of-24-bytes-xx"[:29]]
        want_W = 4
    elif case == "prefix":
        ids = ["abc", "abcd", "abcdefgh", "abcdefghi", "abcdefgh", "ab", "abcdefgh" * 2, "abcdefgh" * 2 + "a", ""]
    elif case == "non_ascii":
        ids = ["Ünï003", "用户017", "Zoë_041", "Zoe_041", "zz", "Z", "é", "e", "\U0001f600", "￿", "用户", "用户017"]
    elif case == "W1":
        distinct = _random_ids(rng, 300, np.arange(1, 9), ASCII)
        ids = [distinct[j] for j in rng.integers(0, 300, 3000)]
        want_W = 1
    elif case == "W4":
        distinct = _random_ids(rng, 300, np.array([25, 32, 26, 31]), ASCII[:3])
        ids = [distinct[j] for j in rng.integers(0, 300, 3000)]
        want_W = 4
    else:  # more than one block of the sort and of every kernel
        distinct = _random_ids(rng, 20000, np.arange(3, 15), ASCII[:8])
        ids = [distinct[j] for j in rng.integers(0, 20000, 70000)]
        want_W = 2
    _check_encode(ids, hip_device, want_W)


# ------------------------------------------------------------------- kcore --
def _cascade(rng):
    """Users and items 0 .. 9 are a full 10 x 10 core. User 10 has 4 records, one of them on item 10, which has 5:
    round 1 removes both. User 11 (5 records, one on item 10) and item 11 (5, one of them user 11's) go in round 2,
    user 12 and item 12 in round 3; round 4 removes nothing."""
    pairs = [(u, i) for u in range(10) for i in range(10)]
    pairs += [(10, 0), (10, 1), (10, 2), (10, 10)]
    pairs += [(0, 10), (1, 10), (2, 10)]
    pairs += [(11, 10), (11, 11), (11, 0), (11, 1), (11, 2)]
    pairs += [(3, 11), (4, 11), (5, 11)]
    pairs += [(12, 11), (12, 12), (12, 0), (12, 1), (12, 2)]
    pairs += [(6, 12), (7, 12), (8, 12), (9, 12)]
    pairs = np.array(pairs)[rng.permutation(len(pairs))]
    return pairs[:, 0], pairs[:, 1]


@pytest.mark.parametrize("case", ["cascade", "cascade_cut_at_2", "nothing_removed", "everything_removed",
                                  "min_user_differs", "random_many_blocks"])
def test_kcore_matches_the_restatement(case, hip_device):
    from hvae import ops
    rng = np.random.default_rng(3)
    min_user = min_item = 5
    max_iterations = 10
    u, i = _cascade(rng)
    if case == "cascade_cut_at_2":
        max_iterations = 2
    elif case == "nothing_removed":
        keep = (u < 10) & (i < 10)
        u, i = u[keep], i[keep]
    elif case == "everything_removed":
        min_user = 16  # no user has 16 records
    elif case == "min_user_differs":
        min_user, min_item = 6, 3
    elif case == "random_many_blocks":
        u = rng.zipf(1.3, 120000) % 9000
        i = rng.zipf(1.2, 120000) % 5000
        min_user, min_item = 4, 7
    n_users, n_items = int(u.max()) + 2, int(i.max()) + 3  # trailing codes without a record
    want, want_rounds = R.kcore(u, i, min_user, min_item, max_iterations)
    alive, n_alive, rounds = ops.prep_kcore(_i32(u, hip_device), _i32(i, hip_device), n_users, n_items, min_user,
                                            min_item, max_iterations)
    assert alive.dtype == torch.bool and np.array_equal(alive.cpu().numpy(), want)
    assert n_alive == int(want.sum()) and rounds == want_rounds
    if case == "cascade":
        assert rounds == 3 and n_alive == 100
    elif case == "cascade_cut_at_2":
        assert rounds == 2 and n_alive > 100
    elif case == "nothing_removed":
        assert rounds == 0 and n_alive == len(u)
    elif case == "everything_removed":
        assert rounds == 1 and n_alive == 0
    elif case == "random_many_blocks":
        assert rounds >= 2 and 0 < n_alive < len(u)


# ------------------------------------------------------------------- split --
def _pandas_split(user, ts):
    """leave_one_out_split as the reference writes it, on a frame that carries its row ids."""
    df = pd.DataFrame({"user_id": user, "timestamp": ts, "row": np.arange(len(user))})
    df = df.sort_values(["user_id", "timestamp"]).reset_index(drop=True)
    df["_rank"] = df.groupby("user_id").cumcount(ascending=False) + 1
    df["_count"] = df["user_id"].map(df.groupby("user_id").size())
    test = (df["_rank"] == 1) & (df["_count"] >= 2)
    val = (df["_rank"] == 2) & (df["_count"] >= 3)
    train = ~test & ~val
    return [df["row"].to_numpy()] + [df["row"][m].to_numpy() for m in (train, val, test)]


@pytest.mark.parametrize("case", ["counts_1_2_3", "ties", "negative_timestamps", "nat_last", "nan_last", "one_user",
                                  "ends_absent", "random_many_blocks"])
def test_split_matches_pandas(case, hip_device):
    from hvae import ops
    from src.preprocessing.dataset import timestamp_keys
    rng = np.random.default_rng(5)
    if case == "counts_1_2_3":
        user = np.array([2, 0, 1, 2, 1, 2, 3, 3, 3, 3])
        ts = pd.Series(np.array([30, 5, 9, 10, 8, 20, 4, 3, 2, 1], dtype=np.int64))
    elif case == "ties":
        user = np.array([0, 0, 0, 0, 1, 1, 1, 0, 1, 2, 2])
        ts = pd.Series(np.array([7, 7, 7, 7, 3, 3, 3, 7, 3, 1, 1], dtype=np.int64))
    elif case == "negative_timestamps":
        user = rng.integers(0, 40, 600)
        ts = pd.Series(rng.integers(-2**62, 2**62, 600))
        ts[:6] = [-1, 0, 1, -2**63, 2**63 - 2, -2**63 + 1]
        user[:6] = 7
    elif case == "nat_last":
        user = np.array([0, 0, 0, 0, 1, 1, 1, 2, 2, 3, 3, 3])
        ts = pd.Series(pd.to_datetime(["2021-03-01", None, "1965-01-01", "2021-03-01", None, None, "2000-01-01",
                                       None, "1999-09-09", "1969-12-31", "1970-01-01", None]))
    elif case == "nan_last":
        user = np.array([0, 0, 0, 0, 1, 1, 1, 2, 2])
        ts = pd.Series([1.5, np.nan, -3.0, 1.5, np.nan, 0.0, -0.0, np.inf, np.nan])
    elif case == "one_user":
        user = np.full(3000, 4)
        ts = pd.Series(rng.integers(0, 50, 3000))
    elif case == "ends_absent":
        user = rng.integers(1, 30, 500)
        ts = pd.Series(rng.integers(0, 1000, 500))
    else:
        user = rng.zipf(1.4, 90000) % 7000
        ts = pd.Series(rng.integers(0, 2000, 90000))  # many ties
    n_users = int(user.max()) + 2
    want = _pandas_split(user, ts)
    keys = timestamp_keys(ts)
    ref = R.split(user, keys)  # the yardstick agrees with pandas on the same keys
    got = ops.prep_split(_i32(user, hip_device), torch.from_numpy(keys).to(hip_device), n_users)
    for name, g, w, r in zip(("perm", "train", "val", "test"), got, want, ref):
        assert g.dtype == torch.int32
        assert np.array_equal(g.cpu().numpy(), w), name
        assert np.array_equal(r, w), name
    if case == "counts_1_2_3":
        assert got[1].cpu().tolist() == [1, 4, 3, 9, 8] and got[2].cpu().tolist() == [5, 7] and \
            got[3].cpu().tolist() == [2, 0, 6]


# --------------------------------------------------------------------- csr --
@pytest.mark.parametrize("case", ["small", "random_many_blocks"])
def test_csr_matches_scipy(case, hip_device):
    from hvae import ops
    rng = np.random.default_rng(9)
    if case == "small":
        # rows 0, 3 and 6 empty; (1, 4) three times with 1, 0, 1; (2, 2) a stored zero; (5, 0) twice zero
        u = np.array([1, 2, 1, 4, 1, 5, 2, 5, 4, 1])
        i = np.array([4, 2, 0, 3, 4, 0, 5, 0, 1, 4])
        v = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1, 1], dtype=np.float32)
        n_users, n_items = 7, 6
    else:
        n_users, n_items = 6000, 900
        u = rng.zipf(1.3, 150000) % (n_users - 2) + 1  # first and last rows empty
        i = rng.zipf(1.2, 150000) % n_items
        v = (rng.random(150000) < 0.4).astype(np.float32)
    want = R.csr(u, i, v, n_users, n_items)
    m = ops.prep_csr(_i32(u, hip_device), _i32(i, hip_device), torch.from_numpy(v).to(hip_device), n_users, n_items)
    assert m.row_ptr.dtype == torch.int64 and m.col_idx.dtype == torch.int32 and m.vals.dtype == torch.float32
    assert np.array_equal(m.row_ptr.cpu().numpy(), want.indptr)
    assert np.array_equal(m.col_idx.cpu().numpy(), want.indices)
    assert np.array_equal(m.vals.cpu().numpy(), want.data)
    if case == "small":
        assert want.nnz == 7 and want[1, 4] == 2 and m.vals.cpu().tolist().count(0.0) == 2
        assert m.row_ptr.cpu().tolist() == [0, 0, 2, 4, 4, 6, 7, 7]
    else:
        assert (want.data == 0).any() and (want.data > 2).any()


# -------------------------------------------------------------- end to end --
@pytest.fixture(scope="module")
def produced(tmp_path_factory):
    """Both command lines on the raw fixture: data/cleaned_reviews.{csv,jsonl} and the dataset directory."""
    from src.preprocessing import cleaning, dataset
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    out = tmp_path_factory.mktemp("preprocess")
    state = np.random.get_state()
    try:
        cleaning.main(["--input", str(R.raw_path()), "--output", str(out / "cleaned_reviews.jsonl")])
        dataset.main(["--input", str(out / "cleaned_reviews.jsonl"), "--output", str(out), "--seed", str(R.SEED)])
        mt = np.random.get_state(legacy=True)
    finally:
        np.random.set_state(state)
    return out, mt


def test_end_to_end_cleaned_files(produced):
    out, _ = produced
    arrays, meta = R.load_fixture()
    want, _, _ = R.clean()
    with open(R.raw_path(), encoding="utf-8") as f:
        raw = f.read().split("\n")
    for frame in (pd.read_csv(out / "cleaned_reviews.csv", keep_default_na=False),
                  pd.read_json(out / "cleaned_reviews.jsonl", lines=True, convert_dates=False)):
        assert list(frame.columns) == meta["columns"] and len(frame) == meta["cleaned_rows"]
        for col in ("user_id", "asin", "title", "text"):
            assert list(frame[col]) == list(want[col]), col
        assert np.array_equal(frame["timestamp"].to_numpy(), want["timestamp"].to_numpy())
        assert np.array_equal(frame["rating"].to_numpy(), want["rating"].to_numpy())
        assert list(frame["item_text"]) == _lines(arrays["item_text"])
        assert np.array_equal(frame["binary_rating"].to_numpy(), arrays["binary_rating"])
        for row in (0, len(frame) // 2, len(frame) - 1):  # the rows are the raw file's kept lines, in file order
            rec = json.loads(raw[arrays["kept_lines"][row] - 1])
            assert (rec["user_id"], rec["asin"], rec["timestamp"]) == (
                frame["user_id"][row], frame["asin"][row], frame["timestamp"][row])


def test_end_to_end_dataset_files(produced):
    out, mt = produced
    arrays, meta = R.load_fixture()
    cleaned, _, _ = R.clean()
    users, items = _lines(arrays["users"]), _lines(arrays["items"])
    with open(out / "mappings.pkl", "rb") as f:
        maps = pickle.load(f)
    assert set(maps) == {"user_to_idx", "item_to_idx", "idx_to_user", "idx_to_item"}
    assert maps["user_to_idx"] == {u: k for k, u in enumerate(users)} and maps["idx_to_user"] == dict(enumerate(users))
    assert maps["item_to_idx"] == {i: k for k, i in enumerate(items)} and maps["idx_to_item"] == dict(enumerate(items))
    assert all(type(k) is str and type(v) is int for k, v in maps["user_to_idx"].items())
    assert all(type(k) is int and type(v) is str for k, v in maps["idx_to_item"].items())
    with open(out / "interaction_matrix.pkl", "rb") as f:
        m = pickle.load(f)
    assert isinstance(m, sp.csr_matrix) and m.dtype == np.float32 and m.shape == (len(users), len(items))
    for name, got in (("indptr", m.indptr), ("indices", m.indices), ("data", m.data)):
        assert np.array_equal(got, arrays[name]), name
    cols = ["user_id", "asin", "binary_rating"]
    frames = {name: pd.read_csv(out / f"{name}.csv", keep_default_na=False) for name in ("train", "val", "test")}
    for name, frame in frames.items():
        assert list(frame.columns) == meta["columns"]
        rows = cleaned.iloc[arrays[name]]
        head = frame.iloc[:len(rows)]
        for col in cols:
            assert list(head[col]) == list(rows[col]), (name, col)
        assert list(head["item_text"]) == list(rows["item_text"])
    train = frames["train"]
    neg = train.iloc[len(arrays["train"]):]
    want_users = np.repeat(arrays["neg_users"], np.diff(arrays["neg_ptr"]))
    assert list(neg["user_id"]) == [users[u] for u in want_users]
    assert list(neg["asin"]) == [items[i] for i in arrays["neg_items"]]
    assert (neg["binary_rating"] == 0).all() and (neg["rating"].astype(float) == 0).all()
    assert (neg["timestamp"].astype(str) == "0").all()
    assert (neg["title"] == "").all() and (neg["text"] == "").all() and (neg["item_text"] == "").all()
    assert len(frames["val"]) == len(arrays["val"]) and len(frames["test"]) == len(arrays["test"])
    with open(out / "dataset_stats.pkl", "rb") as f:
        stats = pickle.load(f)
    assert stats == meta["stats"] and list(stats) == list(meta["stats"])
    assert mt[2] == meta["mt_pos"] and np.array_equal(mt[1][:8], arrays["mt_key_head"])


def test_consumers_accept_the_directory(produced, hip_device):
    """hvae_read_interactions (through load_training_csr) and the pickle loads of RecommendationCore.from_artifacts
    take the directory as it is."""
    from hvae import ops
    from hvae.io import load_training_csr
    out, _ = produced
    arrays, _ = R.load_fixture()
    cleaned, _, _ = R.clean()
    shape, train, val, train_users, val_users, maps = load_training_csr(str(out))
    assert shape == (len(_lines(arrays["users"])), len(_lines(arrays["items"])))
    for name, got in (("train", train), ("val", val)):
        rows = cleaned.iloc[arrays[name]]
        rows = rows[rows["binary_rating"] == 1]
        want = R.csr(rows["user_id"].map(maps["user_to_idx"]).to_numpy(), rows["asin"].map(maps["item_to_idx"]).to_numpy(),
                     np.ones(len(rows), np.float32), *shape)
        got = got.tocsr()
        got.sort_indices()
        assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
        assert np.array_equal(got.data, want.data)
    # the file's users in first-appearance order, whatever their ratings
    assert train_users == list(dict.fromkeys(maps["user_to_idx"][u] for u in cleaned.iloc[arrays["train"]]["user_id"]))
    assert val_users == list(dict.fromkeys(maps["user_to_idx"][u] for u in cleaned.iloc[arrays["val"]]["user_id"]))
    # from_artifacts: the two pickles, the three dictionaries it passes on, and the upload its constructor does
    with open(out / "interaction_matrix.pkl", "rb") as f:
        matrix = pickle.load(f)
    with open(out / "mappings.pkl", "rb") as f:
        mappings = pickle.load(f)
    assert all(k in mappings for k in ("user_to_idx", "item_to_idx", "idx_to_item"))
    csr = ops.csr_from_scipy(matrix.tocsr(), hip_device)
    assert csr.nb == matrix.shape[0] and csr.n_items == len(mappings["item_to_idx"])
    assert np.array_equal(csr.row_ptr.cpu().numpy(), arrays["indptr"])
