"""`make preprocess` without a GPU: the yardstick (tests/preprocess_ref.py) against what the reference itself produced
on the raw fixture, the two command lines against the reference's, the id packing and its refusals, the timestamp
keys, and the extended host sampler against numpy itself."""
import re
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "recommendation-system_amd"))
sys.path.insert(0, str(ROOT / "tests"))

import preprocess_ref as R  # noqa: E402


def _lines(a) -> list[str]:
    return bytes(a).decode("utf-8").split("\n")


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture()


@pytest.fixture(scope="module")
def cleaned():
    return R.clean()


@pytest.fixture(scope="module")
def built(cleaned):
    state = np.random.get_state()
    try:
        return R.build(cleaned[0])
    finally:
        np.random.set_state(state)


# ------------------------------------------------------------ the yardstick --
def test_restatement_reproduces_the_cleaning_fixture(fixture, cleaned):
    arrays, meta = fixture
    df, lines, rounds = cleaned
    assert list(df.columns) == meta["columns"] == R.CLEANED_COLUMNS
    assert np.array_equal(lines, arrays["kept_lines"])
    assert np.array_equal(df["binary_rating"].to_numpy(), arrays["binary_rating"])
    assert list(df["item_text"]) == _lines(arrays["item_text"])
    assert rounds + 1 == meta["filter_iterations"] and rounds >= 3
    assert set(df["binary_rating"]) == {0, 1}


def test_restatement_reproduces_the_dataset_fixture(fixture, built):
    arrays, meta = fixture
    assert list(built["users"]) == _lines(arrays["users"])
    assert list(built["items"]) == _lines(arrays["items"])
    assert any(not u.isascii() for u in built["users"]) and any(not i.isascii() for i in built["items"])
    for k in ("indptr", "indices", "data", "train", "val", "test", "neg_users", "neg_ptr", "neg_items"):
        assert np.array_equal(built[k], arrays[k]), k
    assert (arrays["data"] == 0).any() and (arrays["data"] >= 2).any()  # a stored zero and a summed duplicate
    assert built["stats"] == meta["stats"]
    assert built["mt_pos"] == meta["mt_pos"] and np.array_equal(built["mt_key_head"], arrays["mt_key_head"])


def test_restated_kcore_stops_at_max_iterations(cleaned):
    """The same cascade cut short: two rounds keep records that the third removes."""
    import json
    with open(R.raw_path(), encoding="utf-8") as f:
        df = pd.DataFrame([json.loads(x) for x in f if _is_json(x)])
    df = df.dropna(subset=["user_id", "asin"])
    _, u, _ = R.encode(df["user_id"].values)
    _, i, _ = R.encode(df["asin"].values)
    full, rounds = R.kcore(u, i)
    cut, cut_rounds = R.kcore(u, i, max_iterations=2)
    assert rounds >= 3 and cut_rounds == 2 and cut.sum() > full.sum()


# ------------------------------------------------------------ command lines --
def _flags(parser):
    return {a.option_strings[0]: a.default for a in parser._actions if a.option_strings and a.dest != "help"}


def test_cleaning_parser_matches_the_reference():
    from src.config import config
    from src.preprocessing import cleaning
    assert _flags(cleaning.build_parser()) == {
        "--input": config.RAW_DATA_FILE, "--output": config.PROCESSED_DATA_FILE, "--min-user-interactions": 5,
        "--min-item-interactions": 5, "--rating-threshold": 4.0}
    args = cleaning.build_parser().parse_args(["--rating-threshold", "3"])
    assert args.rating_threshold == 3.0 and isinstance(args.rating_threshold, float)


def test_dataset_parser_matches_the_reference_plus_seed():
    from src.config import config
    from src.preprocessing import dataset
    assert _flags(dataset.build_parser()) == {
        "--input": config.PROCESSED_DATA_FILE, "--output": str(config.DATA_DIR / "processed_dataset"),
        "--no-negatives": False, "--n-negatives": 4, "--seed": None}
    args = dataset.build_parser().parse_args(["--no-negatives", "--n-negatives", "2", "--seed", "7"])
    assert args.no_negatives is True and args.n_negatives == 2 and args.seed == 7


def test_public_names():
    from src.preprocessing import cleaning, dataset
    for name in ("load_jsonl", "validate_and_select_fields", "clean_data", "add_derived_fields",
                 "filter_by_interactions", "preprocess_amazon_reviews", "main"):
        assert callable(getattr(cleaning, name))
    for name in ("fit_encoders", "create_interaction_matrix", "leave_one_out_split", "create_negative_samples",
                 "save_dataset"):
        assert callable(getattr(dataset.DatasetBuilder, name))
    assert callable(dataset.build_recommendation_dataset)
    assert "sklearn" not in Path(dataset.__file__).read_text() + Path(cleaning.__file__).read_text()


def test_host_stages_of_cleaning_match_the_fixture(fixture, tmp_path):
    """Everything of cleaning.py before the device filter, on the raw fixture: the rows that survive the host
    stages contain the fixture's rows, with the same item_text and binary_rating."""
    from src.preprocessing import cleaning
    arrays, _ = fixture
    df = cleaning.add_derived_fields(cleaning.clean_data(cleaning.validate_and_select_fields(
        cleaning.load_jsonl(R.raw_path()))))
    parsed = [n + 1 for n, line in enumerate(open(R.raw_path(), encoding="utf-8")) if _is_json(line)]
    line_of = np.asarray(parsed)[df.index.to_numpy()]
    keep = np.isin(line_of, arrays["kept_lines"])
    assert keep.sum() == len(arrays["kept_lines"]) and len(df) > keep.sum()
    assert list(df["item_text"][keep]) == _lines(arrays["item_text"])
    assert np.array_equal(df["binary_rating"].to_numpy()[keep], arrays["binary_rating"])
    assert list(df.columns) == R.CLEANED_COLUMNS
    assert "spaced out text here" in set(df["item_text"])  # null title, whitespace collapsed and stripped
    with pytest.raises(ValueError, match="Missing required fields"):
        cleaning.validate_and_select_fields(pd.DataFrame({"user_id": ["a"], "asin": ["b"]}))


def _is_json(line: str) -> bool:
    import json
    try:
        json.loads(line)
        return True
    except json.JSONDecodeError:
        return False


def test_dataset_input_suffix_is_checked(tmp_path):
    from src.preprocessing import dataset
    with pytest.raises(ValueError, match="CSV or JSONL"):
        dataset.build_recommendation_dataset(tmp_path / "reviews.parquet", tmp_path)


# ------------------------------------------------------------- id packing --
def test_id_packing_round_trips_and_keeps_order():
    from hvae import ops
    ids = ["A", "AB", "a" * 32, "Ünï003", "用户017", "", "B00001", "B0000", "zz" * 8, "é" * 16, "\U0001f600x"]
    words, W = ops.prep_pack_ids(ids)
    assert W == 4 and words.shape == (len(ids), 4) and words.dtype == np.uint64
    assert ops.prep_unpack_ids(words) == ids
    order = sorted(range(len(ids)), key=lambda r: tuple(int(x) for x in words[r]))
    assert [ids[r] for r in order] == sorted(ids)  # word order is Python's code-point order
    w1, W1 = ops.prep_pack_ids(["abc", "abcdefgh"])
    assert W1 == 1 and int(w1[0, 0]) == int.from_bytes(b"abc\0\0\0\0\0", "big")
    assert ops.prep_pack_ids(["abcdefghi"])[1] == 2
    assert ops.prep_pack_ids(np.array(["x", "y"], dtype=object))[0].shape == (2, 1)


@pytest.mark.parametrize("bad,match", [
    (["ok", "b" * 33], r"row 1.*33 bytes"),
    (["ok", "é" * 17], r"row 1.*34 bytes"),
    (["ok", "fine", "nul\x00inside"], r"row 2.*NUL"),
    (["ok", "trailing\x00"], r"row 1.*NUL"),
    (["ok", 17], r"row 1.*not a string"),
    ([None, "ok"], r"row 0.*not a string"),
    (["ok", float("nan")], r"row 1.*not a string"),
    (["ok", b"bytes"], r"row 1.*not a string"),
])
def test_id_refusals_name_the_row(bad, match):
    from hvae import ops
    with pytest.raises(ValueError, match=match):
        ops.prep_pack_ids(np.array(bad, dtype=object), "user_id")


# ------------------------------------------------------------- timestamps --
def test_timestamp_keys_keep_pandas_order():
    from src.preprocessing.dataset import timestamp_keys
    ints = pd.Series([5, -3, 0, 2**62, -2**62, 5], dtype=np.int64)
    assert np.array_equal(timestamp_keys(ints), ints.to_numpy())
    dt = pd.Series(pd.to_datetime(["2020-01-01", None, "1960-05-05", "2020-01-01", "1970-01-01"]))
    fl = pd.Series([1.5, np.nan, -2.0, 0.0, -0.0, np.inf, -np.inf, 1e300, -1e-300, 1.5])
    for col in (dt, fl):
        keys = timestamp_keys(col)
        assert keys.dtype == np.int64
        want = col.to_frame("t").sort_values("t", kind="stable").index.to_numpy()  # NaT / NaN last, ties stable
        assert np.array_equal(np.argsort(keys, kind="stable"), want)
    assert timestamp_keys(fl)[3] == timestamp_keys(fl)[4]  # 0.0 and -0.0 tie
    for bad in (pd.Series(["2020-01-01", "x"]), pd.Series([1.5, 2.5], dtype=np.float32), pd.Series([True, False])):
        with pytest.raises(ValueError, match="timestamp"):
            timestamp_keys(bad)


# ----------------------------------------------------------------- sampler --
def _numpy_rows(X, users, n_draw, tests=None):
    out = []
    for r, (u, n) in enumerate(zip(users, n_draw)):
        mask = np.ones(X.shape[1], dtype=bool)
        mask[list(set(X[u].indices))] = False
        if tests is not None:
            mask[tests[r]] = False
        out.append(np.random.choice(np.arange(X.shape[1])[mask], size=n, replace=False))
    return out


@pytest.mark.parametrize("form", ["simd", "scalar"])
@pytest.mark.parametrize("n_users,n_items,density,seed", [(60, 400, 0.05, 1), (300, 150, 0.1, 2), (20, 3000, 0.01, 3)])
def test_sampler_rows_match_numpy_choice(n_users, n_items, density, seed, form, monkeypatch):
    """Varying draw counts per row (0, 1, everything available, and across the 127-draw width of the tracked-slot
    map), with and without an excluded test item, over more rows than one 256-row chunk: draw for draw numpy's, and
    numpy's global state where numpy leaves it."""
    from hvae import ops
    monkeypatch.setenv("HVAE_NEG_SCALAR", "1" if form == "scalar" else "0")
    rng = np.random.default_rng(seed)
    X = sp.random(n_users, n_items, density=density, format="csr", random_state=seed)
    users = np.arange(n_users)
    avail = n_items - np.diff(X.indptr)
    n_draw = np.minimum(rng.integers(0, 140, n_users), avail)
    n_draw[:4] = [0, 1, avail[2], min(128, avail[3])]
    for tests in (None, rng.integers(0, n_items, n_users)):
        nd = n_draw if tests is None else np.minimum(n_draw, avail - 1)
        np.random.seed(100 + seed)
        np.random.random(211)  # mid-block on entry
        want = _numpy_rows(X, users, nd, tests)
        after_want = np.random.random(4)
        np.random.seed(100 + seed)
        np.random.random(211)
        flat, ptr = ops.negatives_legacy_rows(X.indptr, X.indices, n_items, users, nd, tests)
        after_got = np.random.random(4)
        assert np.array_equal(np.diff(ptr), nd)
        for r, w in enumerate(want):
            assert np.array_equal(flat[ptr[r]:ptr[r + 1]], w), f"row {r}"
        assert np.array_equal(after_got, after_want)


def test_sampler_refuses_the_replace_true_path():
    from hvae import ops
    X = sp.csr_matrix(np.array([[1, 1, 1, 0, 0], [0, 0, 0, 0, 1]], dtype=np.float32))
    np.random.seed(5)
    before = np.random.get_state(legacy=True)
    with pytest.raises(RuntimeError, match="row 0: 2 available items for 3 draws"):
        ops.negatives_legacy_rows(X.indptr, X.indices, 5, [0, 1], [3, 2])
    after = np.random.get_state(legacy=True)
    assert np.array_equal(before[1], after[1]) and before[2] == after[2]


def test_builder_negatives_match_the_fixture_and_refuse_short_users(fixture, cleaned):
    """create_negative_samples is host code: on the fixture's matrix and train split it appends the reference's
    negatives, leaves numpy where the reference did, and refuses a user with fewer candidates than draws."""
    from src.preprocessing.dataset import DatasetBuilder
    arrays, meta = fixture
    df = cleaned[0]
    users, items = _lines(arrays["users"]), _lines(arrays["items"])
    b = DatasetBuilder(device="cpu")
    b.user_to_idx = {u: i for i, u in enumerate(users)}
    b.item_to_idx = {it: i for i, it in enumerate(items)}
    b.idx_to_user = dict(enumerate(users))
    b.idx_to_item = dict(enumerate(items))
    b._items = np.array(items, dtype=object)
    m = sp.csr_matrix((arrays["data"], arrays["indices"], arrays["indptr"]), shape=(len(users), len(items)))
    train = df.take(arrays["train"]).reset_index(drop=True)
    state = np.random.get_state()
    try:
        np.random.seed(R.SEED)
        out = b.create_negative_samples(train, m, 4)
        pos = np.random.get_state(legacy=True)
        assert pos[2] == meta["mt_pos"] and np.array_equal(pos[1][:8], arrays["mt_key_head"])
        with pytest.raises(ValueError, match=r"--n-negatives.*--no-negatives"):
            b.create_negative_samples(train, m, 40)
    finally:
        np.random.set_state(state)
    assert list(out.columns) == list(train.columns) and len(out) == meta["stats"]["train_interactions"]
    assert out.iloc[:len(train)].equals(train)
    neg = out.iloc[len(train):]
    want_users = np.repeat(arrays["neg_users"], np.diff(arrays["neg_ptr"]))
    assert list(neg["user_id"]) == [users[u] for u in want_users]
    assert list(neg["asin"]) == [items[i] for i in arrays["neg_items"]]
    assert (neg["binary_rating"] == 0).all() and (neg["rating"] == 0).all() and (neg["timestamp"] == 0).all()
    assert (neg["title"] == "").all() and (neg["text"] == "").all() and (neg["item_text"] == "").all()


# ------------------------------------------------------------------ header --
def test_header_declares_k23_under_abi_6():
    from hvae import _lib
    h = (ROOT / "include" / "hvae.h").read_text()
    assert "(K23)" in h and re.search(r"#define HVAE_ABI_VERSION 6\b", h) and _lib.ABI_VERSION == 6
    for name in ("hvae_prep_encode", "hvae_prep_kcore", "hvae_prep_split", "hvae_prep_csr", "hvae_negatives_legacy_rows"):
        assert re.search(rf"\bint {name}\(", h), name
        assert name in _lib.SIGNATURES
    for name in ("hvae_prep_encode", "hvae_prep_kcore", "hvae_prep_split", "hvae_prep_csr"):
        assert re.search(rf"\bsize_t {name}_workspace\(", h) and f"{name}_workspace" in _lib.SIGNATURES
    assert hasattr(_lib.lib(), "hvae_prep_csr")
