"""Popularity and Item-KNN on the device (csrc/hvae_knn.hip, src/ml/baseline.py) against a scipy float64
restatement and against the reference's own run recorded in tests/golden/baselines.npz.

Bar for every Item-KNN score: |got - ref| <= 2^-23 max(|ref|, 1) -- one fp32 rounding of a double sum of
non-negative terms with a factor 2 of headroom; the 1 covers the diagonal subtraction. Popularity is exact.
Ranks: the reference's own ranks inside score ties depend on numpy's unstable argsort, so the checks are the
project's tie rule (test item after its equals; full ranking by larger item index first) for Popularity, whose
scores are exact, and the bracket [#{ref > s_t + tol}, #{ref >= s_t - tol}] for Item-KNN, tol the score bar."""
import json

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

import baseline_ref as BR

pytestmark = pytest.mark.gpu

# (U users, N items, B batch rows, users of the planted long column, entries set to 2.0)
SHAPES = {
    "37x50": (37, 50, 1, 0, 0),
    "300x257": (300, 257, 70, 290, 25),       # more than one wave per column, duplicate-summed entries
    "2100x1030": (2100, 1030, 130, 1500, 40),  # a column longer than any single pass of a wave or a block
}
N_CAND = 12


def _case(name):
    """A random matrix with an empty user row (0), an empty item column (1), the planted column (2), and a batch
    that holds the empty user and one user twice; candidates with a seen item (column 1 of cand) and the empty
    item column (column 2 of cand). With B = 1 the batch is a single non-empty user: the empty user runs as a
    second one-row batch, and a one-row batch cannot hold a user twice."""
    U, N, B, long_col, twos = SHAPES[name]
    rng = np.random.Generator(np.random.PCG64(U * 1000 + N))
    dense = (rng.random((U, N)) < min(0.15, 6.0 / N + 0.02)).astype(np.float64)
    if long_col:
        dense[rng.choice(U, long_col, replace=False), 2] = 1.0
    dense[0, :] = 0.0
    dense[:, 1] = 0.0
    dense[1, [0, 3, 5]] = 1.0  # user 1 is never empty
    if twos:
        r, c = np.nonzero(dense)
        pick = rng.choice(len(r), twos, replace=False)
        dense[r[pick], c[pick]] = 2.0
    matrix = csr_matrix(dense)
    if B == 1:
        rows = np.array([1], np.int32)
    else:
        rows = rng.integers(0, U, size=B).astype(np.int32)
        rows[0], rows[1], rows[2], rows[B - 1] = 0, 1, 5, 5
    cand = rng.integers(0, N, size=(len(rows), N_CAND)).astype(np.int32)
    cand[:, 2] = 1
    for b, u in enumerate(rows):
        seen = matrix[u].indices
        if len(seen):
            cand[b, 1] = seen[len(seen) // 2]
    return matrix, rows, cand


@pytest.fixture(scope="module")
def cases():
    return {name: _case(name) for name in SHAPES}


@pytest.fixture(scope="module")
def oracles(cases):
    return {(name, zd): BR.knn_oracle(m, rows, zd) for name, (m, rows, _) in cases.items() for zd in (False, True)}


def _device_knn(matrix, dev):
    from hvae import ops
    csr = ops.csr_from_scipy(matrix, dev)
    csc = ops.csc_from_scipy(matrix, dev)
    col_sum, inv_norm = ops.csc_col_stats(csc)
    return csr, csc, col_sum, inv_norm


def _batch(csr, rows, dev):
    from hvae import ops
    return ops.Csr(csr.row_ptr, csr.col_idx, csr.vals, csr.n_items, rows=torch.as_tensor(rows, device=dev))


def _score(csr, csc, inv_norm, rows, cand, zd, dev, T=None):
    from hvae import ops
    x = _batch(csr, rows, dev)
    T = ops.knn_user_weights(x, csc, inv_norm, T)
    sc = ops.knn_score_candidates(x, csc, inv_norm, T, torch.as_tensor(cand, device=dev), zd)
    return sc, ops.knn_scores(x, csc, inv_norm, T, zd), T


def _close(got, ref):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all()
    err = np.abs(got - ref)
    assert (err <= BR.bar(ref)).all(), f"max error {err.max():.3e} at reference {ref.ravel()[err.argmax()]:.6f}"


@pytest.mark.parametrize("zero_diag", [False, True])
@pytest.mark.parametrize("name", list(SHAPES))
def test_knn_kernels_match_the_scipy_restatement(hip_device, cases, oracles, name, zero_diag):
    matrix, rows, cand = cases[name]
    csr, csc, _, inv_norm = _device_knn(matrix, hip_device)
    ref = oracles[(name, zero_diag)]
    sc, full, _ = _score(csr, csc, inv_norm, rows, cand, zero_diag, hip_device)
    assert full.shape == (len(rows), matrix.shape[1]) and sc.shape == cand.shape
    _close(full.cpu().numpy(), ref)
    _close(sc.cpu().numpy(), np.take_along_axis(ref, cand.astype(np.int64), axis=1))
    # both entry points sum in the same order: the same bits for the same (row, item)
    assert torch.equal(sc, full.gather(1, torch.as_tensor(cand, device=hip_device).long()))
    assert (full[:, 1] == 0).all()  # the empty item column
    if len(rows) == 1:  # the empty user as a batch of its own
        e_sc, e_full, _ = _score(csr, csc, inv_norm, np.array([0], np.int32), cand, zero_diag, hip_device)
        assert (e_sc == 0).all() and (e_full == 0).all()
    else:
        assert (full[0] == 0).all()  # the empty user row
        assert torch.equal(full[2], full[len(rows) - 1])  # the user that appears twice
    inv = inv_norm.cpu().numpy()
    sq = np.asarray(matrix.multiply(matrix).sum(axis=0)).ravel()
    assert np.isfinite(inv).all() and (inv[sq == 0] == 0).all()
    np.testing.assert_allclose(inv[sq > 0], 1.0 / np.sqrt(sq[sq > 0]), rtol=4e-16)


@pytest.mark.parametrize("name", list(SHAPES))
def test_popularity_column_sums_are_exact(hip_device, cases, name):
    matrix = cases[name][0]
    _, _, col_sum, _ = _device_knn(matrix, hip_device)
    assert np.array_equal(col_sum.cpu().numpy().astype(np.float64), np.asarray(matrix.sum(axis=0)).ravel())


def test_two_calls_are_bitwise_equal_and_a_stale_workspace_does_not_leak(hip_device, cases):
    matrix, rows, cand = cases["2100x1030"]
    csr, csc, _, inv_norm = _device_knn(matrix, hip_device)
    sc1, full1, T = _score(csr, csc, inv_norm, rows, cand, True, hip_device)
    sc2, full2, _ = _score(csr, csc, inv_norm, rows, cand, True, hip_device, T=T)
    assert torch.equal(sc1, sc2) and torch.equal(full1, full2)
    # a different batch through the same T, then the first again: equal to a fresh workspace
    other = ((rows.astype(np.int64) * 7 + 11) % matrix.shape[0]).astype(np.int32)
    _score(csr, csc, inv_norm, other, cand, True, hip_device, T=T)
    sc3, full3, _ = _score(csr, csc, inv_norm, rows, cand, True, hip_device, T=T)
    assert torch.equal(sc1, sc3) and torch.equal(full1, full3)
    # a smaller batch in a larger, dirty workspace
    sc4, full4, _ = _score(csr, csc, inv_norm, rows[:33], cand[:33], True, hip_device, T=T)
    sc5, full5, _ = _score(csr, csc, inv_norm, rows[:33], cand[:33], True, hip_device)
    assert torch.equal(sc4, sc5) and torch.equal(full4, full5)


def test_argument_errors(hip_device, cases):
    from hvae import ops
    matrix, rows, cand = cases["300x257"]
    csr, csc, _, inv_norm = _device_knn(matrix, hip_device)
    x = _batch(csr, rows, hip_device)
    small = torch.empty(8, dtype=torch.float64, device=hip_device)
    with pytest.raises(RuntimeError, match="T holds"):
        ops.knn_user_weights(x, csc, inv_norm, small)
    assert ops.knn_workspace_bytes(len(rows), matrix.shape[0]) == 8 * len(rows) * matrix.shape[0]
    assert ops.knn_workspace_bytes(0, 10) == 0


# ------------------------------------------------------------------ golden --
@pytest.fixture(scope="module")
def fitted(hip_device):
    """Both models fitted on both fixture configs, once."""
    import src.ml.baseline as b
    out = {}
    for cfg in BR.CONFIGS:
        matrix, users, tests = BR.planted(cfg)
        pop, knn = b.PopularityRecommender(device=hip_device), b.ItemKNNRecommender(k=50, device=hip_device)
        pop.fit(matrix)
        knn.fit(matrix)
        out[cfg] = (matrix, users, tests, pop, knn)
    return out


@pytest.mark.parametrize("cfg", list(BR.CONFIGS))
def test_golden_scores(hip_device, fitted, cfg):
    fx = BR.fixture()
    matrix, users, tests, pop, knn = fitted[cfg]
    assert knn.zero_diag == BR.fixture_meta()["configs"][cfg]["zero_diag"] == (matrix.shape[1] <= 10000)
    assert np.array_equal(pop.predict(int(users[0])), fx[f"{cfg}_pop"])
    assert np.array_equal(pop.score_all(users[:3]).cpu().numpy().astype(np.float64), np.tile(fx[f"{cfg}_pop"], (3, 1)))
    if cfg == "small":
        _close(knn.score_all(users).cpu().numpy(), fx["small_knn"])
        p = knn.predict(int(users[5]))
        assert p.shape == (matrix.shape[1],) and p.dtype == np.float64
        _close(p, fx["small_knn"][5])
    else:
        cand = np.concatenate([BR.candidates(tests, fx["large_neg"]),
                               np.tile(fx["large_items"].astype(np.int64), (len(users), 1))], axis=1)
        got = knn.score_candidates(users, torch.as_tensor(cand.astype(np.int32), device=hip_device))
        _close(got.cpu().numpy(), fx["large_knn"])


@pytest.fixture(scope="module")
def golden_ranks(hip_device, fitted):
    """Per config and model: the 99-negative ranks from the fixture's seed (negatives checked draw for draw)."""
    import src.ml.baseline as b
    from hvae import ops
    fx = BR.fixture()
    out = {}
    for cfg, (matrix, users, tests, pop, knn) in fitted.items():
        for key, model in (("pop", pop), ("knn", knn)):
            np.random.seed(BR.SEED)
            neg, cnt = ops.negatives_legacy(matrix.indptr, matrix.indices, matrix.shape[1], users, tests, BR.N_NEG,
                                            arrays=True)
            assert (cnt == BR.N_NEG).all() and np.array_equal(neg, fx[f"{cfg}_neg"])
            np.random.seed(BR.SEED)
            out[(cfg, key)] = b.evaluate_ranks(model, matrix, users, tests, [5, 10, 20], BR.N_NEG)
    return out


@pytest.mark.parametrize("cfg", list(BR.CONFIGS))
def test_golden_negative_sampling_ranks(golden_ranks, cfg):
    fx = BR.fixture()
    cand = BR.candidates(fx[f"{cfg}_tests"], fx[f"{cfg}_neg"])
    gt, eq = BR.exact_bracket(fx[f"{cfg}_pop"][cand])
    assert np.array_equal(golden_ranks[(cfg, "pop")], gt + eq)
    cs = np.take_along_axis(fx["small_knn"], cand, axis=1) if cfg == "small" else fx["large_knn"][:, :cand.shape[1]]
    lo, hi = BR.tol_bracket(cs)
    rank = golden_ranks[(cfg, "knn")]
    assert ((rank >= lo) & (rank <= hi)).all()


@pytest.mark.parametrize("cfg,key", [("small", "pop"), ("large", "pop"), ("small", "knn")])
def test_golden_full_ranking_position(fitted, cfg, key):
    """Seen items masked, ties to the larger item index first; K = 20, positions past it count as absent."""
    import src.ml.baseline as b
    fx = BR.fixture()
    matrix, users, tests, pop, knn = fitted[cfg]
    K, absent = 20, np.iinfo(np.int32).max
    got = b.evaluate_ranks(pop if key == "pop" else knn, matrix, users, tests, [5, 10, K], None)
    ref = np.tile(fx[f"{cfg}_pop"], (len(users), 1)) if key == "pop" else fx["small_knn"].copy()
    for r, u in enumerate(users):
        ref[r, matrix[u].indices] = -np.inf
    s_t = ref[np.arange(len(users)), tests][:, None]
    assert np.isfinite(s_t).all()  # no test item is a seen one in the planted sets
    idx = np.arange(ref.shape[1])[None, :]
    if key == "pop":
        want = (ref > s_t).sum(1) + ((ref == s_t) & (idx > tests[:, None])).sum(1)
        assert np.array_equal(got, np.where(want < K, want, absent))
        return
    tol = BR.bar(s_t)
    others = idx != tests[:, None]
    lo, hi = ((ref > s_t + tol) & others).sum(1), ((ref >= s_t - tol) & others).sum(1)
    present = got != absent
    assert ((got[present] >= lo[present]) & (got[present] <= hi[present]) & (got[present] < K)).all()
    assert (hi[~present] >= K).all() and present[hi < K].all() and (~present[lo >= K]).all()


def test_run_all_baselines_end_to_end(tmp_path, hip_device, fitted, golden_ranks):
    import src.ml.baseline as b
    from gen import write_planted_artifacts
    from src.ml.evaluate import metrics_from_rank
    data, _ = write_planted_artifacts(tmp_path, BR.CONFIGS["small"])
    matrix, users, tests, _, _ = fitted["small"]
    ks = [5, 10, 20]
    out_path = tmp_path / "models" / "figures" / "baseline_results.json"

    def expect(rank):
        m = metrics_from_rank(rank, ks)
        return {str(k): {n: float(np.mean(m[k][n])) for n in ("recall", "ndcg", "hit_ratio")} for k in ks}

    # each model alone from the fixture's seed: the metrics of the ranks checked above, the stream one pass on
    one_pass = BR.replay_choice_stream(matrix, users, tests, 1)
    for name, key in (("Popularity", "pop"), ("Item-KNN", "knn")):
        np.random.seed(BR.SEED)
        res = b.run_all_baselines(str(data), ks, BR.N_NEG, models=[name])
        assert BR.same_state(np.random.get_state(), one_pass)
        js = json.loads(out_path.read_text())
        assert list(js) == [name] and list(js[name]) == ["5", "10", "20", "training_time_seconds"]
        assert {k: js[name][k] for k in ("5", "10", "20")} == expect(golden_ranks[("small", key)])
        assert res[name][5] == js[name]["5"] and res[name]["training_time_seconds"] == js[name]["training_time_seconds"]
    # both, one after the other on one stream: the second model's draws follow the first's
    np.random.seed(BR.SEED)
    b.run_all_baselines(str(data), ks, BR.N_NEG)
    assert BR.same_state(np.random.get_state(), BR.replay_choice_stream(matrix, users, tests, 2))
    js = json.loads(out_path.read_text())
    assert list(js) == ["Popularity", "Item-KNN"]
    assert {k: js["Popularity"][k] for k in ("5", "10", "20")} == expect(golden_ranks[("small", "pop")])
    np.random.set_state(one_pass)
    knn = fitted["small"][4]
    second = b.evaluate_ranks(knn, matrix, users, tests, ks, BR.N_NEG)
    assert {k: js["Item-KNN"][k] for k in ("5", "10", "20")} == expect(second)
    for name in js:
        assert set(js[name]["5"]) == {"recall", "ndcg", "hit_ratio"} and js[name]["training_time_seconds"] >= 0
    # full ranking through the same entry point
    res = b.run_all_baselines(str(data), ks, None, models=["Item-KNN"])
    rank = b.evaluate_ranks(knn, matrix, users, tests, ks, None)
    assert {str(k): res["Item-KNN"][k] for k in ks} == expect(rank)
