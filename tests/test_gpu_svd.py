"""The SVD baseline on the device: hvae_svd_spmm / _gram / _chol_inv / _apply against float64 host restatements at
derived bars, CholeskyQR2 against the host's, the reference's golden run (tests/golden/make_svd_fixture.py), the fp32
scores and ranks, and `make baseline-svd` end to end.

u = 2^-53 is fp64's unit roundoff throughout; every bar is first order in u.
"""
import functools
import json
import sys
from unittest import mock

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

import lightgcn_ref as LR
import svd_ref as SR

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
U32 = 2.0 ** -24
WIDTHS = (18, 60, 64)


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.as_tensor(a, device=torch.device("cuda", 0))


def tall(a: np.ndarray) -> torch.Tensor:
    """A host [n, W] matrix as a device [n, 64] one; the columns from W up hold NaN: they may never be read."""
    t = torch.full((a.shape[0], 64), float("nan"), dtype=torch.float64, device=torch.device("cuda", 0))
    t[:, :a.shape[1]] = dev(np.ascontiguousarray(a, dtype=np.float64))
    return t


def normal(shape, seed: int) -> np.ndarray:
    return np.random.Generator(np.random.PCG64(seed)).standard_normal(shape)


@functools.lru_cache(maxsize=None)
def images(name: str):
    from hvae import ops
    m = LR.kernel_graph(name)
    d = torch.device("cuda", 0)
    return ops.csr_from_scipy(m, d), ops.csc_from_scipy(m, d)


# ------------------------------------------------------------------------------------------------------ spmm ----
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("name", list(LR.KERNEL_GRAPHS))
def test_spmm_against_scipy_float64(hip_device, name, W):
    """A X from the CSR and A^T X from the CSC. Bar per element: (deg + 1) u sum |v x|, the first-order bound of a
    deg-term fp64 sum of exact products v x (v is an fp32 count) in any order. Empty rows are exact zeros and the
    columns from W up are zeros whatever X holds there."""
    from hvae import ops
    a = csr_matrix(LR.kernel_graph(name), dtype=np.float64)
    a.sum_duplicates()
    assert (a.data == 2.0).any()
    for image, mat in zip(images(name), (a, csr_matrix(a.T))):
        x = normal((mat.shape[1], W), 40 + W)
        xd = tall(x)
        out = ops.svd_spmm(image, xd, W)
        got = out.cpu().numpy()
        assert got.dtype == np.float64 and got.shape == (mat.shape[0], 64)
        deg = np.diff(mat.indptr)
        bar = (deg[:, None] + 1) * U * (abs(mat) @ np.abs(x))
        err = np.abs(got[:, :W] - mat @ x)
        print(f"{name} {mat.shape} W={W}: max err/bar {np.max(err / np.maximum(bar, 1e-300)):.3f}, max deg {deg.max()}")
        assert (err <= bar).all()
        assert (deg == 0).any() and (got[deg == 0] == 0).all() and (got[:, W:] == 0).all()
        dirty = torch.full_like(out, float("nan"))
        assert ops.svd_spmm(image, xd, W, out=dirty) is dirty and torch.equal(out, dirty)
        assert torch.equal(out, ops.svd_spmm(image, xd, W))


def test_spmm_refuses_aliasing_and_bad_arguments(hip_device):
    from hvae import ops
    csr, csc = images("37x23")
    x = tall(normal((23, 18), 1))
    sq = tall(normal((37, 18), 2))
    with pytest.raises(ValueError, match="alias"):
        ops.svd_spmm(csr, x, 18, out=x)
    both = torch.zeros(50, 64, dtype=torch.float64, device=x.device)   # X and out overlap in rows 13..22
    with pytest.raises(ValueError, match="alias"):
        ops.svd_spmm(csr, both[:23], 18, out=both[13:50])
    with pytest.raises(ValueError, match=r"\[23, 64\]"):
        ops.svd_spmm(csr, sq, 18)      # X must have one row per column of the image
    with pytest.raises(ValueError, match=r"\[37, 64\]"):
        ops.svd_spmm(csc, x, 18)
    for W in (0, 65):
        with pytest.raises(ValueError, match="1 to 64"):
            ops.svd_spmm(csr, x, W)
    with pytest.raises(ValueError, match="float64"):
        ops.svd_spmm(csr, x.float(), 18)
    with pytest.raises(ValueError, match="leading dimension 64"):
        ops.svd_spmm(csr, x[:, :32].contiguous(), 18)


# ------------------------------------------------------------------------------------------------------ gram ----
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2100])
def test_gram_against_float64(hip_device, n):
    """Bar per entry: (n + 2) u sum_r |y_ri y_rj| -- an n-term sum of fmas in chunks, then a sum over at most n
    partials. Exactly symmetric, zero outside W x W, bitwise repeatable."""
    from hvae import ops
    for W in WIDTHS:
        y = normal((n, W), 50 + n)
        yd = tall(y)
        G = ops.svd_gram(yd, W)
        got = G.cpu().numpy()
        bar = (n + 2) * U * (np.abs(y).T @ np.abs(y))
        err = np.abs(got[:W, :W] - y.T @ y)
        print(f"n={n} W={W}: max err/bar {np.max(err / bar):.3f}")
        assert (err <= bar).all()
        assert np.array_equal(got, got.T) and (got[W:] == 0).all() and (got[:, W:] == 0).all()
        dirty = torch.full_like(G, float("nan"))
        ops.svd_gram(yd, W, dirty)
        assert torch.equal(G, dirty)


# --------------------------------------------------------------------------------------------- orthonormalize ----
def test_chol_inv_inverts_the_factor(hip_device):
    """R^-1 is upper triangular with G R^-1 = R^T to the factorisation's backward error: |R^-T G R^-1 - I| <= a small
    multiple of W u cond; on a well-conditioned G (cond about 10) the bar is 64 W u."""
    from hvae import ops
    for W in WIDTHS:
        y = normal((4 * W, W), 60 + W)
        g = np.zeros((64, 64))
        g[:W, :W] = y.T @ y
        flag = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", 0))
        rinv = ops.svd_chol_inv(dev(g), W, flag).cpu().numpy()
        assert flag.item() == 0
        assert (np.tril(rinv, -1) == 0).all() and (rinv[W:] == 0).all() and (rinv[:, W:] == 0).all()
        assert (rinv.diagonal()[:W] > 0).all()
        want, f = SR.chol_inv(g, W)
        assert f == 0
        r = rinv[:W, :W]
        resid = np.abs(r.T @ g[:W, :W] @ r - np.eye(W)).max()
        print(f"W={W}: |R^-T G R^-1 - I| {resid:.3e}, against the host's R^-1 {np.abs(r - want).max():.3e}")
        assert resid <= 64 * W * U
        np.testing.assert_allclose(r, want, rtol=0, atol=64 * W * U * np.abs(want).max())


@pytest.mark.parametrize("W", (18, 60))
@pytest.mark.parametrize("name", ["300x257", "2100x130"])
def test_orthonormalize_the_sketches(hip_device, name, W):
    """CholeskyQR2 on Y = A Omega: max|Q^T Q - I| at most 16 x what the host restatement reaches on the same input
    (floor W u), Q Q^T Y = Y relatively to the same order, and the in-place apply equal to the out-of-place one."""
    from hvae import ops
    a = LR.kernel_graph(name).astype(np.float64)
    y = a @ SR.sketch(a.shape[1], W)
    q_host, f = SR.cholqr2(y)
    assert f == 0
    host_orth = np.abs(q_host.T @ q_host - np.eye(W)).max()
    bar = max(16 * host_orth, W * U)
    flag = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", 0))
    yd = tall(y)
    # one pass by hand: the in-place apply equals the out-of-place one
    G = ops.svd_gram(yd, W)
    rinv = ops.svd_chol_inv(G, W, flag)
    q1 = ops.svd_apply(yd, W, rinv, W)
    q1_in = ops.svd_apply(yd.clone(), W, rinv, W)
    inplace = yd.clone()
    assert ops.svd_apply(inplace, W, rinv, W, out=inplace) is inplace
    assert torch.equal(q1, inplace) and torch.equal(q1, q1_in) and (q1[:, W:] == 0).all()
    qd = ops.svd_orthonormalize(yd.clone(), W, flag)
    assert flag.item() == 0
    q = qd.cpu().numpy()
    assert (q[:, W:] == 0).all()
    q = q[:, :W]
    orth = np.abs(q.T @ q - np.eye(W)).max()
    back = np.abs(q @ (q.T @ y) - y).max() / np.abs(y).max()
    print(f"{name} W={W}: |Q^T Q - I| {orth:.3e} (host {host_orth:.3e}, bar {bar:.3e}); |Q Q^T Y - Y| / |Y| {back:.3e}")
    assert orth <= bar and back <= bar
    assert torch.equal(qd, ops.svd_orthonormalize(yd.clone(), W, flag))


def test_rank_deficient_sketch_sets_the_flag_and_fit_raises(hip_device):
    from hvae import ops
    import src.ml.svd as svd
    y = SR.rank_deficient_rows()
    assert y.shape == (120, 60) and np.linalg.matrix_rank(y) == 40
    flag = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", 0))
    ops.svd_orthonormalize(tall(y), 60, flag)
    assert flag.item() == 1
    ops.svd_orthonormalize(tall(normal((120, 60), 9)), 60, flag)   # a sound input does not clear it
    assert flag.item() == 1
    with pytest.raises(RuntimeError, match="rank-deficient"):
        svd.SVDRecommender(n_components=50).fit(csr_matrix(y))


# ------------------------------------------------------------------------------------------------------- fit ----
@functools.lru_cache(maxsize=None)
def fitted(name: str, k: int):
    import src.ml.svd as svd
    np.random.seed(21)
    state = LR.state_digest()
    model = svd.SVDRecommender(n_components=k)
    model.fit(SR.case_matrix(name))
    assert LR.state_digest() == state   # the sketch comes from a RandomState of its own
    return model


@pytest.mark.parametrize("name,k", SR.CASES)
def test_fit_follows_the_reference_run(hip_device, name, k):
    """Components, user factors, singular values and the explained-variance sum within the fixture's bars (16 x the
    larger of the reference's own LU-against-QR difference and the restatement's)."""
    model = fitted(name, k)
    fx, meta = SR.fixture(), SR.fixture_meta()
    key = SR.case_key(name, k)
    n_users, n_items = SR.case_matrix(name).shape
    assert model.transposed == (name == "97x150")
    assert model.item_factors.shape == (k, n_items) and model.user_factors.shape == (n_users, k)
    assert model.singular_values_.shape == (k,) and model.explained_variance_ratio_.shape == (k,)
    failed = []
    for a, got in (("components", model.item_factors), ("user_factors", model.user_factors),
                   ("singular_values", model.singular_values_), ("evr_sum", model.explained_variance_ratio_.sum())):
        assert got.dtype == torch.float64 and got.device.type == "cuda"
        err = np.abs(got.cpu().numpy() - fx[f"{key}_{a}"]).max()
        bar = meta["bar"][f"{key}_{a}"]
        print(f"{key}_{a}: max err {err:.3e}, bar {bar:.3e}, noise {meta['noise'][f'{key}_{a}']:.3e}")
        if not err <= bar:
            failed.append(a)
    assert not failed


def test_a_second_fit_is_bitwise_equal(hip_device):
    import src.ml.svd as svd
    for name, k in (("150x97", 50), ("97x150", 8)):
        first = fitted(name, k)
        again = svd.SVDRecommender(n_components=k)
        again.fit(SR.case_matrix(name))
        for a in ("user_factors", "item_factors", "singular_values_", "explained_variance_ratio_"):
            assert torch.equal(getattr(first, a), getattr(again, a))


# ---------------------------------------------------------------------------------------------------- scores ----
@pytest.mark.parametrize("name,k", SR.CASES)
def test_scores_are_fp32_within_the_derived_bar(hip_device, name, k):
    """score_all and predict against the reference's float64 predict: (64 + 5) 2^-24 sum_j |u_j v_j| per element (the
    factors rounded to fp32, the products, a 64-term fp32 sum in any order) plus the float64 bar."""
    model = fitted(name, k)
    fx, meta = SR.fixture(), SR.fixture_meta()
    key = SR.case_key(name, k)
    want = fx[f"{key}_scores"]
    users = np.arange(want.shape[0])
    got = model.score_all(users)
    assert got.dtype == torch.float32 and got.shape == want.shape
    bar = (64 + 5) * U32 * (np.abs(fx[f"{key}_user_factors"]) @ np.abs(fx[f"{key}_components"])) \
        + meta["bar"][f"{key}_scores"]
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    print(f"{key}: max err/bar {np.max(err / bar):.3f}, max err {err.max():.3e}")
    assert (err <= bar).all()
    row = model.predict(3)
    assert row.dtype == np.float32 and row.shape == (want.shape[1],) and (np.abs(row - want[3]) <= bar[3]).all()
    cand = torch.as_tensor(np.tile(np.arange(want.shape[1], dtype=np.int32), (5, 1)), device=got.device)
    sc = model.score_candidates(users[:5], cand)
    assert sc.dtype == torch.float32 and (np.abs(sc.cpu().numpy() - want[:5]) <= bar[:5]).all()


def test_ranks_lie_in_the_reference_brackets(hip_device):
    """99-negative ranks from baseline.evaluate_ranks inside [#{ref > s_t + tol}, #{ref >= s_t - tol}] of the
    reference's stored scores, tol = twice the scores' bar (the test item's and the candidate's score each move by
    one bar); full ranking through hvae_topk with the seen items masked, inside the same brackets; the reference's
    stored rank inside them too; and the brackets are tight: hi - lo <= 1 on at least 90 % of the rows."""
    import src.ml.baseline as b
    name, k = SR.RANKS_CASE
    model = fitted(name, k)
    matrix, key = SR.case_matrix(name), SR.case_key(name, k)
    users, tests = LR.fixture_tests(matrix)
    fx, meta = SR.fixture(), SR.fixture_meta()
    scores = fx[f"{key}_scores"]
    tol = 2 * SR.score_bar32(fx[f"{key}_user_factors"], fx[f"{key}_components"], meta["bar"][f"{key}_scores"])
    state = LR.state_digest()
    ranks = b.evaluate_ranks(model, matrix, users, tests, [5, 10, 20], LR.N_NEG)
    assert LR.state_digest() == state  # fewer than 99 negatives exist: nothing is drawn, as in the reference
    K = 20
    full = b.evaluate_ranks(model, matrix, users, tests, [5, 10, K], None)
    inside = tight = 0
    for u, t, r, f, ref_rank in zip(users, tests, ranks, full, fx["ranks"]):
        lo, hi = SR.ref_bracket(scores[u], SR.candidates(matrix, u, t), t, tol)
        assert lo <= r <= hi and lo <= ref_rank <= hi
        assert lo <= f <= hi if f < K else hi >= K
        inside += f < K
        tight += hi - lo <= 1
    assert 0 < inside < len(users)
    assert tight >= 0.9 * len(users)


# --------------------------------------------------------------------------------------------------- end to end ----
def test_main_writes_the_svd_entry_beside_an_existing_one(hip_device, tmp_path):
    import src.ml.svd as svd
    from gen import write_planted_artifacts
    from src.ml.baseline import _build_input_matrix
    from src.ml.train import load_training_data
    data, _ = write_planted_artifacts(tmp_path, dict(n_users=60, n_items=50, d=4, n_clusters=2))
    full, train_df, val_df, maps = load_training_data(str(data))
    matrix, _ = _build_input_matrix(train_df, val_df, maps["user_to_idx"], maps["item_to_idx"], full.shape)
    assert matrix.shape == (60, 50) and SR.sketch_is_full_rank(matrix, 8)
    out = tmp_path / "models" / "figures" / "baseline_results.json"
    out.parent.mkdir(parents=True)
    pop = {"5": {"recall": 0.1, "ndcg": 0.1, "hit_ratio": 0.1}, "training_time_seconds": 0.01}
    out.write_text(json.dumps({"Popularity": pop}))
    np.random.seed(0)
    with mock.patch.object(sys, "argv", ["svd", "--data", str(data), "--n-components", "8", "--n-negatives", "20",
                                         "--k-values", "5", "10"]):
        svd.main()
    got = json.loads(out.read_text())
    assert list(got) == ["Popularity", "SVD"] and got["Popularity"] == pop
    assert list(got["SVD"]) == ["5", "10", "training_time_seconds"]
    for k in ("5", "10"):
        assert set(got["SVD"][k]) == {"recall", "ndcg", "hit_ratio"}
        assert all(0.0 <= v <= 1.0 for v in got["SVD"][k].values())
    assert got["SVD"]["10"]["hit_ratio"] >= got["SVD"]["5"]["hit_ratio"]
