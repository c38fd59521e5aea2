"""The latent-space projections on the device: hvae_tsne_knn / _perplexity / _forces / _update and the PCA against
the float64 restatement (tests/tsne_ref.py) at derived bars, a short trajectory at a measured bar, the full run
against scikit-learn's recorded KL divergence (tests/golden/make_tsne_fixture.py), bitwise reproducibility, and
`make visualize-training`'s compute end to end.

u = 2^-53 is fp64's unit roundoff throughout; a derived bar is first order in u and covers both sides' rounding (the
restatement sums in numpy's order, the device in its own): an m-term sum in any order is within m u sum |terms| of the
exact one.
"""
import functools
import json

import numpy as np
import pytest
import torch

import tsne_ref as TR

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
TINY = 1e-300
# neighbour cases beyond the fixtures: the smallest served shape (k = n - 1 = 32) and one row past a 256-row tile with
# more columns than a wave's lanes
EXTRA = {"n33": (33, 4, 30.0, 11), "n1025": (1025, 128, 30.0, 12)}


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.as_tensor(a, device=torch.device("cuda", 0))


@functools.lru_cache(maxsize=None)
def case_input(case: str):
    if case in EXTRA:
        n, L, perplexity, seed = EXTRA[case]
        return TR.clustered(n, L, seed), perplexity
    return TR.fixture()[f"{case}_X"], TR.CASES[case][2]


@functools.lru_cache(maxsize=None)
def ref_neighbours(case: str):
    X, perplexity = case_input(case)
    return TR.neighbours(X, TR.neighbour_count(len(X), perplexity))


@functools.lru_cache(maxsize=None)
def dev_neighbours(case: str):
    from hvae import ops
    X, perplexity = case_input(case)
    return ops.tsne_knn(dev(X), perplexity)


@functools.lru_cache(maxsize=None)
def dev_joint(case: str):
    from hvae import ops
    idx, d2 = dev_neighbours(case)
    cond = ops.tsne_perplexity(d2, case_input(case)[1])
    return cond, ops.tsne_joint(idx, cond)


# ------------------------------------------------------------------------------------------------ neighbours ----
@pytest.mark.parametrize("case", ["n33", "dup", "c300", "n1025"])
def test_neighbours_against_the_restatement(hip_device, case):
    """Indices equal exactly; a distance is an L-term sum of squares of once-rounded differences: (L + 3) u d^2."""
    X, perplexity = case_input(case)
    n, L = X.shape
    k = min(n - 1, 91)
    assert k == TR.neighbour_count(n, perplexity)
    idx, d2 = (t.cpu().numpy() for t in dev_neighbours(case))
    want_idx, want_d2 = ref_neighbours(case)
    assert idx.shape == d2.shape == (n, k) and idx.dtype == np.int32 and d2.dtype == np.float64
    assert np.array_equal(idx, want_idx)
    err = np.abs(d2 - want_d2)
    print(f"{case}: max err / bar {np.max(err / np.maximum((L + 3) * U * want_d2, TINY)):.3f}")
    assert (err <= (L + 3) * U * want_d2).all()
    assert (np.diff(d2, axis=1) >= 0).all() and (idx != np.arange(n)[:, None]).all()
    if case == "dup":  # duplicated rows come first, at distance exactly 0, ordered by index
        assert idx[3, :2].tolist() == [7, 70] and idx[7, :2].tolist() == [3, 70] and idx[70, :2].tolist() == [3, 7]
        assert (d2[[3, 7, 70], :2] == 0).all() and (d2[[3, 7, 70], 2] > 0).all()
        assert idx[11, 0] == 192 and idx[192, 0] == 11 and d2[11, 0] == d2[192, 0] == 0
    if case == "n33":
        assert (np.sort(idx, axis=1) == np.array([[j for j in range(33) if j != i] for i in range(33)])).all()


def test_neighbours_read_a_strided_matrix_and_flag_nan_rows(hip_device):
    from hvae import ops
    X, perplexity = case_input("c300")
    wide = torch.full((300, 24), float("nan"), device=hip_device)
    wide[:, :16] = dev(X)
    idx, d2 = ops.tsne_knn(wide[:, :16], perplexity)
    assert torch.equal(idx, dev_neighbours("c300")[0]) and torch.equal(d2, dev_neighbours("c300")[1])
    bad = dev(X).clone()
    bad[5, 2] = float("nan")
    idx, d2 = ops.tsne_knn(bad, perplexity)
    assert (idx[5] == -1).all() and (idx[:5] >= 0).all()
    with pytest.raises(ValueError, match="non-finite"):
        ops.tsne_joint(idx, ops.tsne_perplexity(d2, perplexity))


# --------------------------------------------------------------------------------- perplexity and the joint P ----
@pytest.mark.parametrize("case", list(TR.CASES))
def test_perplexity_search_and_joint_p(hip_device, case):
    """The conditional P from the device's own distances against the restatement's search over the same distances.
    With the same beta path (the fixture keeps every step 1e-9 away from the stopping threshold), p_j = e_j / S with
    e_j = exp(-beta d_j): the argument carries u |beta d_j|, exp about 2 u on either side, S is a k-term sum, the
    division one rounding: |dp_j| <= (2 beta d_j + k + 8) u p_j. The joint P adds two such entries (+ u), divides
    (+ u) by a sum of nnz terms that carry the same relative error each (+ (rel + nnz u))."""
    from hvae import ops
    X, perplexity = case_input(case)
    n = len(X)
    idx, d2 = (t.cpu().numpy() for t in dev_neighbours(case))
    k = d2.shape[1]
    cond_d, P_d = dev_joint(case)
    cond = cond_d.cpu().numpy()
    betas = []
    want = TR.conditional_p(d2, perplexity, betas=betas)
    rel = (2 * np.array(betas)[:, None] * d2 + k + 8) * U
    err = np.abs(cond - want)
    print(f"{case}: cond max err / bar {np.max(err / np.maximum(rel * want, TINY)):.3f}, max rel bar {rel.max():.2e}")
    assert (err <= rel * want + TINY).all()
    # every row's perplexity 2^H is within the search's own tolerance of the target: |H - log perplexity| <= 1e-5 nats
    h = np.log(TR.row_perplexity(cond))
    assert np.abs(cond.sum(axis=1) - 1).max() <= (k + 2) * U and np.abs(h - np.log(perplexity)).max() <= 1e-5 + 1e-9
    # the joint P
    P = P_d.to_scipy()
    dense = P.toarray()
    want_P = TR.joint_p(idx, want)
    assert P.has_sorted_indices and np.array_equal(dense, dense.T) and (np.diff(P.indptr) >= k).all()
    assert np.array_equal(dense != 0, want_P != 0) or case == "dup"
    nnz = P.nnz
    bar = (2 * rel.max() + (nnz + 3) * U) * want_P
    err = np.abs(dense - want_P)
    print(f"{case}: P max err / bar {np.max(err / np.maximum(bar, TINY)):.3f}, nnz {nnz}")
    assert (err <= bar + TINY).all() and abs(P.data.sum() - 1) <= nnz * U
    assert P_d.ptr.dtype == torch.int64 and P_d.col.dtype == torch.int32 and P_d.val.dtype == torch.float64
    # against scikit-learn's own P at the bar measured on the CPU
    fx, meta = TR.fixture(), TR.fixture_meta()
    from scipy.sparse import csr_matrix
    sk = csr_matrix((fx[f"{case}_P_val"], fx[f"{case}_P_col"], fx[f"{case}_P_ptr"]), shape=(n, n)).toarray()
    assert np.abs(dense - sk).max() <= meta["bar"][f"{case}_P"]


# --------------------------------------------------------------------------------- one force evaluation + update ----
def force_case(case: str):
    """(P dense from the device pipeline, TsneP, Y): the fixtures at their recorded embeddings (the duplicated rows of
    "dup" coincide there), n = 1025 at a random embedding with two coincident pairs."""
    _, P_d = dev_joint(case)
    P = P_d.to_scipy().toarray()
    if case in TR.CASES:
        Y = TR.fixture()[f"{case}_Y"].astype(np.float64)
    else:
        Y = np.random.Generator(np.random.PCG64(5)).standard_normal((len(P), 2)) * 3.0
        Y[1000], Y[1024] = Y[3], Y[700]
    return P, P_d, Y


@pytest.mark.parametrize("exaggeration,momentum", [(12.0, 0.5), (1.0, 0.8)])
@pytest.mark.parametrize("case", ["dup", "c300", "n1025"])
def test_forces_and_update_against_the_restatement(hip_device, case, exaggeration, momentum):
    """Per point, with t the terms of a sum and c = 12 roundings in one term (the difference, the squared distance,
    1 + d, the division, the products) on either side:
      attr, rep, z   2 (m + 12) u sum |t|          m = the row's entries, n, n
      Z              2 (n + 1) u Z + sum bar_z
      grad           4 (e bar_attr + bar_rep / Z + |rep| bar_Z / Z^2) + 12 u (e |attr| + |rep| / Z)
      g = grad gains gains bar_grad + u |g|;  update: lr bar_g + 3 u (|m update| + |lr g|);  y: bar_update + u |y|
      |grad|_2       sum |g| bar_g / |g|_2 + (2 n + 4) u |g|_2
      error          2 (sum p (12 u + bar_Z / Z) + (nnz + 3) u sum |t|)
    The gains are discrete: they are equal exactly wherever the sign of update * grad is beyond its bar."""
    from hvae import ops
    P, P_d, Y = force_case(case)
    n = len(Y)
    lr = TR.learning_rate(n)
    rng = np.random.Generator(np.random.PCG64(9))
    gains = rng.choice([0.011, 0.5, 1.0, 2.2], size=(n, 2))
    upd = rng.standard_normal((n, 2)) * 1e-2
    if case == "dup":
        assert np.array_equal(Y[3], Y[7]) and np.array_equal(Y[3], Y[70]) and np.array_equal(Y[11], Y[192])
    want = TR.step(Y, gains, upd, P, exaggeration, momentum, lr)

    yd, y_out = dev(Y), torch.full((n, 2), float("nan"), dtype=torch.float64, device=hip_device)
    attr, rep, z = ops.tsne_forces(yd, P_d)
    gd, ud = dev(gains), dev(upd)
    stats = torch.full((2,), float("nan"), dtype=torch.float64, device=hip_device)
    grad, Z = torch.empty_like(yd), torch.empty(1, dtype=torch.float64, device=hip_device)
    assert ops.tsne_update(attr, rep, z, gd, ud, yd, y_out, exaggeration, momentum, lr, P=P_d, stats=stats,
                           grad_out=grad, z_out=Z) is y_out
    got = {"attr": attr, "rep": rep, "z": z, "grad": grad, "gains": gd, "upd": ud, "Y": y_out}
    got = {k: v.cpu().numpy() for k, v in got.items()}
    got["Z"], (got["error"], got["grad_norm"]) = float(Z.item()), stats.cpu().tolist()
    assert all(np.isfinite(np.asarray(v)).all() for v in got.values())
    assert torch.equal(yd, dev(Y))  # y_in is left alone

    diff = Y[:, None, :] - Y[None, :, :]
    q = 1.0 / (1.0 + (diff ** 2).sum(-1))
    np.fill_diagonal(q, 0.0)
    deg = (P != 0).sum(axis=1)
    bar = {"attr": 2 * (deg[:, None] + 12) * U * ((P * q)[:, :, None] * np.abs(diff)).sum(axis=1),
           "rep": 2 * (n + 12) * U * ((q * q)[:, :, None] * np.abs(diff)).sum(axis=1),
           "z": 2 * (n + 12) * U * q.sum(axis=1)}
    Zw, e = want["Z"], exaggeration
    bar["Z"] = 2 * (n + 1) * U * Zw + bar["z"].sum()
    bar["grad"] = 4 * (e * bar["attr"] + bar["rep"] / Zw + np.abs(want["rep"]) * bar["Z"] / Zw ** 2) \
        + 12 * U * (e * np.abs(want["attr"]) + np.abs(want["rep"]) / Zw)
    g = want["grad"] * want["gains"]
    bar_g = want["gains"] * bar["grad"] + U * np.abs(g)
    bar["upd"] = lr * bar_g + 3 * U * (np.abs(momentum * upd) + np.abs(lr * g))
    bar["Y"] = bar["upd"] + U * np.abs(want["Y"])
    norm = want["grad_norm"]
    bar["grad_norm"] = (np.abs(g) * bar_g).sum() / norm + (2 * n + 4) * U * norm
    p = e * P
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = np.where(p > 0, p * np.log(np.maximum(p, TR.FLT_MIN) / np.maximum(q / Zw, TR.FLT_MIN)), 0.0)
    bar["error"] = 2 * (p.sum() * (12 * U + bar["Z"] / Zw) + ((P != 0).sum() + 3) * U * np.abs(terms).sum())
    for name in ("attr", "rep", "z", "Z", "grad", "upd", "Y", "error", "grad_norm"):
        err = np.abs(np.asarray(got[name]) - np.asarray(want[name]))
        print(f"{case} e={e} {name}: max err {err.max():.3e}, max err / bar "
              f"{np.max(err / np.maximum(bar[name], TINY)):.3f}")
        assert (err <= bar[name]).all(), name
    sure = np.abs(want["grad"]) > bar["grad"]
    assert sure.mean() > 0.99 and np.array_equal(got["gains"][sure], want["gains"][sure])
    assert (got["gains"] >= 0.01).all() and (got["gains"] == 0.01).any() and (got["gains"] > 2.2).any()
    # coincident points: no force between them, q = 1 in z
    if case == "dup":
        assert np.isfinite(got["rep"][[3, 7, 70, 11, 192]]).all() and (got["z"][[3, 7, 70]] >= 2).all()
    # without the statistics the step is the same and the statistics are left alone
    gd2, ud2, y2 = dev(gains), dev(upd), torch.empty_like(yd)
    ops.tsne_update(attr, rep, z, gd2, ud2, yd, y2, exaggeration, momentum, lr)
    assert torch.equal(y2, y_out) and torch.equal(gd2, gd) and torch.equal(ud2, ud)


def test_all_points_coincident_stay_finite(hip_device):
    """n points at one place: q = 1 everywhere, no force, Z = n (n - 1), nothing non-finite."""
    from hvae import ops
    _, P_d, _ = force_case("c300")
    n = 300
    y = torch.full((n, 2), 0.25, dtype=torch.float64, device=hip_device)
    attr, rep, z = ops.tsne_forces(y, P_d)
    assert (attr == 0).all() and (rep == 0).all() and (z == n - 1).all()
    gains, upd, y_out = torch.ones_like(y), torch.zeros_like(y), torch.empty_like(y)
    stats, Z = torch.empty(2, dtype=torch.float64, device=hip_device), torch.empty(1, dtype=torch.float64,
                                                                                   device=hip_device)
    ops.tsne_update(attr, rep, z, gains, upd, y, y_out, 12.0, 0.5, 50.0, P=P_d, stats=stats, z_out=Z)
    assert Z.item() == n * (n - 1) and torch.equal(y_out, y) and torch.isfinite(stats).all()
    assert stats[1].item() == 0 and (gains == 0.8).all()


# -------------------------------------------------------------------------------------------------- trajectory ----
def test_thirty_iterations_follow_the_restatement(hip_device):
    """30 iterations from the PCA init on the 300-point fixture, device pipeline against restatement pipeline. The
    bar is 16 times the restatement's own noise floor (the same 30 iterations with every sum reversed, recorded by
    the fixture generator), relative to max |Y|."""
    import src.ml.visualize as v
    meta = TR.fixture_meta()
    case, iters = meta["trajectory_case"], meta["trajectory_iters"]
    X, perplexity = case_input(case)
    n = len(X)
    proj, _ = v.pca_2d(dev(X))
    state = v.TsneState(v.tsne_init(proj.cpu().numpy()), hip_device)
    _, P_d = dev_joint(case)
    kl, it = v.tsne_descend(state, P_d, 0, iters, 0.5, v.EARLY_EXAGGERATION, v.EXPLORATION_ITER,
                            v.tsne_learning_rate(n))
    idx, d2 = ref_neighbours(case)
    want_state = TR.new_state(TR.tsne_init(TR.pca2(X)[0]))
    want_kl, want_it = TR.descend(want_state, TR.joint_p(idx, TR.conditional_p(d2, perplexity)), 0, iters, 0.5,
                                  TR.EARLY_EXAGGERATION, 250, TR.learning_rate(n))
    assert it == want_it == iters - 1
    err = np.abs(state.y.cpu().numpy() - want_state["Y"]).max() / np.abs(want_state["Y"]).max()
    print(f"trajectory: err {err:.3e}, noise floor {meta['trajectory_noise']:.3e}, bar {meta['trajectory_bar']:.3e}; "
          f"kl {kl!r} vs {want_kl!r}")
    assert err <= meta["trajectory_bar"]
    assert np.isfinite(kl) and kl > 0
    for a, b in (("gains", state.gains), ("upd", state.upd)):
        assert np.isfinite(b.cpu().numpy()).all() and b.shape == want_state[a].shape


# ---------------------------------------------------------------------------------------------------- full run ----
@functools.lru_cache(maxsize=None)
def full_run(case: str):
    import src.ml.visualize as v
    X, perplexity = case_input(case)
    xd = dev(X)
    proj, evr = v.pca_2d(xd)
    P = v.tsne_joint_p(xd, perplexity)
    stages = []
    Y, kl, it = v.tsne_embed(P, v.tsne_init(proj.cpu().numpy()), 1000, on_stage=lambda *a: stages.append(a))
    return P, Y, kl, it, stages


@pytest.mark.parametrize("case", list(TR.CASES))
def test_full_run_lands_at_scikit_learn_s_divergence(hip_device, case):
    """kl_divergence against scikit-learn's recorded run at angle = 0.5. The margin is measured: twice the spread
    among scikit-learn at 0.5, scikit-learn at 0.0 and the float64 restatement's full run (kl_spread)."""
    fx, meta = TR.fixture(), TR.fixture_meta()
    P, Y, kl, it, stages = full_run(case)
    sk = float(fx[f"{case}_kl"][0])
    spread = meta["kl_spread"][case]
    print(f"{case}: kl {kl:.6f}, scikit-learn {fx[f'{case}_kl'].tolist()}, |diff| {abs(kl - sk):.2e}, "
          f"2 x spread {2 * spread:.2e}, n_iter {it}")
    assert stages == [("exaggeration", 0), ("final", 250)]
    assert 250 <= it <= 999 and (it == 999 or (it + 1) % 50 == 0)
    assert Y.shape == (len(fx[f"{case}_X"]), 2) and Y.dtype == np.float64 and np.isfinite(Y).all()
    assert np.abs(Y).max() > 1.0  # the embedding left the 1e-4 init
    assert abs(kl - sk) <= 2 * spread


def test_two_fits_are_bitwise_equal(hip_device):
    import src.ml.visualize as v
    case = "c120"
    X, perplexity = case_input(case)
    P, Y, kl, it, _ = full_run(case)
    xd = dev(X.copy())
    proj, evr = v.pca_2d(xd)
    P2 = v.tsne_joint_p(xd, perplexity)
    Y2, kl2, it2 = v.tsne_embed(P2, v.tsne_init(proj.cpu().numpy()), 1000)
    assert torch.equal(P.ptr, P2.ptr) and torch.equal(P.col, P2.col) and torch.equal(P.val, P2.val)
    assert np.array_equal(Y, Y2) and kl == kl2 and it == it2


# --------------------------------------------------------------------------------------------------------- PCA ----
@pytest.mark.parametrize("case", ["c300", "c120", "dup", "n1025"])
def test_pca_against_the_restatement_and_scikit_learn(hip_device, case):
    """L <= 64 goes through the K19 Gram / apply kernels, L = 128 through torch's fp64 product. Bars: the covariance
    is an n-term sum per entry, dC = 2 (n + 3) u || |Xc|^T |Xc| ||_F / (n - 1), and eigh's own backward error is a
    few L u ||C||; an eigenvector moves by at most that over its gap to the next eigenvalue (dv), a projection by
    |xc_i| dv plus its own L-term sum; an eigenvalue moves by at most dC + 4 L u ||C||."""
    import src.ml.visualize as v
    X, _ = case_input(case)
    n, L = X.shape
    proj_d, evr, comps = v.pca_2d(dev(X), return_components=True)
    proj = proj_d.cpu().numpy()
    want, want_evr, want_comps = TR.pca2(X)
    assert proj.shape == (n, 2) and proj.dtype == np.float64 and proj_d.is_contiguous()
    Xc = X.astype(np.float64) - X.astype(np.float64).mean(axis=0)
    C = Xc.T @ Xc / (n - 1)
    w = np.linalg.eigvalsh(C)[::-1]
    dC = 2 * (n + 3) * U * np.linalg.norm(np.abs(Xc).T @ np.abs(Xc)) / (n - 1) + 4 * L * U * w[0]
    gap = np.array([w[0] - w[1], min(w[0] - w[1], w[1] - w[2])])
    dv = 2 * dC / gap
    bar = np.linalg.norm(Xc, axis=1)[:, None] * dv[None, :] + 2 * (L + 2) * U * (np.abs(Xc) @ np.abs(want_comps.T))
    err = np.abs(proj - want)
    print(f"{case}: projection max err {err.max():.3e}, max err / bar {np.max(err / bar):.3f}; evr {evr.tolist()}")
    assert (err <= bar).all() and np.abs(comps - want_comps).max() <= dv.max()
    # the sign rule of svd_flip(u_based_decision=False): each component's largest-magnitude entry is positive
    big = np.abs(comps).argmax(axis=1)
    assert comps.shape == (2, L) and (comps[np.arange(2), big] > 0).all()
    assert np.abs(comps @ comps.T - np.eye(2)).max() <= 8 * L * U
    # the variance ratios
    assert evr.shape == (2,) and (evr > 0).all() and evr[0] >= evr[1] and evr.sum() <= 1.0
    assert np.abs(evr - want_evr).max() <= 4 * dC / w.sum()
    if case in TR.CASES:  # scikit-learn's golden projection, at the bar measured on the CPU
        fx, meta = TR.fixture(), TR.fixture_meta()
        assert np.abs(proj - fx[f"{case}_pca"]).max() <= meta["bar"][f"{case}_pca"]
        assert np.abs(evr - fx[f"{case}_evr"]).max() <= meta["bar"][f"{case}_evr"]


# -------------------------------------------------------------------------------------------------- end to end ----
def test_latent_projections_and_the_training_figures_end_to_end(hip_device, tmp_path, monkeypatch):
    """Planted artifacts, a tiny model trained for two epochs, then the compute entry point for a sample below and
    above the user count, and visualize_training's files."""
    import pickle
    import src.ml.visualize as v
    from gen import write_planted_artifacts
    from hvae import ops
    from src.ml.evaluate import load_model_from_checkpoint
    from src.ml.train import train_hybrid_vae
    data, emb = write_planted_artifacts(tmp_path, dict(n_users=120, n_items=100, d=64, n_clusters=4))
    out = tmp_path / "models"
    torch.manual_seed(0)
    np.random.seed(0)
    train_hybrid_vae(str(data), str(emb), str(out), latent_dim=16, hidden_dims=[64], batch_size=32, epochs=2,
                     learning_rate=1e-3, beta=0.2, dropout=0.3, device="cuda", patience=5)
    model = load_model_from_checkpoint(str(out / "best_model.pth"), np.load(emb), hip_device).to(hip_device).eval()
    with open(data / "interaction_matrix.pkl", "rb") as f:
        matrix = pickle.load(f).tocsr()
    assert matrix.shape[0] == 120
    for n_samples in (60, 2000):
        indices = v.sample_users(matrix.shape[0], n_samples, seed=3)
        n = min(n_samples, 120)
        assert len(indices) == n and (n_samples < 120 or np.array_equal(indices, np.arange(120)))
        res = v.latent_projections(model, matrix, indices)
        assert isinstance(res, v.LatentProjections)
        assert res.mu.shape == (n, 16) and res.mu.dtype == np.float32
        assert res.pca.shape == res.tsne.shape == (n, 2) and res.explained_variance_ratio.shape == (2,)
        assert np.isfinite(res.tsne).all() and np.isfinite(res.pca).all()
        assert isinstance(res.kl_divergence, float) and res.kl_divergence > 0 and 250 <= res.n_iter <= 999
        csr = ops.csr_from_scipy(matrix, hip_device)
        rows = torch.as_tensor(indices.astype(np.int32), device=hip_device)
        with torch.no_grad():
            want = model.get_user_embedding(ops.Csr(csr.row_ptr, csr.col_idx, csr.vals, csr.n_items, rows=rows))
        assert np.array_equal(res.mu, want.float().cpu().numpy())
    with pytest.raises(ValueError, match="33 <= n <= 16384"):
        v.latent_projections(model, matrix, np.arange(20))
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return
    monkeypatch.setattr(v.config, "RAW_DATA_FILE", "Planted_Set.jsonl", raising=False)
    v.visualize_training(str(out), str(data), str(emb), n_samples=60, seed=3)
    got = sorted(p.name for p in (out / "figures").glob("*.png"))
    assert got == sorted("planted_set_" + name for name in (
        "loss_curves.png", "loss_components.png", "training_summary.png", "latent_space_pca.png",
        "latent_space_tsne.png", "latent_space_combined.png"))
    assert json.loads((out / "training_history.json").read_text())["train_losses"]
