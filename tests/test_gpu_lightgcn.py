"""The LightGCN baseline on the device: hvae_lgcn_norm / _propagate / _bpr against float64 restatements at derived
bars, one full train step against torch autograd, the reference's golden trajectory, and `make baseline-lightgcn`
end to end.

u = 2^-24 is fp32's unit roundoff throughout; every bar is first order in u.
"""
import functools
import json
import sys
from unittest import mock

import numpy as np
import pytest
import torch

import lightgcn_ref as LR

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
DIMS = (64, 128)


@functools.lru_cache(maxsize=None)
def device_graph(name: str):
    from hvae import ops
    return ops.lgcn_graph_from_scipy(LR.kernel_graph(name), torch.device("cuda", 0))


@functools.lru_cache(maxsize=None)
def host_graph(name: str):
    return LR.adjacency(LR.kernel_graph(name))  # (A with fp32-rounded weights, deg^-1/2, deg), float64


def table(n: int, d: int, seed: int, std: float = 0.1) -> np.ndarray:
    return (std * np.random.Generator(np.random.PCG64(seed)).standard_normal((n, d))).astype(np.float32)


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.as_tensor(a, device=torch.device("cuda", 0))


def chain_with_bound(a, deg, e, de, n_layers: int):
    """(the float64 Horner chain of e, the bound of the device chain's error) where de bounds the error e itself
    carries. One link computes y = alpha (add + A x) as an fp32 sum of deg + 1 terms in some order with weights
    rounded once, then one product: |dy| <= alpha (|d add| + A |dx|) + (deg + 3) u alpha (|add| + A |x|)."""
    x, bx = e, de
    for k in range(n_layers):
        alpha = 1.0 / (n_layers + 1) if k == n_layers - 1 else 1.0
        x, bx = (alpha * (e + a @ x),
                 alpha * (de + a @ bx) + (deg[:, None] + 3) * U * alpha * (np.abs(e) + a @ np.abs(x)))
    return x, bx


# ------------------------------------------------------------------------------------------------ the graphs ----
def test_kernel_graphs_have_the_shapes_the_kernels_branch_on():
    for name in LR.KERNEL_GRAPHS:
        s = LR.structure(LR.kernel_graph(name))
        cols, rows = np.diff(s.tocsc().indptr), np.diff(s.indptr)
        assert (cols == 0).any() and (rows == 0).any() and (LR.kernel_graph(name).data == 2.0).any()
        if name == "37x23":
            assert cols.max() < 64 and rows.max() < 64  # every row shorter than a wave
        elif name == "300x257":
            assert cols.max() == 290 and rows.max() < 64
        else:
            assert cols.max() == 1500 and rows.max() == 120


@pytest.mark.parametrize("name", list(LR.KERNEL_GRAPHS))
def test_degree_scales(hip_device, name):
    g = device_graph(name)
    _, _, deg = host_graph(name)
    got = g.scale.cpu().numpy()
    assert got.dtype == np.float64
    iso = deg == 0
    assert iso.any() and (got[iso] == 0).all()
    np.testing.assert_allclose(got[~iso], np.power(deg[~iso], -0.5), rtol=4e-16, atol=0)


# ----------------------------------------------------------------------------------------------- propagation ----
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("name", list(LR.KERNEL_GRAPHS))
def test_propagate_against_scipy_float64(hip_device, name, d):
    """Bar per element: (deg + 3) u alpha (|add| + sum |w x|), the first-order bound of an fp32 sum of deg + 1 terms
    in any order with weights rounded once and one final product. Isolated nodes return exactly alpha * add."""
    from hvae import ops
    g = device_graph(name)
    a, _, deg = host_graph(name)
    x, add = table(g.n_nodes, d, 10), table(g.n_nodes, d, 11)
    xd, addd = dev(x), dev(add)
    iso = deg == 0
    for with_add in (False, True):
        for alpha in (1.0, 0.25):
            out = ops.lgcn_propagate(g, xd, addd if with_add else None, alpha=alpha)
            got = out.cpu().numpy()
            ref, absum = LR.propagate_oracle(a, x, add if with_add else None, alpha)
            bar = (deg[:, None] + 3) * U * absum
            err = np.abs(got - ref)
            print(f"{name} d={d} add={with_add} alpha={alpha}: max err/bar {np.max(err / np.maximum(bar, 1e-300)):.3f}")
            assert (err <= bar).all()
            want_iso = np.float32(alpha) * add[iso] if with_add else np.zeros_like(add[iso])
            assert np.array_equal(got[iso], want_iso)
            again = ops.lgcn_propagate(g, xd, addd if with_add else None, alpha=alpha)
            assert torch.equal(out, again)
            dirty = torch.full_like(out, float("nan"))
            ops.lgcn_propagate(g, xd, addd if with_add else None, out=dirty, alpha=alpha)
            assert torch.equal(out, dirty)


def test_propagate_refuses_aliasing_and_unserved_dims(hip_device):
    from hvae import ops
    g = device_graph("37x23")
    x = dev(table(g.n_nodes, 64, 1))
    with pytest.raises(ValueError, match="alias"):
        ops.lgcn_propagate(g, x, out=x)
    with pytest.raises(ValueError, match="64 and 128"):
        ops.lgcn_propagate(g, dev(table(g.n_nodes, 96, 1)))
    with pytest.raises(ValueError, match="1 to 8"):
        ops.lgcn_chain(g, x, 9, torch.empty_like(x), torch.empty_like(x), torch.empty_like(x))


@pytest.mark.parametrize("n_layers", [1, 3, 8])
def test_chain_is_the_layer_mean(hip_device, n_layers):
    """The Horner chain equals the reference's mean of E, A E, ..., A^L E within the composed link bars."""
    from hvae import ops
    g = device_graph("300x257")
    a, _, deg = host_graph("300x257")
    e = table(g.n_nodes, 64, 12)
    ed = dev(e)
    out = ops.lgcn_chain(g, ed, n_layers, torch.empty_like(ed), torch.empty_like(ed), torch.empty_like(ed))
    e64 = e.astype(np.float64)
    layers = [e64]
    for _ in range(n_layers):
        layers.append(a @ layers[-1])
    ref, bound = chain_with_bound(a, deg, e64, np.zeros_like(e64), n_layers)
    assert np.abs(ref - np.mean(layers, axis=0)).max() < 1e-15
    assert (np.abs(out.cpu().numpy() - ref) <= bound).all()


# ------------------------------------------------------------------------------------------------------- BPR ----
def bpr_batch(nb: int, n_users: int, n_items: int, empty_item: int, seed: int):
    """nb triples; with room for them (nb >= 18): a user repeated 5 times, an item that is a positive and a
    negative, and the empty-column item as a negative. A batch of one has the empty-column negative."""
    rng = np.random.Generator(np.random.PCG64(seed))
    users = rng.integers(0, n_users, nb).astype(np.int32)
    pos = rng.integers(0, n_items, nb).astype(np.int32)
    neg = rng.integers(0, n_items, nb).astype(np.int32)
    pos[pos == empty_item] = (empty_item + 1) % n_items
    neg[0] = empty_item
    if nb >= 18:
        users[[1, 4, 7, 11, 17]] = users[1]
        pos[2], neg[9] = 3, 3
        assert (users == users[1]).sum() >= 5 and np.intersect1d(pos, neg).size
    return users, pos, neg


def bpr_bars(F: np.ndarray, n_users: int, users, pos, neg, reg: float, dF: np.ndarray | None = None):
    """(loss bar, g bar [n, d]) of hvae_lgcn_bpr, first order, V = d / 64 columns per lane; dF optionally bounds an
    error the table itself carries.

    Scores. A dot is V fmas per lane and a 6-level butterfly: |d dot| <= (V + 6) u S with S = sum |F_u F_x|; then
    x = fl(dot_p - dot_n) has ex = (V + 7) u (S_p + S_n) (+ sum |dF_u| |F_p - F_n| + |F_u| (|dF_p| + |dF_n|)).
    Loss. softplus is 1-Lipschitz and evaluated in double: each term is off by at most ex. The sum of squares is
    3 V fmas and the butterfly over non-negative terms: relative (3 V + 6) u (+ 2 |F| |dF|). The result is rounded
    to fp32 once: bar = mean(ex) + reg ((3 V + 7) u ssq + sum 2 |F| |dF|) / nb + 2 u |loss|.
    Gradient. coef = fl32(-sigmoid(-x) / nb), |sigmoid'| <= 1/4: ec = ex / (4 nb) + u |coef|. A node's row is a chain
    of T fmas (3 per user occurrence, 2 per item occurrence) over terms coef F_a, -coef F_b and r2 F_node with
    r2 = fl32(2 reg / nb): bar = sum_occ ec (|F_a| + |F_b|) + (T + 1) u sum |term| (+ the terms' own
    |coef| |dF_a| + |coef| |dF_b| + r2 |dF_node|)."""
    F = F.astype(np.float64)
    d = F.shape[1]
    V = d // 64
    users, pos, neg = (np.asarray(a, np.int64) for a in (users, pos, neg))
    nb = len(users)
    fu, fp, fn = F[users], F[n_users + pos], F[n_users + neg]
    z = np.zeros_like(F) if dF is None else dF
    du, dp, dn = z[users], z[n_users + pos], z[n_users + neg]
    x = (fu * fp).sum(1) - (fu * fn).sum(1)
    ex = (V + 7) * U * ((np.abs(fu * fp)).sum(1) + np.abs(fu * fn).sum(1)) \
        + (du * np.abs(fp - fn) + np.abs(fu) * (dp + dn)).sum(1)
    ssq = (fu ** 2).sum() + (fp ** 2).sum() + (fn ** 2).sum()
    dssq = 2 * (np.abs(fu) * du + np.abs(fp) * dp + np.abs(fn) * dn).sum()
    loss, _ = LR.bpr_oracle(F, n_users, users, pos, neg, reg)
    loss_bar = ex.mean() + reg * ((3 * V + 7) * U * ssq + dssq) / nb + 2 * U * abs(loss)
    c = np.abs(-1.0 / (1.0 + np.exp(x)) / nb)[:, None]
    ec = (ex / (4 * nb))[:, None] + U * c
    r2 = 2 * reg / nb
    inp, terms, T = np.zeros_like(F), np.zeros_like(F), np.zeros(len(F))
    for node, others, dothers, me, dme, t in ((users, np.abs(fp) + np.abs(fn), dp + dn, fu, du, 3),
                                              (n_users + pos, np.abs(fu), du, fp, dp, 2),
                                              (n_users + neg, np.abs(fu), du, fn, dn, 2)):
        np.add.at(inp, node, ec * others + c * dothers + r2 * dme)
        np.add.at(terms, node, c * others + r2 * np.abs(me))
        np.add.at(T, node, t)
    return loss_bar, inp + (T[:, None] + 1) * U * terms


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("nb", [1, 18, 1024])
def test_bpr_against_float64(hip_device, nb, d):
    """Loss, every touched row of g and exact zeros elsewhere, at bpr_bars' derived bars (its docstring)."""
    from hvae import ops
    n_users, n_items, empty_item = 300, 257, 100
    F = table(n_users + n_items, d, 20 + d, std=0.3)
    users, pos, neg = bpr_batch(nb, n_users, n_items, empty_item, seed=nb)
    reg = 1e-4
    Fd = dev(F)
    args = (Fd, n_users, dev(users), dev(pos), dev(neg), reg)
    accum = torch.full((1,), 2.0, dtype=torch.float64, device=Fd.device)
    loss, g = ops.lgcn_bpr(*args, g=torch.full_like(Fd, float("nan")), loss_accum=accum)
    want_loss, want_g = LR.bpr_oracle(F, n_users, users, pos, neg, reg)
    loss_bar, g_bar = bpr_bars(F, n_users, users, pos, neg, reg)
    got_g = g.cpu().numpy()
    err = np.abs(got_g - want_g)
    print(f"nb={nb} d={d}: loss err {abs(loss.item() - want_loss):.3e} bar {loss_bar:.3e}; "
          f"g max err/bar {np.max(err / np.maximum(g_bar, 1e-300)):.3f}")
    assert abs(loss.item() - want_loss) <= loss_bar
    assert accum.item() == 2.0 + float(loss.item())
    touched = np.zeros(n_users + n_items, bool)
    touched[users] = touched[n_users + pos] = touched[n_users + neg] = True
    assert touched[n_users + empty_item]
    assert (got_g[~touched] == 0).all() and (err[touched] <= g_bar[touched]).all()
    assert np.abs(want_g[touched]).max() > 100 * g_bar[touched].max()  # the bar is sharp against a dropped term
    loss2, g2 = ops.lgcn_bpr(*args)
    assert torch.equal(loss, loss2) and torch.equal(g, g2)


def test_bpr_refuses_bad_batches(hip_device):
    from hvae import ops
    F = dev(table(20, 64, 1))
    i = torch.zeros(1025, dtype=torch.int32, device=F.device)
    with pytest.raises(ValueError, match="1 to 1024"):
        ops.lgcn_bpr(F, 10, i, i, i, 1e-4)
    with pytest.raises(ValueError, match="1 to 1024"):
        ops.lgcn_bpr(F, 10, i[:0], i[:0], i[:0], 1e-4)
    loss, g = ops.lgcn_bpr(F, 10, i[:1] + 10, i[:1], i[:1], 1e-4)  # a user id outside [0, n_users)
    assert torch.isnan(loss).all()


# ----------------------------------------------------------------------------------------------- one full step ----
def test_one_train_step_against_torch_autograd(hip_device):
    """Forward chain, BPR, backward chain and Adam on 300x257 against torch's CPU autograd (torch.sparse.mm,
    torch.optim.Adam) from the same table and batch.

    The loss bar is bpr_bars' with the forward chain's bound as the table's own error. The updated table's bar is
    composed likewise: the BPR gradient's bar with that table error, carried through the backward chain's bound,
    then through Adam's first step p - lr g / (|g| + eps), whose slope in g is at most lr eps / (|g| - dg + eps)^2,
    plus 16 u lr for the update's own arithmetic and u |p| for the final rounding. The float64 restatement is the
    truth; torch's own fp32 step is printed beside the device's for orientation (the same arithmetic in another
    order)."""
    from hvae import ops
    name, d, L, lr, reg, eps = "300x257", 64, 3, 1e-3, 1e-4, 1e-8
    g = device_graph(name)
    a, _, deg = host_graph(name)
    matrix = LR.kernel_graph(name)
    n_users, n_items = matrix.shape
    e0 = table(g.n_nodes, d, 31)
    rng = np.random.Generator(np.random.PCG64(32))
    pu, pi = matrix.nonzero()
    pick = rng.permutation(len(pu))[:1024]
    users, pos = pu[pick].astype(np.int32), pi[pick].astype(np.int32)
    neg = rng.integers(0, n_items, 1024).astype(np.int32)

    # device
    E = dev(e0.copy())
    F, gr, dE, ta, tb = (torch.empty_like(E) for _ in range(5))
    m, v = torch.zeros_like(E), torch.zeros_like(E)
    step = torch.zeros(1, dtype=torch.int64, device=E.device)
    ops.lgcn_chain(g, E, L, F, ta, tb)
    loss, _ = ops.lgcn_bpr(F, n_users, dev(users), dev(pos), dev(neg), reg, g=gr)
    ops.lgcn_chain(g, gr, L, dE, ta, tb)
    ops.adam_dense(ops.adam_config(lr, (0.9, 0.999), eps, 0.0, step), E, m, v, dE)
    got = E.cpu().numpy()

    # torch autograd, fp32 and float64
    def torch_step(dtype):
        coo = a.tocoo()
        adj = torch.sparse_coo_tensor(torch.tensor(np.stack([coo.row, coo.col])), torch.tensor(coo.data, dtype=dtype),
                                      coo.shape)
        p = torch.nn.Parameter(torch.tensor(e0, dtype=dtype))
        opt = torch.optim.Adam([p], lr=lr)
        layers = [p]
        for _ in range(L):
            layers.append(torch.sparse.mm(adj, layers[-1]))
        f = torch.stack(layers, dim=1).mean(dim=1)
        u_, p_, n_ = f[torch.tensor(users).long()], f[n_users + torch.tensor(pos).long()], f[n_users + torch.tensor(neg).long()]
        ls = -torch.nn.functional.logsigmoid((u_ * p_).sum(1) - (u_ * n_).sum(1)).mean() \
            + reg * (u_.norm(2).pow(2) + p_.norm(2).pow(2) + n_.norm(2).pow(2)) / len(users)
        ls.backward()
        grad = p.grad.detach().numpy().astype(np.float64)
        opt.step()
        return float(ls), p.detach().numpy().astype(np.float64), grad

    loss64, want, grad64 = torch_step(torch.float64)
    loss32, e32, _ = torch_step(torch.float32)

    e64 = e0.astype(np.float64)
    f64, bF = chain_with_bound(a, deg, e64, np.zeros_like(e64), L)
    loss_bar, g_bar = bpr_bars(f64, n_users, users, pos, neg, reg, dF=bF)
    _, g64 = LR.bpr_oracle(f64, n_users, users, pos, neg, reg)
    de64, bdE = chain_with_bound(a, deg, g64, g_bar, L)
    assert np.abs(de64 - grad64).max() <= 1e-12  # the restatement is torch's float64 gradient
    slope = lr * eps / (np.maximum(np.abs(de64) - bdE, 0) + eps) ** 2
    e_bar = slope * bdE + 16 * U * lr + U * np.abs(want)
    err = np.abs(got - want)
    print(f"step: loss err {abs(loss.item() - loss64):.3e} bar {loss_bar:.3e} (torch fp32 {abs(loss32 - loss64):.3e}); "
          f"table max err/bar {np.max(err / e_bar):.3f} (torch fp32 {np.max(np.abs(e32 - want) / e_bar):.3f}), "
          f"max err {err.max():.3e}")
    assert abs(loss.item() - loss64) <= loss_bar
    assert (err <= e_bar).all()
    assert np.abs(got - e0).max() > 0.5 * lr  # the step moved the table


# ------------------------------------------------------------------------------------------ golden trajectory ----
@functools.lru_cache(maxsize=None)
def fitted(epochs: int):
    import src.ml.lightgcn as lg
    matrix, _, _ = LR.fixture_graph()
    torch.manual_seed(LR.SEED_TORCH)
    np.random.seed(LR.SEED_NUMPY)
    model = lg.LightGCNRecommender(embedding_dim=LR.DIM, n_layers=LR.LAYERS, epochs=epochs)
    model.fit(matrix)
    return model, LR.state_digest()


@pytest.mark.parametrize("epochs", [1, 5])
def test_fit_follows_the_reference_trajectory(hip_device, epochs):
    """Final user and item embeddings within the fixture's bar (16 x the reference's own fp32-against-float64 noise,
    tests/golden/make_lightgcn_fixture.py) of the reference's, and numpy left where the reference leaves it."""
    model, state = fitted(epochs)
    fx, meta = LR.fixture(), LR.fixture_meta()
    assert state == meta["state_digest"][str(epochs)]
    for key, got in ((f"user_e{epochs}", model.user_final_emb), (f"item_e{epochs}", model.item_final_emb)):
        err = np.abs(got.cpu().numpy().astype(np.float64) - fx[key]).max()
        print(f"{key}: max err {err:.3e}, bar {meta['bar'][key]:.3e}, noise {meta['noise'][key]:.3e}")
        assert got.dtype == torch.float32 and err <= meta["bar"][key]
    assert np.abs(fx[f"user_e{epochs}"] - fx["init"][:LR.N_USERS]).max() > 1e3 * meta["bar"][f"user_e{epochs}"]


def ref_bracket(scores: np.ndarray, cand: np.ndarray, t: int, tol: float):
    return int((scores[cand] > scores[t] + tol).sum()), int((scores[cand] >= scores[t] - tol).sum())


def test_ranks_lie_in_the_reference_brackets(hip_device):
    """99-negative ranks from baseline.evaluate_ranks inside [#{ref > s_t + tol}, #{ref >= s_t - tol}] of the
    reference's stored scores, tol = twice the scores' bar (the test item's and the candidate's score each move by
    one bar); full ranking through hvae_topk with the seen items masked, inside the same brackets; predict is the
    fp32 score row within the bar."""
    import src.ml.baseline as b
    model, _ = fitted(5)
    matrix, users, tests = LR.fixture_graph()
    fx, meta = LR.fixture(), LR.fixture_meta()
    bar = meta["bar"]["scores"]
    row = model.predict(3)
    assert row.dtype == np.float32 and row.shape == (LR.N_ITEMS,)
    err = np.abs(model.score_all(users).cpu().numpy().astype(np.float64) - fx["scores"]).max()
    print(f"scores: max err {err:.3e}, bar {bar:.3e}")
    assert err <= bar and np.abs(row - fx["scores"][3]).max() <= bar
    state = LR.state_digest()
    ranks = b.evaluate_ranks(model, matrix, users, tests, [5, 10, 20], LR.N_NEG)
    assert LR.state_digest() == state  # fewer than 99 negatives exist: nothing is drawn, as in the reference
    K = 20
    full = b.evaluate_ranks(model, matrix, users, tests, [5, 10, K], None)
    inside = 0
    for u, t, r, f, ref_rank in zip(users, tests, ranks, full, fx["ranks"]):
        cand = np.setdiff1d(np.arange(LR.N_ITEMS), np.append(matrix[u].indices, t))
        lo, hi = ref_bracket(fx["scores"][u], cand, t, 2 * bar)
        assert lo <= r <= hi and lo <= ref_rank <= hi
        assert lo <= f <= hi if f < K else hi >= K
        inside += f < K
    assert 0 < inside < len(users)


# --------------------------------------------------------------------------------------------------- end to end ----
def test_main_writes_the_lightgcn_entry_beside_an_existing_one(hip_device, tmp_path):
    import src.ml.lightgcn as lg
    from gen import write_planted_artifacts
    data, _ = write_planted_artifacts(tmp_path, dict(n_users=60, n_items=50, d=4, n_clusters=2))
    out = tmp_path / "models" / "figures" / "baseline_results.json"
    out.parent.mkdir(parents=True)
    pop = {"5": {"recall": 0.1, "ndcg": 0.1, "hit_ratio": 0.1}, "training_time_seconds": 0.01}
    out.write_text(json.dumps({"Popularity": pop}))
    np.random.seed(0)
    torch.manual_seed(0)
    with mock.patch.object(sys, "argv", ["lightgcn", "--data", str(data), "--epochs", "2", "--n-negatives", "20",
                                         "--k-values", "5", "10"]):
        lg.main()
    got = json.loads(out.read_text())
    assert list(got) == ["Popularity", "LightGCN"] and got["Popularity"] == pop
    assert list(got["LightGCN"]) == ["5", "10", "training_time_seconds"]
    for k in ("5", "10"):
        assert set(got["LightGCN"][k]) == {"recall", "ndcg", "hit_ratio"}
        assert all(0.0 <= v <= 1.0 for v in got["LightGCN"][k].values())
    assert got["LightGCN"]["10"]["hit_ratio"] >= got["LightGCN"]["5"]["hit_ratio"]


def test_a_second_fit_from_the_same_seeds_is_bitwise_equal(hip_device):
    import src.ml.lightgcn as lg
    matrix, _, _ = LR.fixture_graph()
    first, _ = fitted(1)
    torch.manual_seed(LR.SEED_TORCH)
    np.random.seed(LR.SEED_NUMPY)
    again = lg.LightGCNRecommender(embedding_dim=LR.DIM, n_layers=LR.LAYERS, epochs=1)
    again.fit(matrix)
    assert torch.equal(first.ego, again.ego)
    assert torch.equal(first.user_final_emb, again.user_final_emb)
    assert torch.equal(first.item_final_emb, again.item_final_emb)
