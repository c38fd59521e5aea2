"""Fused exact top-K at d = 1024 (hvae_topk_fused's D-split kernels: the k axis in two halves, run one after the
other in the seed pass and by the two waves of a pair in the LDS scan) against a float64 ranking of the same
fp32 inputs, and the public ranking path (HybridVAE.recommend / topk_scores) using it instead of the fp32 score
matrix.

The bar is tests/test_gpu_topk.py's, whose helpers are restated here: indices identical except between items
whose float64 scores are within 2e-6 max|S| of each other, returned scores within the same tolerance (the fp32
rescore is the same sum at every width; nothing in the split changes its error model)."""
import numpy as np
import pytest
import torch

from gen import synth_csr, synth_embeddings

pytestmark = pytest.mark.gpu

D = 1024


def _case(hip_device, R, N, seed, scale=4.0):
    from hvae import ops
    E = torch.as_tensor(synth_embeddings(N, D, seed=seed))
    g = torch.Generator().manual_seed(seed + 1)
    U = torch.randn(R, D, generator=g) * (scale / D ** 0.5)
    Ed = E.to(hip_device)
    img = ops.decoder_image(Ed)
    emax = ops.row_norm_max(Ed)
    return U, E, U.to(hip_device), Ed, img, emax


def _check(idx, val, U, E, k, seen=None):
    S = U.double() @ E.double().t()
    if seen is not None:
        for r, items in enumerate(seen):
            S[r, items] = -np.inf
    idx = idx.cpu().long()
    val = val.cpu().double()
    tol = 2e-6 * S.abs().max().item()
    for r in range(S.shape[0]):
        order = sorted(range(S.shape[1]), key=lambda i: (-S[r, i].item(), -i))[:k] if S.shape[1] <= 4096 else None
        if order is None:
            top = torch.topk(S[r], k + 16)
            cand = sorted(zip(top.values.tolist(), top.indices.tolist()), key=lambda t: (-t[0], -t[1]))
            order = [i for _, i in cand[:k]]
        got = idx[r].tolist()
        assert len(set(got)) == k, r
        for j in range(k):
            if got[j] != order[j]:
                assert abs(S[r, got[j]].item() - S[r, order[j]].item()) <= tol, (r, j, got[j], order[j])
            assert abs(val[r, j].item() - S[r, got[j]].item()) <= tol, (r, j)
        if seen is not None:
            assert not set(got) & set(seen[r].tolist()), r


def _exclude(hip_device, X, R, N):
    from hvae import ops
    csr = ops.csr_from_scipy(X, hip_device)
    return ops.Csr(csr.row_ptr, csr.col_idx, csr.vals, N, rows=torch.arange(R, dtype=torch.int32, device=hip_device))


@pytest.mark.parametrize("R,N,k", [(37, 5003, 50),      # baseline
                                   (130, 30011, 10),    # more than one 64-user block, a partial last group
                                   (65, 777, 5),        # one user past a 64-user block
                                   (9, 2000, 100),      # K above the 63-slot heap
                                   (1, 100_000, 10)])   # one user, many splits
def test_topk_fused_d1024_exact(hip_device, R, N, k):
    from hvae import ops
    U, E, Ud, Ed, img, emax = _case(hip_device, R, N, seed=N + D)
    idx, val, flag = ops.topk_fused(Ud, img, Ed, emax, k, with_flags=True)
    assert int(flag.sum()) == 0  # the fused path certified every row itself
    _check(idx, val, U, E, k)


@pytest.mark.parametrize("R,N,k", [(5, 20, 5),      # N below one 32-item tile
                                   (2, 31, 7),      # just under one tile
                                   (2, 33, 7),      # just over one tile
                                   (3, 50, 50),     # k = N
                                   (70, 4097, 1)])  # k = 1
def test_topk_fused_d1024_edge_shapes(hip_device, R, N, k):
    from hvae import ops
    U, E, Ud, Ed, img, emax = _case(hip_device, R, N, seed=3 * N + D)
    idx, val = ops.topk_fused(Ud, img, Ed, emax, k)
    _check(idx, val, U, E, k)


def test_topk_fused_d1024_empty_batch(hip_device):
    from hvae import ops
    U, E, Ud, Ed, img, emax = _case(hip_device, 2, 600, seed=17)
    R0 = ops.topk_fused(Ud[:0], img, Ed, emax, 6)
    assert R0[0].shape == (0, 6) and R0[1].shape == (0, 6)


def test_topk_fused_d1024_exclude_seen(hip_device):
    """exclude_seen: K_u = k + |seen_u| shortlist, seen items removed before ranking."""
    from hvae import ops
    R, N, k = 50, 40000, 20
    U, E, Ud, Ed, img, emax = _case(hip_device, R, N, seed=7 * N)
    X = synth_csr(R, N, lam=15.0, seed=N)
    ex = _exclude(hip_device, X, R, N)
    idx, val, flag = ops.topk_fused(Ud, img, Ed, emax, k, exclude=ex, with_flags=True)
    assert int(flag.sum()) == 0
    seen = [torch.as_tensor(X[r].indices.astype(np.int64)) for r in range(R)]
    _check(idx, val, U, E, k, seen)
    # the same as the exact score-matrix path (hvae_gemm_f32 + hvae_topk)
    i2, _ = ops.topk(ops.gemm(Ud, Ed.t()), k, exclude=ex)
    assert (idx.cpu() == i2.cpu()).float().mean() > 0.99


def test_topk_fused_d1024_flagged_rows_take_the_exact_path(hip_device):
    """Rows the fused kernel cannot certify (more seen items than the shortlist heap, an all-but-5-seen row) are
    flagged and ranked by the exact path; the answer stays exact."""
    from scipy.sparse import csr_matrix
    from hvae import ops
    R, N, k = 6, 3000, 8
    U, E, Ud, Ed, img, emax = _case(hip_device, R, N, seed=5)
    rng = np.random.default_rng(0)
    rows_l, cols_l = [], []
    sizes = [3, 400, 0, 10, 2995, 260]  # rows 1, 5: |seen| + k > 256 -> flagged; row 4: 5 unseen < k -> flagged
    for r, s in enumerate(sizes):
        c = rng.choice(N, s, replace=False)
        rows_l += [r] * s
        cols_l += c.tolist()
    X = csr_matrix((np.ones(len(rows_l), np.float32), (rows_l, cols_l)), shape=(R, N))
    ex = _exclude(hip_device, X, R, N)
    idx, val, flag = ops.topk_fused(Ud, img, Ed, emax, k, exclude=ex, with_flags=True)
    assert flag.cpu().tolist() == [0, 1, 0, 0, 1, 1]
    X.sort_indices()
    seen = [torch.as_tensor(X[r].indices.astype(np.int64)) for r in range(R)]
    ok = [r for r in range(R) if r != 4]
    _check(idx[ok], val[ok], U[ok], E, k, [seen[r] for r in ok])
    # row 4 has 5 unseen items: those 5 first (exact order), then -inf
    S4 = (U[4].double() @ E.double().t())
    S4[seen[4]] = -np.inf
    top5 = sorted(range(N), key=lambda i: (-S4[i].item(), -i))[:5]
    assert idx[4, :5].cpu().tolist() == top5
    assert torch.isinf(val[4, 5:]).all()


def test_topk_fused_d1024_bf16_midpoint_adversarial(hip_device):
    """tests/test_gpu_topk.py's midpoint construction at d = 1024: eps_u must cover the bf16 rounding of BOTH u and
    E over all 1024 k's, whichever wave summed them. u's first half (one wave's D-half) and the true top item's
    row sit just below the bf16 rounding midpoint, so the top's bf16 score is 512 against 516.007 in fp32; 40
    bf16-exact competitors live on u's other half at 515.44 .. 515.94 in both precisions: under the top in fp32,
    at least 3.43 above it in bf16, which is more than a 2^-8 bound (2.86) and less than the 2^-7 one."""
    from hvae import ops
    N, k = 3000, 10
    c = 1.0 + 2.0 ** -8 - 2.0 ** -20  # rounds down to 1.0 in bf16
    u = torch.ones(1, D, dtype=torch.float64)
    u[0, : D // 2] = c
    g = torch.Generator().manual_seed(5)
    E = torch.rand(N, D, generator=g, dtype=torch.float64) * 0.05  # the rest: far below
    E[0] = 0.0
    E[0, : D // 2] = c  # the true top
    for j in range(1, 41):  # competitors: bf16-exact, on u's exact half
        E[j] = 0.0
        n_up = (55 + (j % 9)) * (D // 128)
        E[j, D // 2:] = 1.0
        E[j, D // 2: D // 2 + n_up] = 1.0078125
    U = u.float()
    Ef = E.float()
    S = U.double() @ Ef.double().t()
    assert int(S[0].argmax()) == 0 and S[0, 0] - S[0, 1:41].max() > 0  # the true top wins in float64
    bf = (U.bfloat16().double() @ Ef.bfloat16().double().t())[0]
    bound8 = (U.double().norm() * Ef.double().norm(dim=1).max()).item() * 2.0 ** -8
    assert bf[1:41].min() - bf[0] > bound8 * 1.02  # a 2^-8 bound would have dropped the top item
    Ud, Ed = U.to(hip_device), Ef.to(hip_device)
    img = ops.decoder_image(Ed)
    emax = ops.row_norm_max(Ed)
    idx, val, flag = ops.topk_fused(Ud, img, Ed, emax, k, with_flags=True)
    assert int(flag.sum()) == 0
    assert int(idx[0, 0]) == 0
    _check(idx, val, U, Ef, k)
    i2, _ = ops.topk(ops.gemm(Ud, Ed.t()), k)  # the exact score-matrix path
    assert idx.cpu().tolist() == i2.cpu().tolist()


def test_topk_fused_d1024_exact_ties(hip_device):
    """Items 100 .. 119 are copies of one row aligned with u, so they hold the top 20 with bit-equal fp32 scores:
    ties go to the larger item index."""
    from hvae import ops
    N, k = 2000, 10
    U, E, _, _, _, _ = _case(hip_device, 1, N, seed=23)
    E = E.clone()
    E[100:120] = 3.0 * U[0] / U[0].norm()  # |other rows| = 1: by Cauchy-Schwarz nothing else comes close
    Ud, Ed = U.to(hip_device), E.to(hip_device)
    idx, val = ops.topk_fused(Ud, ops.decoder_image(Ed), Ed, ops.row_norm_max(Ed), k)
    assert idx[0].cpu().tolist() == list(range(119, 109, -1))
    assert len(set(val[0].cpu().tolist())) == 1


def test_public_ranking_path_is_fused_at_d1024(hip_device, monkeypatch):
    """HybridVAE.recommend and topk_scores at d = 1024 go through hvae_topk_fused: with the score-matrix top-K
    (ops.topk) made to raise they still return the float64 ranking (tests/test_gpu_embed_dims.py::test_ranking's
    model, inputs and tolerance)."""
    from hvae import ops
    from src.ml.model import HybridVAE
    R_, N, k = 70, 2500, 20
    X = synth_csr(R_, N, lam=15.0, seed=D)
    E = synth_embeddings(N, D, seed=D + 1)
    torch.manual_seed(3)
    m = HybridVAE(N, E, latent_dim=64, hidden_dims=[256], dropout=0.3, beta=0.2).to(hip_device).eval()
    z = torch.randn(R_, 64, generator=torch.Generator().manual_seed(9)).to(hip_device)
    with torch.no_grad():
        u = m.projection_layer(z).contiguous()
    ex = _exclude(hip_device, X, R_, N)
    # no row of this input is flagged (a flagged row is ranked through ops.topk by design)
    E32 = m.item_embeddings.detach().contiguous()
    img, emax = ops.decoder_image(E32), ops.row_norm_max(E32)
    for e in (None, ex):
        assert int(ops.topk_fused(u, img, E32, emax, k, exclude=e, with_flags=True)[2].sum()) == 0

    def no_score_matrix(*a, **kw):
        raise AssertionError("the fp32 score-matrix top-K (ops.topk) was called at d = 1024")

    monkeypatch.setattr(ops, "topk", no_score_matrix)
    S = u.double().cpu() @ torch.as_tensor(E).double().t()
    tol = 2e-5 * S.abs().max().item()

    def check(idx, val, S):
        for r in range(R_):
            ref = torch.topk(S[r], k)
            for j in range(k):
                i = int(idx[r, j])
                assert i == int(ref.indices[j]) or abs(S[r, i].item() - ref.values[j].item()) <= tol
                assert abs(val[r, j].item() - S[r, i].item()) <= tol

    idx, val = m.recommend(z, top_k=k)
    check(idx.cpu(), val.cpu(), S)
    idx, val = m.topk_scores(u, k, exclude=ex)
    Sx = S.clone()
    for r in range(R_):
        Sx[r, torch.as_tensor(X[r].indices.astype(np.int64))] = -float("inf")
    check(idx.cpu(), val.cpu(), Sx)
