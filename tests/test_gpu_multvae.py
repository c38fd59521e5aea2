"""The Mult-VAE baseline on the device: its three kernels against float64 at bars derived from first-order rounding
bounds, one full train step against torch autograd in float64, reproducibility, eval mode and the command line.

Rounding model (u = 2^-24): one fp32 operation is off by at most u relative; sqrtf and the division are correctly
rounded; the device library documents tanhf at 2 ulp and expf / logf at 1 ulp, i.e. 4 u and 2 u relative. A chain
of k fmas over terms of summed magnitude A is off by at most k u A. The multipliers are 0 or 2 at p = 0.5: exact.
"""
import json
import sys
from unittest import mock

import numpy as np
import pytest
import torch

import multvae_ref as MR
import philox_ref as PR

pytestmark = pytest.mark.gpu
U = MR.U
TAG_IN, TAG_H1, TAG_H2 = 0x400, 0x401, 0x402
P = 0.5


def _dev(a, dev, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)


def _graph(name):
    return MR.g_small() if name == "small" else MR.g_wide()


def _rows(name, nb, distinct):
    """Batch rows: the special rows first (the 85- / 300-entry row at nb = 1), the rest shuffled."""
    m = _graph(name)
    rng = np.random.Generator(np.random.PCG64(nb))
    first = [2, 0, 1] if name == "small" else [5]
    if nb == 1:
        return np.array(first[:1], np.int32)
    if distinct:
        rest = rng.permutation(np.setdiff1d(np.arange(m.shape[0]), first))
        return np.concatenate([first, rest])[:nb].astype(np.int32)
    return np.concatenate([first, rng.integers(0, m.shape[0], nb - len(first))]).astype(np.int32)


# ------------------------------------------------------------------------------------------------ encoder_fwd ----
ENC_CASES = [("small", 1, True), ("small", 88, True), ("small", 512, True),
             ("wide", 1, True), ("wide", 37, True), ("wide", 88, False), ("wide", 512, False)]


@pytest.mark.parametrize("H", [8, 600])
@pytest.mark.parametrize("name,nb,distinct", ENC_CASES)
def test_encoder_fwd_against_float64(hip_device, name, nb, distinct, H):
    """t, h and xs with injected multipliers. Bars: xs carries the sqrt, the division and the multiplier, 3 u
    relative; a is a chain of cnt fmas over terms that each carry xs's 3 u: (cnt + 3) u A with A = |b1| + sum |xs w|;
    tanh is 1-Lipschitz and adds 4 u |t|; h = t * mult adds u |h|. With distinct rows also: the Philox run is bitwise
    the run with philox_ref's multipliers injected, and the xs batch through w1_rowgrad gives the float64 dW1t within
    (cnt_j + 1) u sum |xs da| + 3 u sum |xs da| (a chain of cnt_j fmas over terms that carry xs's error)."""
    from hvae import ops
    dev = hip_device
    m = _graph(name)
    N = m.shape[1]
    rows = _rows(name, nb, distinct)
    rng = np.random.Generator(np.random.PCG64(7 * nb + H))
    w1t = (rng.standard_normal((N, H)) / np.sqrt(8)).astype(np.float32)
    b1 = (rng.standard_normal(H) * 0.1).astype(np.float32)
    in_mult = (rng.random(m.nnz) >= P).astype(np.float32) * 2
    m1 = (rng.random((nb, H)) >= P).astype(np.float32) * 2
    x = ops.csr_from_scipy(m, dev)
    assert np.array_equal(x.col_idx.cpu().numpy(), m.indices)
    xb = ops.Csr(x.row_ptr, x.col_idx, x.vals, N, rows=_dev(rows, dev, torch.int32))
    W, B1 = _dev(w1t, dev), _dev(b1, dev)

    # rows that repeat would each write their entries of xs: it is saved for distinct rows only
    h, t, xs = ops.mvae_encoder_fwd(xb, W, B1, P, P, True, in_mult=_dev(in_mult, dev), drop_mult=_dev(m1, dev),
                                    t_out=torch.empty(nb, H, device=dev), save=distinct)
    xs64, a64, t64, h64, A, cnt = MR.encoder64(m, rows, w1t, b1, in_mult, m1)
    bar_a = (cnt[:, None] + 3) * U * A
    bar_t = bar_a + 4 * U * np.abs(t64)
    bar_h = m1 * bar_t + U * np.abs(h64)
    t_, h_ = t.cpu().numpy().astype(np.float64), h.cpu().numpy().astype(np.float64)
    print(f"encoder {name} nb={nb} H={H}: t err {np.abs(t_ - t64).max():.3e} (largest err / bar "
          f"{(np.abs(t_ - t64) / bar_t).max():.3f}), h err {np.abs(h_ - h64).max():.3e}")
    assert (np.abs(t_ - t64) <= bar_t).all() and (np.abs(h_ - h64) <= bar_h).all()
    assert np.isfinite(h_).all()
    if "small" == name and nb > 1:  # the empty row: h = Drop(tanh(b1))
        assert np.abs(h_[1] - np.tanh(b1.astype(np.float64)) * m1[1]).max() <= 10 * U
    if not distinct:
        return
    live, xs_ = ~np.isnan(xs64), xs.cpu().numpy()
    assert (np.abs(xs_[live] - xs64[live]) <= 3 * U * np.abs(xs64[live])).all()

    # Philox: bitwise the injected run
    seed, step = 0x1234567 + H, 5
    step_dev = torch.full((1,), step, dtype=torch.int64, device=dev)
    hp, tp, xp = ops.mvae_encoder_fwd(xb, W, B1, P, P, True, seed=seed, step=step_dev)
    inj_in = np.ones(m.nnz, np.float32)
    for b, r in enumerate(rows):
        s, e = m.indptr[r], m.indptr[r + 1]
        idx = np.uint64(b) * np.uint64(N) + m.indices[s:e].astype(np.uint64)
        inj_in[s:e] = np.where(PR.keep_idx(seed, step, TAG_IN, idx, P), PR.scale(P), np.float32(0))
    inj_m1 = PR.mult(seed, step, TAG_H1, nb, H, P)
    hi, ti, xi = ops.mvae_encoder_fwd(xb, W, B1, P, P, True, in_mult=_dev(inj_in, dev), drop_mult=_dev(inj_m1, dev))
    sel = torch.as_tensor(np.flatnonzero(live), device=dev)
    assert torch.equal(hp, hi) and torch.equal(tp, ti) and torch.equal(xp[sel], xi[sel])
    if nb * H >= 4096:
        assert 0.4 < float((hp == 0).float().mean()) < 0.6

    # the xs batch feeds the existing row gradient
    da = rng.standard_normal((nb, H)).astype(np.float32)
    rg = ops.RowGradBuffers(N, H, max(int(live.sum()), 1), dev)
    ops.w1_rowgrad(ops.Csr(x.row_ptr, x.col_idx, xs, N, rows=xb.rows), _dev(da, dev), rg)
    dense = torch.zeros(N, H, device=dev)
    ops.rowgrad_to_dense(rg, dense)
    want, mag, cj = np.zeros((N, H)), np.zeros((N, H)), np.zeros(N)
    for b, r in enumerate(rows):
        s, e = m.indptr[r], m.indptr[r + 1]
        j = m.indices[s:e]
        want[j] += xs64[s:e, None] * da[b].astype(np.float64)
        mag[j] += np.abs(xs64[s:e, None] * da[b].astype(np.float64))
        cj[j] += 1
    assert (np.abs(dense.cpu().numpy() - want) <= (cj[:, None] + 4) * U * mag).all()


def test_encoder_eval_mode_ignores_the_seeds_and_refusals(hip_device):
    from hvae import ops
    dev = hip_device
    m = MR.g_small()
    x = ops.csr_from_scipy(m, dev)
    W, b1 = torch.randn(97, 600, device=dev) * 0.1, torch.randn(600, device=dev) * 0.1
    step = torch.full((1,), 3, dtype=torch.int64, device=dev)
    h0, _, _ = ops.mvae_encoder_fwd(x, W, b1, P, P, False, seed=1, step=step, save=False)
    h1, _, _ = ops.mvae_encoder_fwd(x, W, b1, 0.0, 0.0, False, seed=2, save=False)
    assert torch.equal(h0, h1)
    _, a64, t64, _, A, cnt = MR.encoder64(m, np.arange(600), W.cpu().numpy(), b1.cpu().numpy())
    assert (np.abs(h0.cpu().numpy() - t64) <= (cnt[:, None] + 3) * U * A + 4 * U * np.abs(t64)).all()
    for H in (6, 2052):
        with pytest.raises(ValueError, match="multiples of 4 from 4 to 2048"):
            ops.mvae_encoder_fwd(x, torch.zeros(97, H, device=dev), torch.zeros(H, device=dev), P, P, False)
    # the library's own check, behind the wrapper's
    from hvae import _lib
    rc = _lib.lib().hvae_mvae_encoder_fwd(x.ref, W.data_ptr(), b1.data_ptr(), 6, 0.5, 0.5, None, None, 0, None, 0,
                                          None, None, h0.data_ptr(), None)
    assert rc == _lib.HVAE_ERR_UNSUPPORTED and "multiple of 4" in _lib.last_error()
    rc = _lib.lib().hvae_mvae_nll(x.ref, None, 100, 1.0, None, None, None)
    assert rc == -1 and "null" in _lib.last_error()


# -------------------------------------------------------------------------------------------------- tanh_drop ----
@pytest.mark.parametrize("W", [4, 200, 600])
@pytest.mark.parametrize("nb", [1, 88, 512])
def test_tanh_drop_forward_and_backward(hip_device, nb, W):
    """Over views with a leading dimension of W + 8. Forward: 4 u |t| (tanhf), + u |h| for the product. Backward
    from the same fp32 t: a product, the fma 1 - t^2 (one rounding of the exact value) and a product: 3 u |da|.
    Philox (tag 0x402) is bitwise the injected run; without a mask h, t and a may be one tensor."""
    from hvae import ops
    dev = hip_device
    rng = np.random.Generator(np.random.PCG64(nb * 1000 + W))
    ld = W + 8
    a = (rng.standard_normal((nb, W)) * 2).astype(np.float32)
    a.flat[0] = 30.0  # saturated
    mult = (rng.random((nb, W)) >= P).astype(np.float32) * 2
    dh = rng.standard_normal((nb, W)).astype(np.float32)
    A = torch.full((nb, ld), float("nan"), device=dev)
    A[:, :W] = _dev(a, dev)
    T, Hh, DH = torch.full_like(A, 7.0), torch.full_like(A, 7.0), torch.full_like(A, float("nan"))
    DH[:, :W] = _dev(dh, dev)
    M = _dev(mult, dev)
    h, t = ops.mvae_tanh_drop_fwd(A[:, :W], P, True, TAG_H2, drop_mult=M, t_out=T[:, :W], h_out=Hh[:, :W])
    t64 = np.tanh(a.astype(np.float64))
    t_, h_ = t.cpu().numpy(), h.cpu().numpy()
    assert (np.abs(t_ - t64) <= 4 * U * np.abs(t64)).all()
    assert (np.abs(h_ - t64 * mult) <= 5 * U * np.abs(t64 * mult)).all()
    assert (T[:, W:] == 7.0).all() and (Hh[:, W:] == 7.0).all()  # nothing beyond W is written
    da = ops.mvae_tanh_drop_bwd(DH[:, :W], T[:, :W], P, True, TAG_H2, drop_mult=M)
    want = dh.astype(np.float64) * mult * (1 - t_.astype(np.float64) ** 2)
    assert (np.abs(da.cpu().numpy() - want) <= 3 * U * np.abs(want)).all()

    seed, step = 99 + W, 11
    step_dev = torch.full((1,), step, dtype=torch.int64, device=dev)
    inj = _dev(PR.mult(seed, step, TAG_H2, nb, W, P), dev)
    hp, tp = ops.mvae_tanh_drop_fwd(A[:, :W], P, True, TAG_H2, seed=seed, step=step_dev)
    hi, ti = ops.mvae_tanh_drop_fwd(A[:, :W], P, True, TAG_H2, drop_mult=inj)
    assert torch.equal(hp, hi) and torch.equal(tp, ti)
    dp = ops.mvae_tanh_drop_bwd(DH[:, :W], tp, P, True, TAG_H2, seed=seed, step=step_dev)
    di = ops.mvae_tanh_drop_bwd(DH[:, :W], tp, P, True, TAG_H2, drop_mult=inj)
    assert torch.equal(dp, di)

    # p = 0 and train = 0: no mask; in place over a, and the backward in place over dh
    for p, train in ((0.0, True), (P, False)):
        A2 = A.clone()
        h2, t2 = ops.mvae_tanh_drop_fwd(A2[:, :W], p, train, TAG_H2, seed=seed, step=step_dev, t_out=A2[:, :W],
                                        h_out=A2[:, :W])
        assert h2.data_ptr() == t2.data_ptr() == A2.data_ptr() and torch.equal(A2[:, :W], tp)
        D2 = DH.clone()
        ops.mvae_tanh_drop_bwd(D2[:, :W], tp, p, train, TAG_H2, seed=seed, step=step_dev, da=D2[:, :W])
        want = dh.astype(np.float64) * (1 - tp.cpu().numpy().astype(np.float64) ** 2)
        assert (np.abs(D2[:, :W].cpu().numpy() - want) <= 2 * U * np.abs(want)).all()
    with pytest.raises(ValueError, match="only without a mask"):
        ops.mvae_tanh_drop_fwd(A[:, :W], P, True, TAG_H2, t_out=T[:, :W], h_out=T[:, :W])


# -------------------------------------------------------------------------------------------------------- nll ----
def _nll_case(nb, N):
    if N == 97:
        m = MR.g_small()
        rows = np.array([0], np.int32) if nb == 1 else _rows("small", nb, True)  # nb = 1: the empty row
    elif N == 4101:
        m, rows = MR.g_wide(), np.arange(37, dtype=np.int32)
    else:
        rng = np.random.Generator(np.random.PCG64(N))
        r, c = np.repeat(np.arange(nb), 40), np.concatenate([rng.choice(N, 40, replace=False) for _ in range(nb)])
        m, rows = MR._canonical(r, c, np.ones(len(r)), (nb, N)), np.arange(nb, dtype=np.int32)
    return m, rows


@pytest.mark.parametrize("nb,N", [(1, 97), (88, 97), (37, 4101), (3, 12101)])
def test_nll_against_float64(hip_device, nb, N):
    """lse, recon and the in-place gradient, with lds = N rounded up to 4 plus 4 and NaN in the dead columns; the last
    row holds logits +80 and -80. With d_j = |s_j - mx| and T = ceil(N / 256) + 10 additions per partial sum chain:
      se:    each term carries the subtraction (u d_j, amplified by exp) and expf (2 u): E_se = (2 + max d + T) u
      lse:   E_lse = E_se + 2 u |log se| + u |lse|
      recon: each entry's (s - lse) carries E_lse + u |s - lse|; a chain of ceil(cnt / 256) + 10 fmas and additions
      grad:  gs n p_j carries p's argument error E_lse + u |s_j - lse|, expf 2 u and two products 2 u; gs x_j one
             product; the subtraction u |g_j|; plus 2^-126 gs n where p_j is below the normal range."""
    from hvae import ops
    dev = hip_device
    m, rows = _nll_case(nb, N)
    rng = np.random.Generator(np.random.PCG64(nb + N))
    lds = (N + 3) // 4 * 4 + 4
    s = (rng.standard_normal((nb, N)) * 3).astype(np.float32)
    s[-1, 0], s[-1, N - 1] = 80.0, -80.0
    gs = np.float32(1.0 / nb)
    x = ops.csr_from_scipy(m, dev)
    xb = ops.Csr(x.row_ptr, x.col_idx, x.vals, N, rows=_dev(rows, dev, torch.int32))

    def run():
        S = torch.full((nb, lds), float("nan"), device=dev)
        S[:, :N] = _dev(s, dev)
        lse, recon = ops.mvae_nll(xb, S, float(gs))
        return S, lse, recon

    S, lse, recon = run()
    S2, lse2, recon2 = run()
    assert torch.equal(S[:, :N], S2[:, :N]) and torch.equal(lse, lse2) and torch.equal(recon, recon2)
    assert torch.isnan(S[:, N:]).all() and torch.isfinite(S[:, :N]).all()  # dead columns untouched, nothing spread

    s64 = s.astype(np.float64)
    X = np.asarray(m[rows].todense(), dtype=np.float64)
    mx = s64.max(1, keepdims=True)
    se = np.exp(s64 - mx).sum(1, keepdims=True)
    lse64 = mx + np.log(se)
    n = X.sum(1, keepdims=True)
    recon64 = -(X * (s64 - lse64)).sum(1)
    g64 = float(gs) * (n * np.exp(s64 - lse64) - X)
    T = -(-N // 256) + 10
    E_lse = (2 + np.abs(s64 - mx).max(1, keepdims=True) + T) * U + 2 * U * np.abs(np.log(se)) + U * np.abs(lse64)
    cnt = (X != 0).sum(1)
    bar_recon = (X * (E_lse + U * np.abs(s64 - lse64))).sum(1) \
        + (-(-cnt // 256) + 10) * U * np.abs(X * (s64 - lse64)).sum(1)
    gnp = float(gs) * n * np.exp(s64 - lse64)
    bar_g = gnp * (E_lse + U * np.abs(s64 - lse64) + 4 * U) + U * float(gs) * X + U * np.abs(g64) \
        + 2.0 ** -126 * float(gs) * n
    err_l, err_r = np.abs(lse.cpu().numpy() - lse64[:, 0]), np.abs(recon.cpu().numpy() - recon64)
    err_g = np.abs(S[:, :N].cpu().numpy() - g64)
    print(f"nll nb={nb} N={N}: lse err {err_l.max():.3e} recon err {err_r.max():.3e} grad err {err_g.max():.3e}")
    assert (err_l <= E_lse[:, 0]).all() and (err_r <= bar_recon).all() and (err_g <= bar_g).all()
    empty = np.flatnonzero(cnt == 0)
    if N == 97:
        assert len(empty) == 1  # the empty row: zero gradient, recon 0, a valid lse
        assert (S[int(empty[0]), :N] == 0).all() and float(recon[int(empty[0])]) == 0.0
        assert np.isfinite(float(lse[int(empty[0])]))


# ------------------------------------------------------------------------------------------------- train step ----
def _ragged_batch():
    """G_small's ragged batch: 88 users, among them the empty, the single-item and the 85-item row."""
    m = MR.g_small()
    order = np.concatenate([np.setdiff1d(np.arange(600), [0, 1, 2])[:512], [2, 0, 1],
                            np.setdiff1d(np.arange(600), [0, 1, 2])[512:]]).astype(np.int32)
    assert len(order) == 600 and len(np.unique(order)) == 600
    return m, order


def _draws(rng, nb, N, H, L):
    mk = lambda *s: (rng.random(s) >= P).astype(np.float32) * 2  # noqa: E731
    return mk(nb, N), mk(nb, H), mk(nb, H), rng.standard_normal((nb, L)).astype(np.float32)


def test_one_train_step_against_torch_autograd_in_float64(hip_device):
    """The ragged batch (88 rows) at the served default widths with injected masks and eps: the three loss terms,
    every gradient and every updated parameter within 16 x the noise, where the noise of a tensor is the largest
    distance between the float32 and the float64 run of the torch restatement from the same draws (the rule of the
    LightGCN and SVD fixtures)."""
    from hvae import ops
    from src.ml import multvae as MV
    dev = hip_device
    m, order = _ragged_batch()
    H, L, N = 600, 200, 97
    params = MR.random_params(N, H, L, seed=3)
    rows = order[512:]
    nb = len(rows)
    X = np.asarray(m[rows].todense(), dtype=np.float32)
    in_mask, m1, m2, eps = _draws(np.random.Generator(np.random.PCG64(5)), nb, N, H, L)
    r64, r32 = MR.Model(params, torch.float64), MR.Model(params, torch.float32)
    loss64, g64 = r64.step(X, in_mask, m1, m2, eps)
    loss32, g32 = r32.step(X, in_mask, m1, m2, eps)

    ts = MV.TrainSteps(m, params, dev, seed=0)
    ts.load_epoch(order)
    ts.run(1, inject={"in_mult": _dev(MR.entry_mult(m, rows, in_mask), dev), "m1": _dev(m1, dev),
                      "m2": _dev(m2, dev), "eps": _dev(eps, dev)})
    torch.cuda.synchronize()
    got_loss = ts.loss3.cpu().numpy().astype(np.float64)
    for i, name in enumerate(("total", "recon", "kl")):
        noise = abs(loss32[i] - loss64[i])
        bar = 16 * max(noise, U * abs(loss64[i]))  # never below the rounding of the fp32 result itself
        print(f"step loss {name}: hip {got_loss[i]:.8g} ref {loss64[i]:.8g} err {abs(got_loss[i] - loss64[i]):.3e} "
              f"bar {bar:.3e}")
        assert abs(got_loss[i] - loss64[i]) <= bar
    assert float(ts.total[0]) == pytest.approx(float(got_loss[0]), rel=1e-7) and int(ts.step) == 1

    dW1t = torch.zeros(N, H, device=dev)
    ops.rowgrad_to_dense(ts.rg, dW1t)
    G = ts.G
    grads = {"encoder.0.weight": dW1t.t(), "encoder.0.bias": G["b1"], "encoder.3.weight": G["W2"],
             "encoder.3.bias": G["b2"], "mu_layer.weight": G["Wh"][:L], "mu_layer.bias": G["bh"][:L],
             "logvar_layer.weight": G["Wh"][L:], "logvar_layer.bias": G["bh"][L:], "decoder.0.weight": G["Wd1"],
             "decoder.0.bias": G["bd1"], "decoder.2.weight": G["Wd2"], "decoder.2.bias": G["bd2"]}
    new, p64, p32 = ts.state_dict(), r64.state(), r32.state()
    bad = []
    for k in g64:
        for what, got, w64, w32 in (("grad", grads[k].cpu(), g64[k], g32[k]), ("param", new[k], p64[k], p32[k])):
            noise = float((w32.double() - w64).abs().max())
            err = float((got.double() - w64).abs().max())
            print(f"step {what} {k}: err {err:.3e} noise {noise:.3e}")
            if not err <= 16 * noise:
                bad.append((what, k, err, noise))
    assert not bad, bad
    # items outside the batch: exact zero gradient rows, parameters unchanged by the first step
    absent = np.flatnonzero(np.asarray((m[rows] != 0).sum(0)).ravel() == 0)
    assert len(absent) > 0 and (dW1t[torch.as_tensor(absent, device=dev)] == 0).all()
    assert torch.equal(new["encoder.0.weight"][:, absent], params["encoder.0.weight"][:, absent])


# ------------------------------------------------------------------------------ reproducibility and eval mode ----
def _fit(seed, torch_seed=11, epochs=2, **kw):
    from src.ml.multvae import MultVAERecommender
    torch.manual_seed(torch_seed)
    r = MultVAERecommender(hidden_dim=600, latent_dim=200, epochs=epochs, seed=seed, **kw)
    r.fit(MR.g_small())
    return r


def test_a_second_fit_is_bitwise_equal_and_the_seed_matters(hip_device):
    a, b, c = _fit(0), _fit(0), _fit(1)
    sa, sb, sc = a.state_dict(), b.state_dict(), c.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert not torch.equal(sa["decoder.2.weight"], sc["decoder.2.weight"])
    users = np.arange(600)
    assert torch.equal(a.score_all(users), b.score_all(users))
    assert np.array_equal(a.predict(7), a.score_all(np.array([7]))[0].cpu().numpy()) and a.predict(7).shape == (97,)
    assert int(a.steps.step) == 4 and np.isfinite(a.predict(0)).all()


def test_eval_mode_ignores_the_seeds_and_matches_float64(hip_device):
    """score_all and score_candidates of two models with the same parameters and different seeds are bitwise equal,
    and within 16 x the fp32-against-fp64 noise of the torch restatement's eval-mode logits."""
    from src.ml import multvae as MV
    dev = hip_device
    m = MR.g_small()
    params = MR.random_params(97, 600, 200, seed=4, scale=2.0)
    r = []
    for seed in (1, 2):
        rec = MV.MultVAERecommender(seed=seed)
        rec.device, rec.matrix = dev, m
        rec.steps = MV.TrainSteps(m, params, dev, seed=seed)
        r.append(rec)
    users = np.arange(600)
    s0, s1 = r[0].score_all(users), r[1].score_all(users)
    assert torch.equal(s0, s1)
    X = np.asarray(m.todense(), dtype=np.float32)
    want64, want32 = MR.Model(params, torch.float64).scores(X), MR.Model(params, torch.float32).scores(X)
    noise = np.abs(want32 - want64).max()
    assert np.abs(s0.cpu().numpy() - want64).max() <= 16 * noise
    cand = torch.as_tensor(np.random.Generator(np.random.PCG64(1)).integers(0, 97, (600, 20)), dtype=torch.int32,
                           device=dev)
    sc = r[0].score_candidates(users, cand)
    assert torch.equal(sc, r[1].score_candidates(users, cand))
    assert np.abs(sc.cpu().numpy() - np.take_along_axis(want64, cand.cpu().numpy().astype(np.int64), 1)).max() \
        <= 16 * noise
    sd = r[0].state_dict()
    assert all(torch.equal(sd[k], params[k]) for k in params) and list(sd) == list(params)


# ----------------------------------------------------------------------------------------------- command line ----
def test_main_writes_the_multvae_entry_beside_an_existing_one(hip_device, tmp_path):
    import src.ml.multvae as mv
    from gen import write_planted_artifacts
    data, _ = write_planted_artifacts(tmp_path, dict(n_users=60, n_items=50, d=4, n_clusters=2))
    out = tmp_path / "models" / "figures" / "baseline_results.json"
    out.parent.mkdir(parents=True)
    pop = {"5": {"recall": 0.1, "ndcg": 0.1, "hit_ratio": 0.1}, "training_time_seconds": 0.01}
    out.write_text(json.dumps({"Popularity": pop}))
    np.random.seed(0)
    torch.manual_seed(0)
    with mock.patch.object(sys, "argv", ["multvae", "--data", str(data), "--epochs", "2", "--seed", "3",
                                         "--n-negatives", "20", "--k-values", "5", "10"]):
        mv.main()
    got = json.loads(out.read_text())
    assert list(got) == ["Popularity", "Mult-VAE"] and got["Popularity"] == pop
    assert list(got["Mult-VAE"]) == ["5", "10", "training_time_seconds"]
    for k in ("5", "10"):
        assert set(got["Mult-VAE"][k]) == {"recall", "ndcg", "hit_ratio"}
        assert all(0.0 <= v <= 1.0 for v in got["Mult-VAE"][k].values())
    assert got["Mult-VAE"]["10"]["hit_ratio"] >= got["Mult-VAE"]["5"]["hit_ratio"]


# ------------------------------------------------------------------------------- the reference's trajectory ----
def test_the_references_trajectory_after_one_and_three_epochs(hip_device):
    """The reference's own fit on g_small (tests/golden/make_multvae_fixture.py) followed on the device: the initial
    parameters and epoch orders from torch's generator, the masks from the device's own Philox streams (the fixture's
    masks are philox_ref's for the same seed and steps, and the kernels are held to philox_ref bit for bit above),
    eps injected (philox_ref.normal32, as the fixture drew it). Per-step losses and the eval-mode scores of every
    user after 1 and 3 epochs within the fixture's bars (16 x the reference's own fp32-against-fp64 noise); every
    rank of the project's evaluation inside the bracket the reference's scores allow at that bar, as is the
    reference's own rank."""
    from src.ml import baseline as B
    from src.ml import multvae as MV
    dev = hip_device
    fx, meta, m = MR.fixture(), MR.fixture_meta(), MR.g_small()
    N, L = m.shape[1], MR.LATENT
    torch.manual_seed(MR.SEED_TORCH)
    params = MV.init_params(N, MR.HIDDEN, L)
    assert MR.params_digest(params) == meta["init_digest"]
    rec = MV.MultVAERecommender(MR.HIDDEN, L, seed=MR.SEED_DEV)
    rec.device, rec.matrix = dev, m
    rec.steps = ts = MV.TrainSteps(m, params, dev, seed=MR.SEED_DEV)
    users, tests = MR.fixture_tests(m)
    losses, scores, step = [], {}, 0
    for ep in range(MR.FIX_EPOCHS[-1]):
        order = MV.epoch_order(m.shape[0])
        assert np.array_equal(order, fx["orders"][ep])
        ts.load_epoch(order)
        for k in range(ts.n_batches):
            nb = min(MR.BATCH, len(order) - k * MR.BATCH)
            ts.run(k, inject={"eps": _dev(PR.normal32(MR.SEED_DEV, step, nb, L), dev)})
            losses.append(ts.loss3[:1].clone())
            step += 1
        if ep + 1 in MR.FIX_EPOCHS:
            scores[ep + 1] = rec.score_all(users).cpu().numpy()
    losses = torch.cat(losses).cpu().numpy()
    err = np.abs(losses.astype(np.float64) - fx["losses"])
    print(f"trajectory losses {losses.tolist()} err {err.max():.3e} bar {meta['bar']['losses']:.3e}")
    assert (err <= meta["bar"]["losses"]).all()
    for e in MR.FIX_EPOCHS:
        err = np.abs(scores[e].astype(np.float64) - fx[f"scores_e{e}"]).max()
        print(f"trajectory scores after {e} epochs: err {err:.3e} bar {meta['bar'][f'scores_e{e}']:.3e}")
        assert err <= meta["bar"][f"scores_e{e}"]
    cand = np.asarray(m.todense()) == 0  # fewer than 99 unseen items: every unseen item is a candidate
    lo, hi = MR.bracket(fx["scores_e3"].astype(np.float64), cand, tests, meta["bar"]["scores_e3"])
    np.random.seed(0)
    ranks = B.evaluate_ranks(rec, m, users, tests, [10], 99)
    assert ((ranks >= lo) & (ranks <= hi)).all() and ((fx["ranks"] >= lo) & (fx["ranks"] <= hi)).all()


# ------------------------------------------------------------------------- quality under the device's masks ----
def test_quality_under_the_devices_own_masks_matches_the_references(hip_device, tmp_path):
    """NDCG@10 (99 negatives) of 8 seeded fits on the planted set of the fixture's quality record (one batch per
    epoch), with the device's own Philox masks and eps, against the reference's 8 fits with torch's dropout: the two
    sample means within 3 standard errors of their difference, computed from the two samples."""
    import pandas as pd
    from gen import write_planted_artifacts
    from src.ml import multvae as MV
    from src.ml.baseline import _build_input_matrix, evaluate_model
    from src.ml.train import load_training_data
    q = MR.fixture_meta()["quality"]
    data, _ = write_planted_artifacts(tmp_path, q["cfg"])
    full, train_df, val_df, maps = load_training_data(str(data))
    matrix, _ = _build_input_matrix(train_df, val_df, maps["user_to_idx"], maps["item_to_idx"], full.shape)
    assert matrix.shape[0] <= MV.BATCH_SIZE
    test_df = pd.read_csv(data / "test.csv")
    got = []
    for seed in q["seeds"]:
        torch.manual_seed(seed)
        np.random.seed(seed)
        rec = MV.MultVAERecommender(epochs=q["epochs"], seed=seed, device=hip_device)
        rec.fit(matrix)
        res = evaluate_model(rec, "Mult-VAE", matrix, test_df, maps["user_to_idx"], maps["item_to_idx"], [q["k"]],
                             q["n_negatives"])
        got.append(res[q["k"]]["ndcg"])
    ref = np.array(q["ndcg"])
    got = np.array(got)
    se = np.sqrt(got.var(ddof=1) / len(got) + ref.var(ddof=1) / len(ref))
    print(f"quality: device {got.mean():.4f} +- {got.std(ddof=1):.4f}  reference {ref.mean():.4f} +- "
          f"{ref.std(ddof=1):.4f}  difference {got.mean() - ref.mean():+.4f}  3 se {3 * se:.4f}")
    assert abs(got.mean() - ref.mean()) <= 3 * se
