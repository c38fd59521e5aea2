"""Generated dropout masks and reparameterisation noise against the numpy restatement of the random stream.

Production training injects nothing: every mask and all noise come from the Philox4x32-10 of csrc/hvae_common.h as a
function of (seed, *step_dev, tag, element index), and every backward kernel draws its mask again. The other GPU
tests inject masks and noise (drop_mult / eps_in / ext=) or compare one kernel with another, so a backward kernel that
rebuilt other bits than its forward used would pass them all. Here every drawing kernel, the module API and the fused
trainer must equal tests/philox_ref.py (pinned on the CPU by tests/test_philox_reference_cpu.py):

  (a) forward masks, bit for bit, recovered exactly by making the pre-dropout activation the constant GELU(1);
  (b) the noise, to a bar derived from the float32 / float64 distance of the restatement itself;
  (c) every backward kernel in generated mode == the same kernel with the restated multipliers injected (bitwise),
      whose injected arm is anchored to float64;
  (d) steps and seeds give separate streams on the device;
  (e) loss.backward() of the module API in train mode against the float64 oracle fed the restated masks and noise;
  (f) the fused trainer with nothing injected == the fused trainer with the restated masks injected (bitwise), over
      three steps, eager and graph-replayed.

Every seed has a high word ((5 << 40) + 1234 and the like) and step_dev holds 5 unless a case says otherwise.
"""
import ctypes as C
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from gen import synth_csr, synth_embeddings
from oracle import ref_cpu as R

sys.path.insert(0, str(Path(__file__).resolve().parent))
import philox_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = (5 << 40) + 1234
STEP = 5
PD = 0.3
GELU1 = float(np.float32(0.5 * (1.0 + math.erf(1.0 / math.sqrt(2.0)))))


@pytest.fixture(scope="module")
def ops(hip_device):
    from hvae import ops
    return ops


@pytest.fixture()
def step5(hip_device):
    return torch.full((1,), STEP, dtype=torch.int64, device=hip_device)


def _maxrel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / max(b.abs().max().item(), 1e-30))


def _t(a, dev=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dev is None else t.to(dev)


def _check_const_mask(out, keep_ref, p=PD):
    """out = GELU(1) * dropout multiplier: its zero pattern is the mask (GELU(1) = 0.84 cannot underflow), and the
    survivors carry 1 / (1 - p)."""
    assert torch.isfinite(out).all()
    assert torch.equal((out != 0).cpu(), _t(keep_ref))
    kept = out[out != 0].double().cpu()
    if kept.numel():
        want = GELU1 * float(P.scale(p))
        assert float((kept / want - 1).abs().max()) < 1e-6


def _rand(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


# ============================================================ (a) forward masks ==
@pytest.mark.parametrize("H", [4, 64, 600, 1028])
def test_encoder_fwd_mask(ops, hip_device, step5, H):
    """hvae_encoder_fwd (NV = 1, 1, 4, 8): the generated mask is keep(seed, step, 0x100, row * H + col)."""
    X = synth_csr(37, 500, lam=6.0, seed=1)
    xd = ops.csr_from_scipy(X, hip_device)
    g = torch.Generator().manual_seed(H)
    w1t, b1 = _rand(g, 500, H, scale=0.05).to(hip_device), _rand(g, H).to(hip_device)
    zero, one = torch.zeros(H, device=hip_device), torch.ones(H, device=hip_device)
    h, _, _ = ops.encoder_fwd(xd, w1t, b1, zero, one, PD, True, SEED, step=step5)
    _check_const_mask(h, P.keep(SEED, STEP, P.TAG_ENC_DROP, 37, H, PD))
    if H == 64:  # step_dev = NULL is step 0
        h0, _, _ = ops.encoder_fwd(xd, w1t, b1, zero, one, PD, True, SEED, step=None)
        _check_const_mask(h0, P.keep(SEED, 0, P.TAG_ENC_DROP, 37, H, PD))
        assert not torch.equal(h0 != 0, h != 0)


def test_encoder_fwd_mask_is_indexed_by_batch_position(ops, hip_device, step5):
    """The batch as a permuted subset of a larger matrix's rows (`rows` read from `rows_offset` on): the mask follows
    the position in the batch, not the matrix row."""
    H, nb = 64, 37
    X = synth_csr(100, 500, lam=6.0, seed=2)
    full = ops.csr_from_scipy(X, hip_device)
    sel = np.random.default_rng(3).permutation(100)[:nb].astype(np.int32)
    assert not np.array_equal(sel, np.arange(nb))
    rows = _t(np.concatenate([np.full(5, 99, np.int32), sel]), hip_device)
    off = torch.full((1,), 5, dtype=torch.int64, device=hip_device)
    xd = ops.Csr(full.row_ptr, full.col_idx, full.vals, 500, rows=rows, nb=nb, rows_offset=off)
    g = torch.Generator().manual_seed(4)
    w1t, b1 = _rand(g, 500, H, scale=0.05).to(hip_device), _rand(g, H).to(hip_device)
    zero, one = torch.zeros(H, device=hip_device), torch.ones(H, device=hip_device)
    h, _, _ = ops.encoder_fwd(xd, w1t, b1, zero, one, PD, True, SEED, step=step5)
    _check_const_mask(h, P.keep(SEED, STEP, P.TAG_ENC_DROP, nb, H, PD))
    # and the rows really are the selected ones: with the real LayerNorm and no dropout, h is that of the subset
    hs, _, _ = ops.encoder_fwd(xd, w1t, b1, one, zero, PD, False, SEED, step=step5)
    hd, _, _ = ops.encoder_fwd(ops.csr_from_scipy(X[sel], hip_device), w1t, b1, one, zero, PD, False, SEED, step=step5)
    assert torch.equal(hs, hd)


@pytest.mark.parametrize("nb", [1, 37])
@pytest.mark.parametrize("H", [4, 64, 600, 1028])
def test_ln_gelu_drop_fwd_mask(ops, hip_device, step5, H, nb):
    """hvae_ln_gelu_drop_fwd: layer k draws from tag 0x100 + k, and the layers' masks differ."""
    g = torch.Generator().manual_seed(H + nb)
    a = _rand(g, nb, H).to(hip_device)
    zero, one = torch.zeros(H, device=hip_device), torch.ones(H, device=hip_device)
    masks = {}
    for layer in (0, 1, 3):
        h, _, _ = ops.ln_gelu_drop_fwd(a, zero, one, PD, True, SEED, layer, step=step5)
        _check_const_mask(h, P.keep(SEED, STEP, P.TAG_ENC_DROP + layer, nb, H, PD))
        masks[layer] = h != 0
    if nb * H >= 64:  # (4 elements can coincide by chance)
        assert not torch.equal(masks[0], masks[1]) and not torch.equal(masks[1], masks[3])
        assert not torch.equal(masks[0], masks[3])


# (M, N, K, split-K planned, ldc - N, kernel, which epi_apply call of gemm_finish the shape reaches)
GEMM_SHAPES = [
    (50, 70, 33, False, 2, "register-staged", "unsplit (the first epi_apply of gemm_finish), ragged tiles, ldc > N"),
    (128, 96, 64, False, 0, "LDS-DMA 32 x 32", "unsplit, whole tiles"),
    (64, 128, 1024, True, 0, "LDS-DMA 32 x 32", "split-K over whole tiles (fragment-order slab, the second call)"),
    (64, 128, 1000, True, 0, "register-staged (K % 32 != 0)", "split-K over whole tiles (the second call)"),
    (50, 70, 1000, True, 0, "register-staged", "split-K over ragged tiles (element-order slab, the third call; "
                                               "the LDS-DMA kernel takes whole tiles only)"),
]
GEMM_IDS = [f"{m}x{n}x{k}" for m, n, k, *_ in GEMM_SHAPES]


def _assert_plan(M, N, K, split):
    """The planner still splits (or does not split) this shape, so the case still reaches the site it names."""
    from hvae._lib import lib
    assert (int(lib().hvae_gemm_f32_workspace(M, N, K)) > 0) == split


def _strided(M, N, pad, dev):
    """An [M, N] view of an [M, N + pad] buffer (ldc = N + pad), NaN outside the view."""
    return torch.full((M, N + pad), float("nan"), device=dev)[:, :N]


@pytest.mark.parametrize("M,N,K,split,pad,kernel,site", GEMM_SHAPES, ids=GEMM_IDS)
def test_gemm_bias_gelu_drop_mask(ops, hip_device, step5, M, N, K, split, pad, kernel, site):
    """HVAE_EPI_BIAS_GELU_DROP with A = 0 and bias = 1: the mask is keep(seed, step, tag, row * N + col) -- N, not
    ldc -- at each of the three places gemm_finish applies the epilogue, in both GEMM kernels."""
    from hvae import _lib
    _assert_plan(M, N, K, split)
    g = torch.Generator().manual_seed(M + K)
    A, W = torch.zeros(M, K, device=hip_device), _rand(g, N, K).to(hip_device)
    bias = torch.ones(N, device=hip_device)
    out, pre = _strided(M, N, pad, hip_device), _strided(M, N, pad, hip_device)
    epi = ops.epilogue(_lib.EPI_BIAS_GELU_DROP, bias=bias, pre_out=pre, p_drop=PD, seed=SEED, step=step5,
                       tag=_lib.TAG_PROJ_DROP, train=True)
    ops.gemm(A, W.t(), out=out, epi=epi)
    assert torch.equal(pre, torch.ones_like(pre))
    _check_const_mask(out, P.keep(SEED, STEP, P.TAG_PROJ_DROP, M, N, PD))


def _mlp_tensors(B, H, L, D, dev, seed, const_q=False):
    g = torch.Generator().manual_seed(seed)
    t = dict(h=_rand(g, B, H), Wh=_rand(g, 2 * L, H, scale=H ** -0.5), bh=_rand(g, 2 * L, scale=0.1),
             Wa=_rand(g, D, L, scale=L ** -0.5), ba=_rand(g, D, scale=0.1),
             Wb=_rand(g, D, D, scale=D ** -0.5), bb=_rand(g, D, scale=0.1), dU=_rand(g, B, D, scale=0.01))
    if const_q:  # p1 = 1 in every unit
        t["Wa"], t["ba"] = torch.zeros(D, L), torch.ones(D)
    d = {k: v.to(dev) for k, v in t.items()}
    f = lambda *s: torch.full(s, float("nan"), device=dev)
    out = dict(heads=f(B, 2 * L), z=f(B, L), eps=f(B, L), kl=f(B), p1=f(B, D), q=f(B, D), u=f(B, D), dp1=f(B, D),
               dheads=f(B, 2 * L), dh=f(B, H))
    return d, out


def _mlp_args(B, H, L, D, d, out, train=True, p=PD, mult=None, eps_in=None, step=None, seed=SEED):
    from hvae import _lib
    from hvae._lib import ptr
    return _lib.MlpRows(
        nb=B, H=H, L=L, D=D, W_heads=ptr(d["Wh"]), b_heads=ptr(d["bh"]), W_a=ptr(d["Wa"]), b_a=ptr(d["ba"]),
        W_b=ptr(d["Wb"]), b_b=ptr(d["bb"]), train=int(train), p_drop=p, drop_mult=ptr(mult), eps_in=ptr(eps_in),
        seed=seed, step_dev=ptr(step), h=ptr(d["h"]), heads=ptr(out["heads"]), z=ptr(out["z"]), eps=ptr(out["eps"]),
        kl_rows=ptr(out["kl"]), p1=ptr(out["p1"]), q=ptr(out["q"]), u=ptr(out["u"]), dU=ptr(d["dU"]), ks=0.2 / B,
        ks_dev=None, dp1=ptr(out["dp1"]), dheads=ptr(out["dheads"]), dh=ptr(out["dh"]))


def _mlp_fwd(a):
    from hvae._lib import check, lib
    check(lib().hvae_mlp_fwd_rows(C.byref(a), None), "mlp_fwd_rows")


def _mlp_bwd(a):
    from hvae._lib import check, lib
    check(lib().hvae_mlp_bwd_rows(C.byref(a), None), "mlp_bwd_rows")


@pytest.mark.parametrize("B,H,L,D", [(1, 512, 128, 384), (33, 96, 32, 64), (129, 512, 128, 384)])
def test_mlp_rows_q_mask(hip_device, step5, B, H, L, D):
    """hvae_mlp_fwd_rows (1 and 2 rows per block): q's mask at tag 0x200 with W_a = 0, b_a = 1."""
    d, out = _mlp_tensors(B, H, L, D, hip_device, B + D, const_q=True)
    _mlp_fwd(_mlp_args(B, H, L, D, d, out, step=step5))
    assert torch.equal(out["p1"], torch.ones_like(out["p1"]))
    _check_const_mask(out["q"], P.keep(SEED, STEP, P.TAG_PROJ_DROP, B, D, PD))


def test_mlp_rows_fused_encoder_mask(ops, hip_device, step5):
    """The first encoder layer inside hvae_mlp_fwd_rows' launch (enc_x, H <= 512): h's mask at tag 0x100 and q's at
    0x200 from the same launch."""
    from hvae._lib import ptr
    B, H, L, D = 33, 96, 32, 64
    d, out = _mlp_tensors(B, H, L, D, hip_device, 7, const_q=True)
    xd = ops.csr_from_scipy(synth_csr(B, 500, lam=6.0, seed=5), hip_device)
    g = torch.Generator().manual_seed(8)
    w1t, b1 = _rand(g, 500, H, scale=0.05).to(hip_device), _rand(g, H).to(hip_device)
    zero, one = torch.zeros(H, device=hip_device), torch.ones(H, device=hip_device)
    h = torch.full((B, H), float("nan"), device=hip_device)
    xhat, rstd = torch.empty(B, H, device=hip_device), torch.empty(B, device=hip_device)
    a = _mlp_args(B, H, L, D, d, out, step=step5)
    a.h, a.enc_x, a.w1t, a.b1, a.ln_w, a.ln_b = ptr(h), C.pointer(xd.struct), ptr(w1t), ptr(b1), ptr(zero), ptr(one)
    a.xhat, a.rstd = ptr(xhat), ptr(rstd)
    _mlp_fwd(a)
    _check_const_mask(h, P.keep(SEED, STEP, P.TAG_ENC_DROP, B, H, PD))
    _check_const_mask(out["q"], P.keep(SEED, STEP, P.TAG_PROJ_DROP, B, D, PD))


@pytest.mark.parametrize("family", ["layernorm", "gemm", "mlp_rows"])
def test_dropout_edges(ops, hip_device, step5, family):
    """One kernel of each family: train = 0 is the identity at any p, p = 0 with train = 1 too, and p = 1 gives
    zeros without a NaN (the launchers set the survivors' scale to 0, not 1 / 0)."""
    from hvae import _lib
    g = torch.Generator().manual_seed(21)
    if family == "layernorm":
        a, lw = _rand(g, 37, 64).to(hip_device), (1 + 0.1 * _rand(g, 64)).to(hip_device)
        lb = _rand(g, 64).to(hip_device)
        run = lambda p, train: ops.ln_gelu_drop_fwd(a, lw, lb, p, train, SEED, 1, step=step5)[0]
    elif family == "gemm":
        A, W, b = (_rand(g, 50, 33, scale=33 ** -0.5).to(hip_device), _rand(g, 70, 33).to(hip_device),
                   _rand(g, 70, scale=0.1).to(hip_device))  # pre-activations ~ N(0, 1)

        def run(p, train):
            pre = torch.empty(50, 70, device=hip_device)
            return ops.gemm(A, W.t(), epi=ops.epilogue(_lib.EPI_BIAS_GELU_DROP, bias=b, pre_out=pre, p_drop=p,
                                                       seed=SEED, step=step5, tag=_lib.TAG_PROJ_DROP, train=train))
    else:
        d, out = _mlp_tensors(33, 96, 32, 64, hip_device, 22)

        def run(p, train):
            _mlp_fwd(_mlp_args(33, 96, 32, 64, d, out, train=train, p=p, step=step5,
                               eps_in=torch.zeros(33, 32, device=hip_device)))
            return out["q"].clone()
    ident = run(PD, False)
    # the identity is not a trivial one (float32 GELU is -0 below about -5.5, which N(0, 1) inputs all but never reach)
    assert torch.isfinite(ident).all() and float((ident != 0).float().mean()) > 0.99
    assert torch.equal(run(0.0, True), ident)
    assert torch.equal(run(0.9, False), ident) and torch.equal(run(1.0, False), ident)
    dropped = run(1.0, True)
    assert torch.equal(dropped, torch.zeros_like(dropped))
    if family == "mlp_rows":  # u = q W_b^T + b_b stays finite behind the all-zero q
        assert torch.equal(out["u"], d["bb"].expand_as(out["u"]))


# ===================================================================== (b) noise ==
def _eps_ok(eps, seed, step, nb, L, label):
    """|eps - normal| <= 8 x max |normal32 - normal| over the same indices; prints the measured ratio to that max."""
    ref = P.normal(seed, step, nb, L)
    dev32 = float(np.abs(P.normal32(seed, step, nb, L).astype(np.float64) - ref).max())
    got = float(np.abs(eps.double().cpu().numpy() - ref).max())
    print(f"eps {label} ({nb} x {L}): max |gpu - float64| = {got:.3e}, max |numpy float32 - float64| = {dev32:.3e}, "
          f"ratio {got / dev32:.2f} (bar 8)")
    assert torch.isfinite(eps).all()
    assert got <= 8.0 * dev32


@pytest.mark.parametrize("nb,L", [(33, 64), (129, 128)])
def test_noise_equals_restatement(ops, hip_device, step5, nb, L):
    """eps of hvae_reparam_kl_fwd and of hvae_mlp_fwd_rows: N(0, 1) draws of the restatement (tag 0x300, index
    row * L + col), bitwise equal to each other, and z = mu + eps exp(0.5 logvar) from the kernel's own eps."""
    H, D = 96, 64
    d, out = _mlp_tensors(nb, H, L, D, hip_device, nb + L)
    _mlp_fwd(_mlp_args(nb, H, L, D, d, out, step=step5))
    mu, lv = out["heads"][:, :L], out["heads"][:, L:]
    z, eps, _ = ops.reparam_kl_fwd(mu, lv, True, SEED, step=step5)
    _eps_ok(eps, SEED, STEP, nb, L, "hvae_reparam_kl_fwd")
    _eps_ok(out["eps"], SEED, STEP, nb, L, "hvae_mlp_fwd_rows")
    assert torch.equal(eps, out["eps"])
    for zz, ee in ((z, eps), (out["z"], out["eps"])):
        assert _maxrel(zz, mu.double() + ee.double() * torch.exp(0.5 * lv.double())) < 1e-6
    z0, eps0, _ = ops.reparam_kl_fwd(mu, lv, True, SEED, step=None)  # step_dev = NULL: step 0
    _eps_ok(eps0, SEED, 0, nb, L, "hvae_reparam_kl_fwd, step_dev NULL")


# ============================================= (c) backward regenerates the forward ==
@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("nb,H", [(37, 64), (261, 128), (2051, 64), (37, 1028)])
def test_ln_bwd_generated_equals_injected(ops, hip_device, step5, nb, H, layer):
    """hvae_ln_gelu_drop_bwd: the ticket path (nb = 37), the two-launch reduction (nb = 261: 66 partials), four rows
    per wave (nb = 2051) and NV = 8 (H = 1028). Generated mode == the restated multipliers injected, bitwise, in
    the forward and in all four backward outputs; the injected arm against float64 autograd at the bars of
    test_encoder_fwd_bwd."""
    g = torch.Generator().manual_seed(nb + H)
    a, dh = _rand(g, nb, H), _rand(g, nb, H)
    lw, lb = 1 + 0.1 * _rand(g, H), _rand(g, H)
    dv = lambda t: t.to(hip_device)
    mult = P.mult(SEED, STEP, P.TAG_ENC_DROP + layer, nb, H, PD)
    md = _t(mult, hip_device)
    hg, xhat, rstd = ops.ln_gelu_drop_fwd(dv(a), dv(lw), dv(lb), PD, True, SEED, layer, step=step5)
    hi, xhat_i, rstd_i = ops.ln_gelu_drop_fwd(dv(a), dv(lw), dv(lb), PD, True, 0, layer, drop_mult=md)
    assert torch.equal(hg, hi) and torch.equal(xhat, xhat_i) and torch.equal(rstd, rstd_i)
    gen = ops.ln_gelu_drop_bwd(dv(dh), xhat, rstd, dv(lw), dv(lb), PD, True, SEED, layer, step=step5, want_dbias=True)
    gen = [t.clone() for t in gen]  # (the next call reuses the workspace, not the outputs; cloned to be plain)
    inj = ops.ln_gelu_drop_bwd(dv(dh), xhat, rstd, dv(lw), dv(lb), PD, True, 0, layer, drop_mult=md, want_dbias=True)
    for name, x, y in zip(("da", "d_ln_w", "d_ln_b", "d_bias"), gen, inj):
        assert torch.equal(x, y), name
    a64 = a.double().requires_grad_(True)
    lw64, lb64 = lw.double().requires_grad_(True), lb.double().requires_grad_(True)
    y = R.gelu(R.layer_norm(a64, lw64, lb64)) * _t(mult).double()
    assert _maxrel(hi, y) < 2e-5
    (y * dh.double()).sum().backward()
    da, dlw, dlb, dbias = inj
    assert _maxrel(da, a64.grad) < 5e-5 and _maxrel(dbias, a64.grad.sum(0)) < 5e-5
    assert _maxrel(dlw, lw64.grad) < 5e-5 and _maxrel(dlb, lb64.grad) < 5e-5


@pytest.mark.parametrize("M,N,K,split,pad,kernel,site", GEMM_SHAPES, ids=GEMM_IDS)
def test_gemm_bwd_epilogues_generated_equal_injected(ops, hip_device, step5, M, N, K, split, pad, kernel, site):
    """HVAE_EPI_GELU_DROP_BWD and HVAE_EPI_DROP_BWD at the shapes of the forward case: generated == injected,
    bitwise; DROP_BWD's injected arm, C = (G W) * mult, against float64."""
    from hvae import _lib
    _assert_plan(M, N, K, split)
    g = torch.Generator().manual_seed(M * 3 + K)
    G, W, pre = _rand(g, M, K), _rand(g, K, N), _rand(g, M, N)
    Gd, Wd = G.to(hip_device), W.to(hip_device)
    pre_d = _strided(M, N, pad, hip_device)
    pre_d.copy_(pre)
    mult = P.mult(SEED, STEP, P.TAG_PROJ_DROP, M, N, PD)
    md = _t(mult, hip_device)
    outs = {}
    for kind in (_lib.EPI_GELU_DROP_BWD, _lib.EPI_DROP_BWD):
        for arm in ("generated", "injected"):
            kw = (dict(seed=SEED, step=step5, tag=_lib.TAG_PROJ_DROP) if arm == "generated"
                  else dict(drop_mult=md, seed=0, tag=0))
            out = _strided(M, N, pad, hip_device)
            ops.gemm(Gd, Wd, out=out, epi=ops.epilogue(kind, pre_in=pre_d, p_drop=PD, train=True, **kw))
            outs[kind, arm] = out
        assert torch.equal(outs[kind, "generated"], outs[kind, "injected"]), kind
    acc = G.double() @ W.double()
    m64 = _t(mult).double()
    assert _maxrel(outs[_lib.EPI_DROP_BWD, "injected"], acc * m64) < 1e-5
    x = pre.double().requires_grad_(True)
    (R.gelu(x) * m64 * acc).sum().backward()
    assert _maxrel(outs[_lib.EPI_GELU_DROP_BWD, "injected"], x.grad) < 1e-5
    # train = 0: no mask at all
    out0 = ops.gemm(Gd, Wd, epi=ops.epilogue(_lib.EPI_DROP_BWD, p_drop=PD, seed=SEED, step=step5,
                                             tag=_lib.TAG_PROJ_DROP, train=False))
    assert _maxrel(out0, acc) < 1e-5


@pytest.mark.parametrize("B,H,L,D,enc_layer", [(1, 512, 128, 384, 0), (33, 96, 32, 64, 1), (129, 512, 128, 384, 0)])
def test_mlp_rows_generated_equals_injected(ops, hip_device, step5, B, H, L, D, enc_layer):
    """hvae_mlp_fwd_rows / hvae_mlp_bwd_rows on random inputs: nothing injected == the restated projection mask and
    the forward's own eps injected, bitwise (heads, z, q, u; dp1, dheads, dh), and with the last hidden layer's
    LayerNorm backward fused (ln_w set) also da and the three column sums at tag 0x100 + enc_layer."""
    from hvae._lib import lib, ptr
    g = torch.Generator().manual_seed(B)
    xhat = _rand(g, B, H).to(hip_device)
    rstd = (torch.rand(B, generator=g) + 0.5).to(hip_device)
    ln_w, ln_b = (1 + 0.2 * _rand(g, H)).to(hip_device), _rand(g, H, scale=0.1).to(hip_device)
    md = _t(P.mult(SEED, STEP, P.TAG_PROJ_DROP, B, D, PD), hip_device)
    emd = _t(P.mult(SEED, STEP, P.TAG_ENC_DROP + enc_layer, B, H, PD), hip_device)
    res = {}
    eps_gen = None
    for arm in ("generated", "injected"):
        d, out = _mlp_tensors(B, H, L, D, hip_device, B + H)
        if arm == "generated":
            a = _mlp_args(B, H, L, D, d, out, step=step5)
        else:
            a = _mlp_args(B, H, L, D, d, out, mult=md, eps_in=eps_gen, seed=0)
        _mlp_fwd(a)
        eps_gen = out["eps"].clone() if arm == "generated" else eps_gen
        _mlp_bwd(a)
        plain = {k: out[k].clone() for k in ("dp1", "dheads", "dh")}
        f = lambda *s: torch.full(s, float("nan"), device=hip_device)
        da, dw, db, dbias = f(B, H), f(H), f(H), f(H)
        ws = torch.empty(max(int(lib().hvae_mlp_bwd_rows_workspace(B, H)), 256), dtype=torch.uint8, device=hip_device)
        a.ln_w, a.ln_b, a.xhat, a.rstd, a.enc_layer = ptr(ln_w), ptr(ln_b), ptr(xhat), ptr(rstd), enc_layer
        a.enc_drop_mult = ptr(emd) if arm == "injected" else None
        a.da, a.d_ln_w, a.d_ln_b, a.d_bias = ptr(da), ptr(dw), ptr(db), ptr(dbias)
        a.ws, a.ws_bytes = ptr(ws), ws.numel()
        _mlp_bwd(a)
        res[arm] = dict({k: out[k].clone() for k in ("heads", "z", "eps", "kl", "p1", "q", "u", "dp1", "dheads", "dh")},
                        da=da, d_ln_w=dw, d_ln_b=db, d_bias=dbias, **{"plain_" + k: v for k, v in plain.items()})
    for k, v in res["generated"].items():
        assert torch.isfinite(v).all(), k
        assert torch.equal(v, res["injected"][k]), k
    # and the fused LayerNorm backward's da is hvae_ln_gelu_drop_bwd's on the restated mask (anchored to float64 in
    # test_ln_bwd_generated_equals_injected)
    da2, *_ = ops.ln_gelu_drop_bwd(res["injected"]["dh"], xhat, rstd, ln_w, ln_b, PD, True, 0, enc_layer, drop_mult=emd)
    assert torch.equal(res["generated"]["da"], da2)


# ======================================================== (d) stream separation ==
def test_steps_and_seeds_are_separate_streams(ops, hip_device):
    """Steps 5 and 6 of one kernel give independent masks (agreement p^2 + (1 - p)^2 = 0.58 at p = 0.3), each its
    restatement; so does a seed that differs only in bit 40."""
    nb, H = 37, 600
    a = _rand(torch.Generator().manual_seed(9), nb, H).to(hip_device)
    zero, one = torch.zeros(H, device=hip_device), torch.ones(H, device=hip_device)
    step = torch.full((1,), STEP, dtype=torch.int64, device=hip_device)
    m = {}
    for seed, s in ((SEED, STEP), (SEED, STEP + 1), (SEED ^ (1 << 40), STEP)):
        step.fill_(s)
        h, _, _ = ops.ln_gelu_drop_fwd(a, zero, one, PD, True, seed, 1, step=step)
        _check_const_mask(h, P.keep(seed, s, P.TAG_ENC_DROP + 1, nb, H, PD))
        m[seed, s] = h != 0
    base = m[SEED, STEP]
    for other in (m[SEED, STEP + 1], m[SEED ^ (1 << 40), STEP]):
        agree = float((base == other).float().mean())
        assert abs(agree - 0.58) < 0.03, agree


# ================================================= (4) reparameterisation backward ==
@pytest.mark.parametrize("form", ["kl_only", "eval", "eval_heads_layout"])
def test_reparam_kl_bwd_module_forms(ops, hip_device, form):
    """hvae_reparam_kl_bwd as the module API calls it: dz = NULL (the KL term alone, VaeLossFn.backward) and
    train = 0 (z = mu), the latter also writing into a heads-shaped [B, 2L] gradient (ld_out = 2L != L)."""
    g = torch.Generator().manual_seed(6)
    B, L, beta = 33, 64, 0.2
    heads = _rand(g, B, 2 * L)
    dz = _rand(g, B, L)
    hd = heads.to(hip_device)
    mu, lv = hd[:, :L], hd[:, L:]
    m_, l_ = heads[:, :L].double().requires_grad_(True), heads[:, L:].double().requires_grad_(True)
    klr = -0.5 * (1 + l_ - m_ ** 2 - l_.exp()).sum(1)
    if form == "kl_only":
        (beta * klr.sum() / B).backward()
        dmu, dlv = ops.reparam_kl_bwd(None, mu, lv, None, beta / B, False)
    else:
        ((m_ * dz.double()).sum() + beta * klr.sum() / B).backward()
        if form == "eval":
            dmu, dlv = ops.reparam_kl_bwd(dz.to(hip_device), mu, lv, None, beta / B, False)
        else:
            dheads = torch.full((B, 2 * L), float("nan"), device=hip_device)
            dmu, dlv = ops.reparam_kl_bwd(dz.to(hip_device), mu, lv, None, beta / B, False, dmu=dheads[:, :L],
                                          dlv=dheads[:, L:])
            assert torch.isfinite(dheads).all()
    assert _maxrel(dmu, m_.grad) < 1e-5 and _maxrel(dlv, l_.grad) < 1e-5


@pytest.mark.parametrize("train,scale_dev", [(False, False), (True, True), (False, True)])
def test_reparam_bwd_epilogue_equals_kernel(ops, hip_device, train, scale_dev):
    """HVAE_EPI_REPARAM_BWD with train = 0 and with the KL scale read from the device (aux_scale_dev) writes what
    hvae_reparam_kl_bwd writes from the same dz, bitwise."""
    from hvae import _lib
    g = torch.Generator().manual_seed(7)
    B, L, ks = 33, 64, 0.2 / 33
    hd = _rand(g, B, 2 * L).to(hip_device)
    eps = _rand(g, B, L).to(hip_device)
    Gm, W = _rand(g, B, 96).to(hip_device), _rand(g, 96, L).to(hip_device)
    ks_dev = torch.full((1,), ks, device=hip_device) if scale_dev else None
    host_ks = 123.0 if scale_dev else ks  # the device scalar must win
    dz = ops.gemm(Gm, W)
    dmu, dlv = ops.reparam_kl_bwd(dz, hd[:, :L], hd[:, L:], eps if train else None, host_ks, train,
                                  kl_scale_dev=ks_dev)
    dheads = torch.full((B, 2 * L), float("nan"), device=hip_device)
    epi = ops.epilogue(_lib.EPI_REPARAM_BWD, pre_in=hd, train=train, aux=eps if train else None, aux_scale=host_ks,
                       aux_scale_dev=ks_dev)
    ops.gemm(Gm, W, out=dheads[:, :L], epi=epi)
    assert torch.equal(dheads[:, :L], dmu) and torch.equal(dheads[:, L:], dlv)
    # against float64, so that the pair is anchored
    m_, l_ = hd[:, :L].double().cpu().requires_grad_(True), hd[:, L:].double().cpu().requires_grad_(True)
    z = m_ + eps.double().cpu() * torch.exp(0.5 * l_) if train else m_
    klr = -0.5 * (1 + l_ - m_ ** 2 - l_.exp()).sum(1)
    ((z * (Gm.double() @ W.double()).cpu()).sum() + float(np.float32(ks)) * klr.sum()).backward()
    assert _maxrel(dmu, m_.grad) < 1e-5 and _maxrel(dlv, l_.grad) < 1e-5


# ======================================================== (e) the module API ==
_FN_ORDER = ["EncoderFirstFn", "LnGeluDropFn", "ReparamFn", "LinearFn"]


@pytest.mark.parametrize("latent", [32, 64])
def test_module_api_train_backward_vs_float64(hip_device, monkeypatch, latent):
    """model(x) -> vae_loss_function -> backward() in train mode, dropout on: each autograd Function draws a seed
    (hvae.autograd._seed) that its backward must reuse. The seeds are handed out by the test (distinct, >= 2^32),
    the masks and eps rebuilt from them at step 0 (the module API passes no step counter), and the float64 oracle
    fed those must give the model's losses and every parameter's gradient. latent = 64 = d: no projection layer."""
    from hvae import autograd, ops
    from src.ml.model import HybridVAE, vae_loss_function
    N, d, hidden, B, beta = 300, 64, [64, 48], 16, 0.2
    seeds, callers, saved = [], [], []

    def fake_seed():
        callers.append(type(sys._getframe(1).f_locals.get("ctx")).__name__.replace("Backward", ""))
        seeds.append(((len(seeds) + 3) << 40) + 1000 + 17 * len(seeds))
        return seeds[-1]

    real_reparam = ops.reparam_kl_fwd

    def spy_reparam(mu, logvar, train, seed, *a, **k):
        out = real_reparam(mu, logvar, train, seed, *a, **k)
        if train:
            saved.append(out[1])
        return out
    monkeypatch.setattr(autograd, "_seed", fake_seed)
    monkeypatch.setattr(ops, "reparam_kl_fwd", spy_reparam)
    X = synth_csr(B, N, lam=6.0, seed=31)
    E = synth_embeddings(N, d, seed=32)
    torch.manual_seed(0)
    model = HybridVAE(N, E, latent_dim=latent, hidden_dims=hidden, dropout=PD, beta=beta).to(hip_device).train()
    x = torch.as_tensor(X.toarray(), dtype=torch.float32)
    xd = x.to(hip_device)
    scores, mu, logvar = model(xd)
    total, recon, kl = vae_loss_function(scores, xd, mu, logvar, beta)
    total.backward()
    has_proj = latent != d
    want_order = _FN_ORDER if has_proj else _FN_ORDER[:3]
    assert callers == want_order and len(set(seeds)) == len(seeds) == len(want_order)
    assert all(s >= 2 ** 32 for s in seeds)
    # the restated randomness of this forward
    enc = [_t(P.mult(seeds[k], 0, P.TAG_ENC_DROP + k, B, hidden[k], PD)).double() for k in range(2)]
    proj = _t(P.mult(seeds[3], 0, P.TAG_PROJ_DROP, B, d, PD)).double() if has_proj else None
    assert len(saved) == 1
    _eps_ok(saved[0], seeds[2], 0, B, latent, "module API")
    eps = _t(P.normal(seeds[2], 0, B, latent))
    p64 = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    g64, loss64 = R.grads(p64, x.double(), beta, enc_masks=enc, proj_mask=proj, eps=eps)
    got = [float(t) for t in (total, recon, kl)]
    rel = [abs(a - b) / abs(b) for a, b in zip(got, loss64)]
    print("module API losses (total, recon, kl) relative to float64:", [f"{r:.2e}" for r in rel])
    err = {}
    params = dict(model.named_parameters())
    assert sorted(params) == sorted(g64)
    for n, ref in g64.items():
        assert params[n].grad is not None, n
        err[n] = _maxrel(params[n].grad, ref)
    print("module API gradients relative to float64:", {n: f"{e:.2e}" for n, e in err.items()})
    assert max(rel) < 2e-5, rel
    bad = {n: e for n, e in err.items() if not e < 5e-5}
    assert not bad, bad


# ==================================================== (f) the fused trainer ==
FSEED = (7 << 40) + 55
F_B, F_N, F_D, F_L, F_BETA = 32, 300, 128, 64, 0.2
STATE = ("flat", "m", "v", "w1t", "m_w1t", "v_w1t")


def _trainers(hip_device, hidden, rows, graphs, n_users, B=F_B):
    """Trainer G (nothing injected; graphs as asked) and trainer I (eager, for injection) from the same model."""
    from hvae.executor import FusedTrainer
    from src.ml.model import HybridVAE
    X = synth_csr(n_users, F_N, lam=6.0, seed=41)
    E = synth_embeddings(F_N, F_D, seed=42)

    def build(use_graphs):
        torch.manual_seed(0)
        model = HybridVAE(F_N, E, latent_dim=F_L, hidden_dims=hidden, dropout=PD, beta=F_BETA).to(hip_device)
        f = FusedTrainer(model, hip_device, precision="fp32", seed=FSEED, use_graphs=use_graphs)
        f.mlp_rows = rows
        return f, f.device_data(X, list(range(n_users)))
    (G, dG), (I, dI) = build(graphs), build(False)
    assert G._mlp_rows_ok(B) == (rows and hidden == [128])
    assert torch.equal(G.flat, I.flat)
    return G, dG, I, dI


def _restated_ext(hidden, t, eps, dev, B=F_B):
    return {"enc_masks": [_t(P.mult(FSEED, t, P.TAG_ENC_DROP + k, B, hk, PD), dev) for k, hk in enumerate(hidden)],
            "proj_mask": _t(P.mult(FSEED, t, P.TAG_PROJ_DROP, B, F_D, PD), dev), "eps": eps}


@pytest.mark.parametrize("hidden,rows,B", [([128], True, F_B), ([128], False, F_B), ([64, 48], True, F_B),
                                           ([128], True, 512), ([128], False, 512)],
                         ids=["rows", "gemm_chain", "two_hidden", "rows_b512", "gemm_chain_b512"])
def test_fused_trainer_generated_equals_injected(hip_device, hidden, rows, B):
    """Trainer G runs three steps with nothing injected; trainer I, built from the same model, runs them with the
    masks restated at (seed, step t) and G's saved eps injected. Losses, parameters and Adam moments must be
    bitwise equal after every step: then the forward and the backward of every layer saw the same (seed, step,
    tag) inside a real step -- on the row-parallel path (hidden [128]: the encoder layer fused into it) and on the
    GEMM chain (mlp_rows off; and hidden [64, 48], whose width 48 the row kernels do not take). B = 512 is the
    smallest batch whose step spreads over streams: the row-gradient plan on its own stream and the weight-gradient
    GEMMs on a side stream, beside the kernels that draw the masks again and ahead of the clip that advances
    step_dev."""
    G, dG, I, dI = _trainers(hip_device, hidden, rows, False, B, B)
    assert (G.side is not None and B >= G.plan_side_min_batch) == (B == 512)
    for t in range(3):
        assert int(G.step_dev.item()) == t and int(I.step_dev.item()) == t
        loss_g = G.step_batch(dG, None, B, F_BETA, PD, train=True).clone()
        eps_g = G._bufs[(B, True)].eps.clone()
        _eps_ok(eps_g, FSEED, t, B, F_L, f"fused trainer step {t}")
        loss_i = I.step_batch(dI, None, B, F_BETA, PD, train=True, ext=_restated_ext(hidden, t, eps_g, hip_device, B))
        torch.cuda.synchronize()
        assert torch.isfinite(loss_g).all()
        assert torch.equal(loss_g, loss_i), (t, loss_g, loss_i)
        for name in STATE:
            assert torch.equal(getattr(G, name), getattr(I, name)), (t, name)
    assert int(G.step_dev.item()) == 3


def test_fused_trainer_graph_replay_generated_equals_injected(ops, hip_device):
    """The same with G's steps 1 and 2 replayed from a captured graph: one run_epoch over three batches of 32 (the
    first batch of a buffer set runs eagerly, the second is captured and replayed, the third replayed; step_dev
    advances on the device between them). G's eps is overwritten by each step, so I is fed the eps of
    hvae_reparam_kl_fwd at (seed, step t) -- bitwise the trainer's, as G's last one shows -- with the restated masks;
    the epoch's mean losses and the state after it must equal I's three eager steps."""
    from hvae.executor import ConstBeta
    hidden = [128]
    G, dG, I, dI = _trainers(hip_device, hidden, True, True, 3 * F_B)
    assert int(G.step_dev.item()) == 0
    res = G.run_epoch(dG, F_B, False, ConstBeta(F_BETA), PD)
    bf = G._bufs[(F_B, True)]
    assert bf.graph is not None and int(G.step_dev.item()) == 3
    zero = torch.zeros(F_B, F_L, device=hip_device)
    sums = [0.0, 0.0, 0.0]
    for t in range(3):
        assert int(I.step_dev.item()) == t
        step = torch.full((1,), t, dtype=torch.int64, device=hip_device)
        _, eps_t, _ = ops.reparam_kl_fwd(zero, zero, True, FSEED, step=step)
        _eps_ok(eps_t, FSEED, t, F_B, F_L, f"graph-replayed trainer, step {t}")
        users = torch.arange(t * F_B, (t + 1) * F_B, dtype=torch.int32, device=hip_device)
        loss_i = I.step_batch(dI, users, F_B, F_BETA, PD, train=True, ext=_restated_ext(hidden, t, eps_t, hip_device))
        sums = [s + float(v) for s, v in zip(sums, loss_i.cpu())]
    torch.cuda.synchronize()
    assert torch.equal(bf.eps, eps_t)
    for name in STATE:
        assert torch.equal(getattr(G, name), getattr(I, name)), name
    for key, s in zip(("total_loss", "recon_loss", "kl_loss"), sums):
        assert math.isfinite(res[key]) and abs(res[key] - s / 3) <= 1e-12 * abs(s), (key, res[key], s / 3)
