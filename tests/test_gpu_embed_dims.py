"""512- and 1024-wide item embeddings through every layer: the decoder sweeps (bf16 at 512 with the two-way D
split and at 1024 with the four-way one, fp32 and fp8 at 512), the fused train form, the large-norm fix-up, the
whole train step against the oracle, the captured step, ranking, and the refusals that remain (fp32 at
768 / 1024, fp8 at 1024).

The sweep, train-form and fix-up checks are the bodies of tests/test_gpu_kernels.py and tests/test_gpu_fp8.py run
at the new widths (called as plain functions, so the bars are theirs); the whole-step check has the structure
of tests/test_gpu_large_step.py at the bars of tests/test_gpu_train.py::STEP_TOL.
"""
import numpy as np
import pytest
import torch

from gen import synth_csr, synth_embeddings
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

L, H, P_DROP, BETA, LR = 128, [512], 0.3, 0.2, 1e-3


@pytest.fixture(scope="module")
def ops(hip_device):
    from hvae import ops
    return ops


# ---------------------------------------------------------------- 1. sweeps ---
@pytest.mark.parametrize("D", [512, 1024])
@pytest.mark.parametrize("nb,N", [(7, 100), (64, 2000), (130, 5001), (300, 12101)])
def test_sweep_bf16(ops, hip_device, nb, N, D):
    """A partial first wave with fewer tiles than splits; one 64-user block; a partial last block with an item
    tail that is no multiple of 32; several blocks and 8 splits."""
    from test_gpu_kernels import _check_decoder
    _check_decoder(ops, hip_device, "bf16", nb, N, D)


@pytest.mark.parametrize("nb,N", [(3, 50), (129, 777), (200, 5001)])
def test_sweep_fp32_512(ops, hip_device, nb, N):
    from test_gpu_kernels import _check_decoder
    _check_decoder(ops, hip_device, "f32", nb, N, 512)


@pytest.mark.parametrize("nb,N", [(7, 100), (130, 5001), (300, 12101)])
def test_sweep_fp8_512(ops, hip_device, nb, N):
    """tests/test_gpu_fp8.py's sweep check (float64 on the quantised operands, the e4m3 envelope on O)."""
    from test_gpu_fp8 import test_decoder_fp8
    test_decoder_fp8(ops, hip_device, nb, N, 512)


# ------------------------------------------------------ 2. fused train form ---
@pytest.mark.parametrize("D", [512, 1024])
@pytest.mark.parametrize("nb,N", [(64, 3000), (130, 4001)])
def test_train_fused_bf16(ops, hip_device, nb, N, D):
    from test_gpu_kernels import _check_decoder_train_fused
    _check_decoder_train_fused(ops, hip_device, "bf16", nb, N, D)


def test_train_fused_fp32_512(ops, hip_device):
    from test_gpu_kernels import _check_decoder_train_fused
    _check_decoder_train_fused(ops, hip_device, "f32", 40, 700, 512)


# -------------------------------------------------------- 3. large norms ---
@pytest.mark.parametrize("D", [512, 1024])
def test_large_norm_fixup(ops, hip_device, D):
    """96 users with |u| from 1 to 1500 over 4000 items: the underflow flags of the D-split sweeps (every wave of
    a user group must agree on the offset) and the finalize's exact recompute."""
    from test_gpu_kernels import test_decoder_large_norm_fixup
    test_decoder_large_norm_fixup(ops, hip_device, D, 12)


# ------------------------------------------------- 4. whole step vs oracle ---
def _maxrel(a, b):
    a = a.detach().double()
    b = b.detach().double().to(a.device)
    return float((a - b).abs().max() / max(b.abs().max().item(), 1e-30))


def _rms_lr(a, b):
    d = a.detach().double() - b.detach().double().to(a.device)
    return float(d.pow(2).mean().sqrt()) / LR


STEP_CASES = [("bf16", 512, 96), ("bf16", 512, 1100), ("bf16", 1024, 96), ("bf16", 1024, 1100),
              ("fp32", 512, 96), ("fp8", 512, 96)]


@pytest.mark.parametrize("precision,d,B", STEP_CASES)
def test_fused_step_vs_oracle(hip_device, precision, d, B):
    """Two steps with injected dropout masks and noise: B = 96 runs the row-parallel MLP chain, B = 1100 the
    GEMM path with K = d."""
    from test_gpu_train import STEP_TOL

    from hvae import ops
    from hvae.executor import FusedTrainer
    from src.ml.model import HybridVAE
    N, dev, seed = 3000, hip_device, 7 * d + B
    X = synth_csr(B, N, lam=15.0, seed=seed)
    E = synth_embeddings(N, d, seed=seed + 1)
    g = torch.Generator(device=dev).manual_seed(seed + 2)

    def ext():
        return {"enc_masks": [(torch.rand(B, H[0], device=dev, generator=g) >= P_DROP).float() / (1 - P_DROP)],
                "proj_mask": (torch.rand(B, d, device=dev, generator=g) >= P_DROP).float() / (1 - P_DROP),
                "eps": torch.randn(B, L, device=dev, generator=g)}
    steps = [ext(), ext()]

    torch.manual_seed(seed)
    model = HybridVAE(N, E, latent_dim=L, hidden_dims=H, dropout=P_DROP, beta=BETA).to(dev)
    fused = FusedTrainer(model, dev, lr=LR, precision=precision, use_graphs=False)
    data = fused.device_data(X, list(range(B)))
    got_loss, got_norm = [], []
    for s in range(2):
        got_loss.append(fused.step_batch(data, None, B, BETA, P_DROP, train=True, ext=steps[s]).cpu().numpy())
        got_norm.append(fused.norm.item())
        if s == 0:
            bf = fused._bufs[(B, True)]
            w1 = torch.zeros(N, H[0], device=dev)
            ops.rowgrad_to_dense(bf.rg, w1)
            gW, gb = fused.gW_heads, fused.gb_heads
            got_grad = {"encoder.0.weight": w1.t().contiguous(), "fc_mu.weight": gW[:L].clone(),
                        "fc_logvar.weight": gW[L:].clone(), "fc_mu.bias": gb[:L].clone(),
                        "fc_logvar.bias": gb[L:].clone()}
            for n, t in fused.G.items():
                got_grad[n] = t.clone()
    torch.cuda.synchronize()
    lay = fused.layout
    got_p = {n: p.detach().clone() for n, p in model.named_parameters()}
    got_m = {n: (fused.m_w1t.t() if n == "encoder.0.weight" else lay.view(fused.m, n)).clone() for n in got_p}
    got_v = {n: (fused.v_w1t.t() if n == "encoder.0.weight" else lay.view(fused.v, n)).clone() for n in got_p}

    # the oracle: the reference's dense fp32 step on the same device
    p = {k: v.to(dev) for k, v in R.init_params(N, E, L, H, seed=seed).items()}
    x = torch.as_tensor(X.toarray(), dtype=torch.float32, device=dev)
    state, ref = {}, []
    for s in range(2):
        ref.append(R.train_step(p, state, x, BETA, lr=LR, enc_masks=steps[s]["enc_masks"],
                                proj_mask=steps[s]["proj_mask"], eps=steps[s]["eps"]))
        if s == 0:
            ref_grad = {n: t.clone() for n, t in ref[0]["grads"].items()}
    torch.cuda.synchronize()

    tol = STEP_TOL[precision]
    err = {}
    for s in range(2):
        want = np.asarray(ref[s]["loss"])
        err[f"loss:{s}"] = float(np.max(np.abs(got_loss[s] - want) / np.abs(want)))
        err[f"norm:{s}"] = abs(got_norm[s] - ref[s]["total_norm"]) / ref[s]["total_norm"]
    for n, t in ref_grad.items():
        err[f"grad:{n}"] = _maxrel(got_grad[n], t)
    for n, t in got_p.items():
        m, v = state[n]
        # fp32 bars parameters relative to their magnitude, the low precisions by RMS in units of lr
        # (tests/test_gpu_train.py::_step_errors)
        err[f"param:{n}"] = _maxrel(t, p[n]) if precision == "fp32" else _rms_lr(t, p[n])
        err[f"m:{n}"] = _maxrel(got_m[n], m)
        err[f"v:{n}"] = _maxrel(got_v[n], v)
    print(precision, d, B, {k: f"{e:.2e}" for k, e in err.items()})
    bad = {k: e for k, e in err.items() if not e <= tol[k.split(":")[0]]}
    assert not bad, (precision, d, B, bad)


# ------------------------------------------------- 5. captured step == eager ---
def test_graph_replay_is_bitwise_eager_d1024(hip_device):
    """One epoch of three 96-user batches at d = 1024 through the captured step leaves bitwise the parameters of
    the eager epoch (tests/test_gpu_train.py::test_graph_replay_is_bitwise_eager's idiom)."""
    from hvae.executor import ConstBeta, FusedTrainer
    from src.ml.model import HybridVAE
    n_users, N, d = 288, 3000, 1024
    X = synth_csr(n_users, N, seed=3)
    E = synth_embeddings(N, d, seed=4)
    outs = []
    for graphs in (False, True):
        torch.manual_seed(0)
        model = HybridVAE(N, E, latent_dim=L, hidden_dims=H, dropout=P_DROP, beta=BETA).to(hip_device)
        fused = FusedTrainer(model, hip_device, precision="bf16", seed=1234, use_graphs=graphs)
        data = fused.device_data(X, list(range(n_users)))
        gen = torch.Generator().manual_seed(5)
        m1 = fused.run_epoch(data, 96, True, ConstBeta(BETA), P_DROP, generator=gen)
        outs.append((m1, fused.flat.clone()))
    (a1, af), (b1, bf_) = outs
    assert a1 == b1
    assert torch.equal(af, bf_)


# ------------------------------------------------------------- 6. ranking ---
@pytest.mark.parametrize("d", [512, 1024])
def test_ranking(hip_device, d):
    """HybridVAE.recommend and topk_scores (with seen items excluded) at d = 512 (the fused top-K) and d = 1024
    (fp32 score matrix + hvae_topk): the float64 ranking up to fp32 ties."""
    from hvae import ops
    from src.ml.model import HybridVAE
    R_, N, k = 70, 2500, 20
    X = synth_csr(R_, N, lam=15.0, seed=d)
    E = synth_embeddings(N, d, seed=d + 1)
    torch.manual_seed(3)
    m = HybridVAE(N, E, latent_dim=64, hidden_dims=[256], dropout=0.3, beta=0.2).to(hip_device).eval()
    z = torch.randn(R_, 64, generator=torch.Generator().manual_seed(9)).to(hip_device)
    with torch.no_grad():
        u = m.projection_layer(z).contiguous()
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
    csr = ops.csr_from_scipy(X, hip_device)
    ex = ops.Csr(csr.row_ptr, csr.col_idx, csr.vals, N, rows=torch.arange(R_, dtype=torch.int32, device=hip_device))
    idx, val = m.topk_scores(u, k, exclude=ex)
    Sx = S.clone()
    for r in range(R_):
        Sx[r, torch.as_tensor(X[r].indices.astype(np.int64))] = -float("inf")
    check(idx.cpu(), val.cpu(), Sx)


# ------------------------------------------------------------ 7. refusals ---
@pytest.mark.parametrize("precision", ["fp32", "fp8"])
def test_refused_precisions_at_1024(hip_device, precision):
    from hvae import _lib, ops
    from hvae.executor import FusedTrainer
    from src.ml.model import HybridVAE
    N, d = 300, 1024
    model = HybridVAE(N, synth_embeddings(N, d, seed=1), latent_dim=64, hidden_dims=[128]).to(hip_device)
    with pytest.raises(NotImplementedError) as e:
        FusedTrainer(model, hip_device, precision=precision, use_graphs=False)
    dt = _lib.HVAE_F32 if precision == "fp32" else _lib.HVAE_FP8
    widths = [w for w in range(1, 1025) if ops.decoder_supported(dt, w)]
    assert 512 in widths and d not in widths
    named = [int(t) for t in str(e.value).replace(",", " ").replace(")", " ").split() if t.isdigit()]
    assert named == [d] + widths, str(e.value)
    # with no precision asked for, 512 and 1024 resolve to the bf16 sweep
    assert FusedTrainer(model, hip_device, use_graphs=False).precision == "bf16"
