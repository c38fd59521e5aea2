"""Checks of the A/B variant kernels (not collected by default: no test_ prefix).

The product libhvae.so runs one sweep per (dtype, d) and ignores the environment. The retired variants -- bf16
versions 2, 3 and 4 at d = 768 beside version 5, version 6 (96 users per E tile), the d = 384 version 5
(k_dec5w_bf16), the fp8 sweep with version 4's structure (k_dec4_f8) and the D-split ring beside the fp8 version 5
(k_dec5_f8) -- live in recommendation-system_amd/csrc/ab/ and build only with -DHVAE_AB=1
(`make -C recommendation-system_amd lib-ab` -> build_var/libhvae_ab.so), where HVAE_DEC_* select them at plan time.
The same build holds the fused top-K's A/B arms (HVAE_TOPK_LDS, HVAE_TOPK_WAVE_USERS, HVAE_TK_TAU_PERIOD: the
global-load scan at the LDS-served widths and its tile-split mapping). tests/test_gpu_ab_variant.py runs this file
in a subprocess with HVAE_LIB pointing at that build, so the variants keep their parity checks without being
shipped.
"""
import os
import sys
from pathlib import Path

import pytest
import torch

HERE = Path(__file__).resolve().parent
for _p in (str(HERE.parent / "recommendation-system_amd"), str(HERE.parent), str(HERE / "golden"), str(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from gen import synth_csr, synth_embeddings  # noqa: E402

pytestmark = pytest.mark.skipif(not os.environ.get("HVAE_LIB", "").endswith("libhvae_ab.so"),
                                reason="runs against the A/B variant build only (tests/test_gpu_ab_variant.py)")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ops(dev):
    from hvae import ops
    return ops


def _maxrel(a, b):
    a = a.detach().double()
    b = b.detach().double().to(a.device)
    return float((a - b).abs().max() / max(b.abs().max().item(), 1e-30))


def _sweep(dtype, nb, N, D):
    """The sweep hvae_decoder_plan names for a call with the whole workspace, under the environment as it is now."""
    import ctypes as C
    from hvae._lib import DEC_SWEEPS, DecPlan, check, lib
    p = DecPlan()
    check(lib().hvae_decoder_plan(dtype, nb, N, D, 2 ** 64 - 1, C.byref(p)), "hvae_decoder_plan")
    return DEC_SWEEPS[p.sweep]


def test_decoder_d768_versions_agree(ops, dev, monkeypatch):
    """Versions 5 (GEMM1 and GEMM2 on different waves, the product sweep), 4 (item-split GEMM1, one barrier
    per tile) and 3 (item-half softmax ownership) against version 2 (whole-tile softmax in both waves) of the
    d = 768 bf16 sweep: all round the same bf16 operands (P to bf16 included); only fp32 summation order
    differs."""
    nb, N, D = 700, 50_001, 768
    g = torch.Generator(device=dev).manual_seed(11)
    E = torch.randn(N, D, device=dev, generator=g)
    E /= E.norm(dim=1, keepdim=True)
    U = torch.randn(nb, D, device=dev, generator=g)
    U *= 4.0 / U.norm(dim=1, keepdim=True)
    X = synth_csr(nb, N, lam=15.0, seed=3)
    xd = ops.csr_from_scipy(X, dev)
    img = ops.decoder_image(E)
    enorm = ops.row_norm_max(img)
    out = {}
    for name, v3, v4, v5 in (("v5", "1", "1", "1"), ("v4", "1", "1", "0"), ("v3", "1", "0", "0"),
                             ("v2", "0", "0", "0")):
        monkeypatch.setenv("HVAE_DEC_V3", v3)
        monkeypatch.setenv("HVAE_DEC_V4", v4)
        monkeypatch.setenv("HVAE_DEC_V5", v5)
        assert _sweep(img.dtype, nb, N, D) == "bf16_" + name  # the four settings run four different kernels
        out[name] = ops.decoder_train(xd, U, img, enorm, E, 1.0 / nb, want_o=True)
    l2, o2, r2, d2 = out["v2"]
    for name in ("v5", "v4", "v3"):
        la, oa, ra, da = out[name]
        assert (la - l2).abs().max() < 1e-4, name
        assert _maxrel(oa, o2) < 5e-3 and _maxrel(ra, r2) < 1e-5 and _maxrel(da, d2) < 5e-3, name


@pytest.mark.parametrize("variant", ["F8V4", "ring"])
@pytest.mark.parametrize("nb,N", [(64, 2000), (300, 5001), (7, 100), (130, 4000)])
def test_decoder_fp8_v4_structure(ops, dev, nb, N, variant, monkeypatch):
    """The retired fp8 d = 768 sweeps -- k_dec4_f8 (HVAE_DEC_F8V4=1) and the D-split ring (HVAE_DEC_F8V5=0) --
    against float64 on the quantised operands, inside the e4m3 envelope of tests/test_gpu_fp8.py, and the
    fused train form equal to fwd + bwd."""
    from test_gpu_fp8 import _image, _o_envelope, _quantised
    D = 768
    if variant == "F8V4":
        monkeypatch.setenv("HVAE_DEC_F8V4", "1")
    else:
        monkeypatch.setenv("HVAE_DEC_F8V5", "0")
    from hvae import _lib
    assert _sweep(_lib.HVAE_FP8, nb, N, D) == ("fp8_v4" if variant == "F8V4" else "fp8_ring")
    E = torch.as_tensor(synth_embeddings(N, D, seed=N))
    g = torch.Generator().manual_seed(nb)
    U = torch.randn(nb, D, generator=g) * 3.0
    img = _image(ops, E.to(dev))
    enorm = ops.row_norm_max(img)
    lse, O = ops.decoder_fwd(U.to(dev), img, enorm)
    Eq, Uq, _ = _quantised(E, U)
    S = Uq.double() @ Eq.double().t()
    lse_ref = torch.logsumexp(S, 1)
    O_ref = torch.softmax(S, 1) @ Eq.double()
    assert (lse.double().cpu() - lse_ref).abs().max() < 2e-4 * max(1.0, lse_ref.abs().max().item())
    assert ((O.double().cpu() - O_ref).abs() <= _o_envelope(S, Eq)).all()
    X = synth_csr(nb, N, lam=5.0, seed=nb + N)
    xd = ops.csr_from_scipy(X, dev)
    lse_t, O_t, rr, dU = ops.decoder_train(xd, U.to(dev), img, enorm, E.to(dev), 1.0 / nb, want_o=True)
    rr_b, dU_b = ops.decoder_bwd(xd, U.to(dev), E.to(dev), lse, O, 1.0 / nb)
    assert torch.equal(lse_t, lse) and torch.equal(O_t, O) and torch.equal(rr, rr_b) and torch.equal(dU, dU_b)


@pytest.mark.parametrize("nb,N", [(300, 5001), (4096, 20_000), (129, 777)])
def test_decoder_d384_v5w_agrees_v2(ops, dev, nb, N, monkeypatch):
    """The d = 384 128-user producer / consumer sweep (k_dec5w_bf16, HVAE_DEC_V5W=1, A/B only: slower) against
    version 2's DS = 1 sweep (the product's): the same bf16 operands, P rounded to bf16 in both; only fp32
    summation order differs."""
    D = 384
    g = torch.Generator(device=dev).manual_seed(nb)
    E = torch.randn(N, D, device=dev, generator=g)
    E /= E.norm(dim=1, keepdim=True)
    U = torch.randn(nb, D, device=dev, generator=g)
    U *= 4.0 / U.norm(dim=1, keepdim=True)
    xd = ops.csr_from_scipy(synth_csr(nb, N, lam=15.0, seed=3), dev)
    img = ops.decoder_image(E)
    enorm = ops.row_norm_max(img)
    out = {}
    for v in ("1", "0"):
        monkeypatch.setenv("HVAE_DEC_V5W", v)
        assert _sweep(img.dtype, nb, N, D) == ("bf16_v5w" if v == "1" else "bf16_v2")
        out[v] = ops.decoder_train(xd, U, img, enorm, E, 1.0 / nb, want_o=True)
    (la, oa, ra, da), (lb, ob, rb, db) = out["1"], out["0"]
    assert (la - lb).abs().max() < 1e-4
    assert _maxrel(oa, ob) < 5e-3 and _maxrel(ra, rb) < 1e-5 and _maxrel(da, db) < 5e-3


@pytest.mark.parametrize("nb,N,lam,hot", [(4096, 100_000, 15.0, 300), (300, 2000, 8.0, 100), (40000, 3000, 1.0, 6000),
                                         (2000, 1_000_003, 15.0, 0), (32768, 1_000_000, 15.0, 0)])
def test_rowgrad_sorted_plan_equals_atomic_plan(ops, dev, nb, N, lam, hot, monkeypatch):
    """The radix-sort plan (hvae_rgsort.hip, HVAE_RG_SORTED=1; the product's for batches of >= 32 K entries) against
    the atomic plan (HVAE_RG_SORTED=0): every
    output the apply and the lazy Adam read is bitwise equal (slots, segments, contributions and their slots,
    slot_of at the batch's items), and so are the gradient rows."""
    import numpy as np
    import scipy.sparse as sp
    X = synth_csr(nb, N, lam=lam, seed=nb)
    if hot:
        X = X.tolil()
        X[:hot, 0] = 1.0
        X = sp.csr_matrix(X)
    H = 64
    da = torch.randn(nb, H, generator=torch.Generator().manual_seed(2)).to(dev)
    xd = ops.csr_from_scipy(X, dev)
    outs = {}
    for v in ("1", "0"):
        monkeypatch.setenv("HVAE_RG_SORTED", v)
        rg = ops.RowGradBuffers(N, H, int(X.nnz), dev)
        ops.w1_rowgrad(xd, da, rg)
        nu = int(rg.n_unique.item())
        tot = int(rg.seg_off[nu].item())
        items = rg.item_of[:nu].long()
        outs[v] = (nu, tot, rg.item_of[:nu].clone(), rg.seg_off[: nu + 1].clone(), rg.contrib_row[:tot].clone(),
                   rg.contrib_val[:tot].clone(), rg.contrib_slot[:tot].clone(), rg.slot_of[items].clone(),
                   rg.rows[:nu].clone(), int(rg.cnt.abs().sum()), int(rg.fill.abs().sum()))
    a, b = outs["1"], outs["0"]
    assert a[0] == b[0] and a[1] == b[1] == X.nnz
    for x, y in zip(a[2:9], b[2:9]):
        assert torch.equal(x, y)
    assert a[9] == 0 and a[10] == 0
    np.testing.assert_array_equal(a[2].cpu().numpy(), np.unique(X.indices))


@pytest.mark.parametrize("R,N", [(33, 4097), (130, 777)])
@pytest.mark.parametrize("D", [128, 768])
def test_topk_fused_scans_and_mappings_agree(ops, dev, D, R, N, monkeypatch):
    """The fused top-K's A/B arms -- the global-load scan where the product runs the LDS scan (HVAE_TOPK_LDS=0), its
    tile-split mapping (HVAE_TOPK_WAVE_USERS=0) and a read of the other waves' bounds at every tile
    (HVAE_TK_TAU_PERIOD=1) -- against float64 (tests/test_gpu_topk.py's check and tolerance), each named by the plan
    query before it runs. The final ranking is an exact fp32 rescore of the candidates in a fixed order, so the path
    the candidates took must not show: idx and val are bitwise the default setting's."""
    import ctypes as C
    from hvae._lib import TOPK_SCANS, TopkPlan, check, lib
    from test_gpu_topk import _case, _check
    k = 10
    U, E, Ud, Ed, img, emax = _case(dev, R, N, D, seed=N + D)
    settings = [({}, ("lds", 1, 128, 8)),
                ({"HVAE_TOPK_LDS": "0"}, ("global", 1, 128, 8)),
                ({"HVAE_TOPK_LDS": "0", "HVAE_TOPK_WAVE_USERS": "0"}, ("global", 0, 32, 8)),
                ({"HVAE_TK_TAU_PERIOD": "1"}, ("lds", 1, 128, 1))]
    out = []
    for env, want in settings:
        for name in ("HVAE_TOPK_LDS", "HVAE_TOPK_WAVE_USERS", "HVAE_TK_TAU_PERIOD"):
            monkeypatch.delenv(name, raising=False)
        for name, v in env.items():
            monkeypatch.setenv(name, v)
        p = TopkPlan()
        check(lib().hvae_topk_fused_plan(R, N, D, k, C.byref(p)), "hvae_topk_fused_plan")
        assert (TOPK_SCANS[p.scan], p.wave_users, p.block_users, p.tau_period) == want, env
        assert p.nseg == p.splits * (2 if p.wave_users else 8)
        idx, val, flag = ops.topk_fused(Ud, img, Ed, emax, k, with_flags=True)
        assert int(flag.sum()) == 0, env
        _check(idx, val, U, E, k)
        out.append((idx, val))
    for (idx, val), (env, _) in zip(out[1:], settings[1:]):
        assert torch.equal(idx, out[0][0]) and torch.equal(val, out[0][1]), env


@pytest.mark.parametrize("nb,N", [(97, 3001), (700, 50_001), (4096, 3000), (4096, 200_000), (1000, 40_000)])
def test_decoder_bf16_d768_v6_tasks(ops, dev, nb, N, monkeypatch):
    """The d = 768 bf16 sweep above 64 users (k_dec6_bf16: 96 users per E tile, csrc/ab/hvae_decoder6.hip) against
    float64 on the bf16-rounded operands, over its work assignment: a partial user block (97), 8 user blocks x 32
    splits (700), 43 user blocks with the two excess tasks cut into 128 pieces each -- at 3000 items most of the
    pieces are empty, at 200,000 every piece runs 40 tiles (4096) -- and 11 user blocks with 8 excess tasks (1000).
    The fused train form (merge + sparse terms) equals decoder_fwd + decoder_bwd on the same inputs. Version 6
    tied with version 5 at the Syn-10M shard, so it runs only here (HVAE_DEC_V6=1)."""
    monkeypatch.setenv("HVAE_DEC_V6", "1")
    D = 768
    g = torch.Generator(device=dev).manual_seed(nb + N)
    E = torch.randn(N, D, device=dev, generator=g)
    E /= E.norm(dim=1, keepdim=True)
    U = torch.randn(nb, D, device=dev, generator=g) * (4.0 / D ** 0.5)
    Ek = ops.decoder_image(E)
    enorm = ops.row_norm_max(Ek)
    lse, O = ops.decoder_fwd(U, Ek, enorm)
    Ur, Er = U.bfloat16().double(), Ek.bf16.double()
    S = Ur @ Er.t()
    lse_ref = torch.logsumexp(S, 1)
    O_ref = torch.softmax(S, 1) @ Er
    assert torch.isfinite(lse).all() and torch.isfinite(O).all()
    assert (lse.double() - lse_ref).abs().max() < 2e-3 * max(1.0, lse_ref.abs().max().item())
    assert _maxrel(O, O_ref) < 1e-2
    lse2, _ = ops.decoder_fwd(U, Ek, enorm, with_o=False)
    assert torch.allclose(lse2, lse, rtol=0, atol=1e-5)
    # no user may be flagged: a flagged user is recomputed exactly by the finalize, so a sweep that flags every
    # user still returns the right lse and O (slowly). The workspace begins with the sweep's flag words (one per
    # partial row); poisoned with 0xFF, rows the sweep never writes stay -1, and 1 marks a flagged row
    from hvae._lib import check, lib, ptr, stream_of
    dt, _, Eh = ops._dec_operand(Ek)
    need = int(lib().hvae_decoder_workspace(dt, nb, N, D))
    assert int(lib().hvae_decoder_users_per_tile(dt, nb, N, D)) == 96  # the plan took version 6
    assert _sweep(dt, nb, N, D) == "bf16_v6"
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    lse3, O3 = torch.empty_like(lse), torch.empty_like(O)
    check(lib().hvae_decoder_fwd(dt, ptr(U), U.stride(0), ptr(Eh), ptr(enorm), nb, N, D, ptr(lse3), ptr(O3), ptr(ws),
                                 ws.numel(), stream_of(U)), "hvae_decoder_fwd")
    ntiles, nub = -(-N // 32), -(-nb // 96)
    S = max(1, min(-(-256 // nub), max(1, ntiles // 8)))
    S = -(-ntiles // -(-ntiles // S))
    slots = nub * S if nub * S <= 256 else 256 + (nub * S - 256) * (256 // (nub * S - 256))
    flags = ws[:slots * 96 * 4].view(torch.int32)
    assert int((flags == 1).sum()) == 0 and int((flags == 0).sum()) >= nb
    assert torch.equal(lse3, lse) and torch.equal(O3, O)
    X = synth_csr(nb, N, lam=5.0, seed=nb)
    xd = ops.csr_from_scipy(X, dev)
    lse_t, O_t, rr, dU = ops.decoder_train(xd, U, Ek, enorm, E, 1.0 / nb, want_o=True)
    assert torch.equal(lse_t, lse) and torch.equal(O_t, O)
    rr_b, dU_b = ops.decoder_bwd(xd, U, E, lse, O, 1.0 / nb)
    assert torch.equal(rr, rr_b) and torch.equal(dU, dU_b)
