"""The d = 768 bf16 sweep's tile loops (k_dec5_bf16, hvae_decoder5.hip) at the smallest shapes where they can go
wrong: the steady-state loop runs only from a split's third-last tile back, its last two iterations are peeled
off, the ring's slots and the P parity rotate in scalars, and only the sweep's last tile takes the item-tail mask.

Users 1, 33, 64, 97: a partial user group, an inactive wave pair, the nb - 1 row clamp, a second user block.
Items 31 .. 4097: splits of 1, 2, 3 and >= 4 tiles (asserted from the library's split rule, restated here and
checked against the split count the library's workspace size implies), N % 32 in {0, 1, 31}. The rule never makes
a split without tiles (the last split holds the remainder, at least one tile), so that count cannot be reached
through the library; the test asserts that as well.

Every call gets a workspace filled with 0xFF bytes (NaN as floats, -1 as flag words) and no user may come out
flagged: the finalize recomputes a flagged user exactly, which would hide a broken sweep.
"""
import pytest
import torch

from gen import synth_csr, synth_embeddings

pytestmark = pytest.mark.gpu

D = 768
NBS = [1, 33, 64, 97]
NS = [31, 32, 33, 65, 97, 389, 4097]


@pytest.fixture(scope="module")
def ops(hip_device):
    from hvae import ops
    return ops


def _maxrel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / max(b.abs().max().item(), 1e-30))


def _cdiv(a, b):
    return -(-a // b)


def _split_tiles(nb, N):
    """hvae_decoder.hip's dec_plan for bf16 at d = 768 (64 users per block, 32-item tiles): tiles of each split."""
    nub, tiles = _cdiv(nb, 64), _cdiv(N, 32)
    s = _cdiv(256, max(1, nub))
    s = min(s, max(1, tiles // 2))
    s = min(s, max(1, N // max(1, 2 * nb)))
    if s >= 8:
        s = s // 8 * 8

    def set_splits(s):
        s = max(1, min(s, tiles, 4096))
        tps = max(1, _cdiv(tiles, s))
        return tps, _cdiv(tiles, tps)

    tps, S = set_splits(s)
    if S >= 8 and S % 8:
        tps, S = set_splits(S // 8 * 8)
    return [min(tiles, (i + 1) * tps) - i * tps for i in range(S)]


def _ws_bytes(S, nb):
    return _cdiv(S * nb * 4, 256) * 256 + ((_cdiv(2 * S * nb, 4) * 4 + S * nb * D) * 4 if S > 1 else 0) + nb * D * 4


def test_cases_cover_the_tile_counts_and_tails():
    """A split of 1, 2, 3 and >= 4 tiles, never 0 (the rule's remainder split); N % 32 of 0, 1 and 31."""
    seen = set()
    for nb in NBS:
        for N in NS:
            counts = _split_tiles(nb, N)
            assert min(counts) >= 1 and sum(counts) == _cdiv(N, 32)
            seen |= {min(c, 4) for c in counts}
    assert seen == {1, 2, 3, 4}
    assert {N % 32 for N in NS} >= {0, 1, 31}


@pytest.fixture(scope="module")
def items(hip_device, ops):
    """Per N: the bf16 image, its norm bound, the fp32 E on the device and the bf16-rounded E in float64."""
    out = {}
    for N in NS:
        Ed = torch.as_tensor(synth_embeddings(N, D, seed=N)).to(hip_device)
        Ek = ops.decoder_image(Ed)
        out[N] = (Ek, ops.row_norm_max(Ek), Ed, Ek.bf16.float().cpu().double())
    return out


def _poisoned_ws(ops, hip_device, Ek, nb, N):
    """A 0xFF-filled workspace of the library's size for (nb, N), and the split count that size implies."""
    from hvae._lib import lib
    dt, _, _ = ops._dec_operand(Ek)
    need = int(lib().hvae_decoder_workspace(dt, nb, N, D))
    counts = _split_tiles(nb, N)
    assert need == _ws_bytes(len(counts), nb), "the split rule restated in this file is not the library's"
    return torch.full((need,), 0xFF, dtype=torch.uint8, device=hip_device), len(counts)


def _assert_no_flag(ws, S, nb):
    flags = ws[:S * nb * 4].view(torch.int32)
    assert int((flags == 1).sum()) == 0, "the sweep flagged a user"
    assert int((flags == 0).sum()) == S * nb, "a split left a user's flag unwritten"


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("nb", NBS)
def test_dec5_forward(ops, hip_device, items, nb, N):
    """decoder_fwd with and without O against float64 on the bf16-rounded operands (test_decoder_bf16_d768's
    tolerances), from a poisoned workspace, no user flagged."""
    from hvae._lib import check, lib, ptr, stream_of
    Ek, enorm, _, Er = items[N]
    g = torch.Generator().manual_seed(nb)
    U = torch.randn(nb, D, generator=g) * 3.0
    Ud = U.to(hip_device)
    S = U.bfloat16().double() @ Er.t()
    lse_ref = torch.logsumexp(S, 1)
    O_ref = torch.softmax(S, 1) @ Er
    dt, _, Eh = ops._dec_operand(Ek)
    ws, nsplit = _poisoned_ws(ops, hip_device, Ek, nb, N)
    lse, O = torch.empty(nb, device=hip_device), torch.empty(nb, D, device=hip_device)
    check(lib().hvae_decoder_fwd(dt, ptr(Ud), Ud.stride(0), ptr(Eh), ptr(enorm), nb, N, D, ptr(lse), ptr(O), ptr(ws),
                                 ws.numel(), stream_of(Ud)), "hvae_decoder_fwd")
    _assert_no_flag(ws, nsplit, nb)
    lse_err = float((lse.double().cpu() - lse_ref).abs().max())
    o_err = _maxrel(O, O_ref)
    print(f"nb {nb} N {N} splits {nsplit}: lse err {lse_err:.3g}, O maxrel {o_err:.3g}")
    assert torch.isfinite(lse).all() and torch.isfinite(O).all()
    assert lse_err < 2e-3 * max(1.0, lse_ref.abs().max().item())
    assert o_err < 1e-2
    ws.fill_(0xFF)
    lse2 = torch.empty(nb, device=hip_device)
    check(lib().hvae_decoder_fwd(dt, ptr(Ud), Ud.stride(0), ptr(Eh), ptr(enorm), nb, N, D, ptr(lse2), None, ptr(ws),
                                 ws.numel(), stream_of(Ud)), "hvae_decoder_fwd")
    _assert_no_flag(ws, nsplit, nb)
    assert torch.allclose(lse2, lse, rtol=0, atol=1e-5)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("nb", NBS)
def test_dec5_train_fused(ops, hip_device, items, nb, N):
    """The fused train call (sweep + merge + sparse terms) from a poisoned workspace == decoder_fwd + decoder_bwd,
    and against torch autograd with test_decoder_train_fused_d768's tolerances; no user flagged."""
    from hvae._lib import check, lib, ptr, stream_of
    Ek, enorm, Ed, _ = items[N]
    X = synth_csr(nb, N, lam=5.0, seed=nb + N)
    x = torch.as_tensor(X.toarray(), dtype=torch.float32)
    g = torch.Generator().manual_seed(5)
    U = torch.randn(nb, D, generator=g) * 2
    Ud = U.to(hip_device)
    xd = ops.csr_from_scipy(X, hip_device)
    dt, _, Eh = ops._dec_operand(Ek)
    ws, nsplit = _poisoned_ws(ops, hip_device, Ek, nb, N)

    def train(want_o, want_du):
        ws.fill_(0xFF)
        lse = torch.empty(nb, device=hip_device)
        O = torch.empty(nb, D, device=hip_device) if want_o else None
        rr = torch.empty(nb, device=hip_device)
        dU = torch.empty(nb, D, device=hip_device) if want_du else None
        check(lib().hvae_decoder_train(dt, ptr(Ud), Ud.stride(0), ptr(Eh), ptr(enorm), ptr(Ed), xd.ref, D, 1.0 / nb,
                                       ptr(lse), ptr(O), ptr(rr), ptr(dU), None, 0.0, None, None, None, ptr(ws),
                                       ws.numel(), stream_of(Ud)), "hvae_decoder_train")
        _assert_no_flag(ws, nsplit, nb)
        return lse, O, rr, dU

    lse, O, rr, dU = train(True, True)
    lse_b, O_b = ops.decoder_fwd(Ud, Ek, enorm)
    rr_b, dU_b = ops.decoder_bwd(xd, Ud, Ed, lse_b, O_b, 1.0 / nb)
    assert torch.equal(lse, lse_b) and torch.equal(rr, rr_b) and torch.equal(dU, dU_b) and torch.equal(O, O_b)
    _, _, rr2, dU2 = train(False, True)  # O kept internal
    assert torch.equal(rr2, rr) and torch.equal(dU2, dU)
    _, _, rr3, _ = train(False, False)  # the sweep without O
    assert torch.equal(rr3, rr)
    u_ = U.clone().requires_grad_(True)
    rr_t = -(x * torch.log_softmax(u_ @ Ed.cpu().t(), 1)).sum(1)
    rr_t.mean().backward()
    rr_err, du_err = _maxrel(rr, rr_t), _maxrel(dU, u_.grad)
    print(f"nb {nb} N {N} splits {nsplit}: recon maxrel {rr_err:.3g}, dU maxrel {du_err:.3g}")
    assert rr_err < 3e-3
    assert du_err < 2e-2
