"""The d = 768 bf16 sweep (k_dec5_bf16) after its consumer waves were re-mapped: consumer c owns all 64 users of
the block over D quarter c, refills the item-half-0 rows of its own quarter of slot t % 3 with tile t + 3 as soon
as its MFMAs have consumed them, and waits for those pieces with vmcnt(DEC5_DMA_B) two barriers later. Its
steady-state loop therefore ends three tiles before the split's end, so splits of 1 .. 5 tiles are the counts that
can go wrong.

Users 1, 32, 33, 64, 65, 97: an empty second user group, a group boundary inside a consumer's 64 users, a second
user block. Items 31 .. 4097: splits of exactly 1, 2, 3, 4, 5, 6 and >= 7 tiles, a last split of each of those
sizes whose final tile is partial, N % 32 in {0, 1, 5, 31} -- asserted from the library's split rule (restated in
tests/golden/make_dec5_regionfill_fixture.py and checked against hvae_decoder_workspace in every call). The rule
never makes a split without tiles; the test asserts that as well instead of trying to make one.

Every call gets a workspace filled with 0xFF bytes and no user may come out flagged. The bounds are
tests/test_gpu_dec5_tileloop.py's. The re-mapping moved MFMAs between waves and reordered no sum, so lse (whole
grid), and O and the flag words (O_CASES), must equal tests/golden/dec5_regionfill_parent.npz, recorded on the
commit before it, bit for bit.
"""
from pathlib import Path

import numpy as np
import pytest
import torch

from gen import synth_csr, synth_embeddings
from make_dec5_regionfill_fixture import D, NBS, NS, O_CASES, cdiv, split_tiles, sweep, users

pytestmark = pytest.mark.gpu

FIXTURE = Path(__file__).resolve().parent / "golden" / "dec5_regionfill_parent.npz"


@pytest.fixture(scope="module")
def ops(hip_device):
    from hvae import ops
    return ops


@pytest.fixture(scope="module")
def parent():
    return dict(np.load(FIXTURE, allow_pickle=False))


def _maxrel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / max(b.abs().max().item(), 1e-30))


def test_cases_cover_the_tile_counts_and_tails():
    """Splits of exactly 1 .. 6 and >= 7 tiles, never 0; a last split of each size ending in a partial tile;
    N % 32 of 0, 1, 5 and 31."""
    seen, partial_last = set(), set()
    for nb in NBS:
        for N in NS:
            counts = split_tiles(nb, N)
            assert min(counts) >= 1 and sum(counts) == cdiv(N, 32)
            seen |= {min(c, 7) for c in counts}
            if N % 32:
                partial_last.add(min(counts[-1], 7))
    assert seen == {1, 2, 3, 4, 5, 6, 7}
    assert partial_last == {1, 2, 3, 4, 5, 6, 7}
    assert {N % 32 for N in NS} >= {0, 1, 5, 31}


def test_fixture_holds_the_grid(parent):
    want = {f"lse_{nb}_{N}" for nb in NBS for N in NS}
    want |= {f"{k}_{nb}_{N}" for nb, N in O_CASES for k in ("O", "flag")}
    assert set(parent) == want


@pytest.fixture(scope="module")
def items(hip_device, ops):
    """Per N: the bf16 image, its norm bound, the fp32 E on the device and the bf16-rounded E in float64."""
    out = {}
    for N in NS:
        Ed = torch.as_tensor(synth_embeddings(N, D, seed=N)).to(hip_device)
        Ek = ops.decoder_image(Ed)
        out[N] = (Ek, ops.row_norm_max(Ek), Ed, Ek.bf16.float().cpu().double())
    return out


def _assert_no_flag(flags, S, nb):
    assert flags.numel() == S * nb
    assert int((flags == 1).sum()) == 0, "the sweep flagged a user"
    assert int((flags == 0).sum()) == S * nb, "a split left a user's flag unwritten"


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("nb", NBS)
def test_dec5_forward(ops, hip_device, items, parent, nb, N):
    """decoder_fwd with and without O: float64 on the bf16-rounded operands, the parent's recorded bits, a poisoned
    workspace, no user flagged."""
    Ek, enorm, _, Er = items[N]
    U = users(nb)
    Ud = U.to(hip_device)
    S = U.bfloat16().double() @ Er.t()
    lse_ref = torch.logsumexp(S, 1)
    O_ref = torch.softmax(S, 1) @ Er
    nsplit = len(split_tiles(nb, N))
    lse, O, flags = sweep(ops, hip_device, Ek, enorm, Ud, nb, N)
    _assert_no_flag(flags, nsplit, nb)
    lse_err = float((lse.double().cpu() - lse_ref).abs().max())
    o_err = _maxrel(O, O_ref)
    print(f"nb {nb} N {N} splits {nsplit}: lse err {lse_err:.3g}, O maxrel {o_err:.3g}")
    assert torch.isfinite(lse).all() and torch.isfinite(O).all()
    assert lse_err < 2e-3 * max(1.0, lse_ref.abs().max().item())
    assert o_err < 1e-2
    assert torch.equal(lse.cpu(), torch.from_numpy(parent[f"lse_{nb}_{N}"]))
    if (nb, N) in O_CASES:
        assert torch.equal(O.cpu(), torch.from_numpy(parent[f"O_{nb}_{N}"]))
        assert torch.equal(flags.cpu(), torch.from_numpy(parent[f"flag_{nb}_{N}"]))
    lse2, _, flags2 = sweep(ops, hip_device, Ek, enorm, Ud, nb, N, with_o=False)
    _assert_no_flag(flags2, nsplit, nb)
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
    nsplit = len(split_tiles(nb, N))
    ws = torch.empty(int(lib().hvae_decoder_workspace(dt, nb, N, D)), dtype=torch.uint8, device=hip_device)

    def train(want_o, want_du):
        ws.fill_(0xFF)
        lse = torch.empty(nb, device=hip_device)
        O = torch.empty(nb, D, device=hip_device) if want_o else None
        rr = torch.empty(nb, device=hip_device)
        dU = torch.empty(nb, D, device=hip_device) if want_du else None
        check(lib().hvae_decoder_train(dt, ptr(Ud), Ud.stride(0), ptr(Eh), ptr(enorm), ptr(Ed), xd.ref, D, 1.0 / nb,
                                       ptr(lse), ptr(O), ptr(rr), ptr(dU), None, 0.0, None, None, None, ptr(ws),
                                       ws.numel(), stream_of(Ud)), "hvae_decoder_train")
        _assert_no_flag(ws[:nsplit * nb * 4].view(torch.int32), nsplit, nb)
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
