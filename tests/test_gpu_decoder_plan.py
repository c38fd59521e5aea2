"""hvae_decoder_fwd runs the plan hvae_decoder_plan names, for every product sweep that writes flag words.

Each call gets a workspace of exactly plan.workspace bytes filled with 0xFF (flag words -1, floats NaN). The
workspace starts with one flag word per (split, user), padded to 256 bytes: after the call the first
splits * nb words are 0 (written, no user flagged for the exact recomputation), and the pad words behind them are
still -1, so the sweep ran with the plan's split count and not a larger one. Then the same call with one byte less
and the plan queried for that size: the smaller splits * nb flags, the same tolerances (test_gpu_kernels.py's for
bf16 and fp32, test_gpu_fp8.py's for fp8, against float64 on the rounded / quantised operands).

nb = 64 takes bf16_v2's ds = 2 form below 512; nb = 130 takes ds = 1 and leaves a partial user block. The pad is
non-empty at nb = 130 (asserted); at nb = 64 a split's flags are 256 bytes, so there the pad is empty whatever the
split count is (asserted too) and only the flag words themselves are checked. fp32 writes no flags and is checked
against float64 only.
"""
import ctypes as C

import pytest
import torch

from gen import synth_embeddings

pytestmark = pytest.mark.gpu

N = 2001
NBS = (64, 130)
CASES = [("bf16", D) for D in (64, 384, 512, 768, 1024)] + [("fp8", D) for D in (384, 768)] + [("f32", 64)]
SWEEP = {("bf16", 768): "bf16_v5", ("fp8", 768): "fp8_v5", ("fp8", 384): "fp8_ring", ("f32", 64): "f32"}


@pytest.fixture(scope="module")
def ops(hip_device):
    from hvae import ops
    return ops


@pytest.fixture(scope="module")
def operands(hip_device, ops):
    """Per (dtype, D), built once: the image, its norm bound and the rounded E (float64, CPU) the sweep multiplies."""
    from hvae import _lib
    out = {}

    def get(dtype, D):
        if (dtype, D) not in out:
            E = torch.as_tensor(synth_embeddings(N, D, seed=N))
            Ed = E.to(hip_device)
            if dtype == "fp8":
                from test_gpu_fp8 import _quantised
                img = ops.decoder_image(Ed, _lib.HVAE_FP8)
                Er = _quantised(E, torch.ones(1, D))[0].double()
            elif dtype == "bf16":
                img = ops.decoder_image(Ed)
                Er = img.bf16.float().cpu().double()
            else:
                img, Er = Ed, E.double()
            out[dtype, D] = (img, ops.row_norm_max(img), Er)
        return out[dtype, D]

    return get


def _plan(dt, nb, D, ws_bytes):
    from hvae._lib import DEC_SWEEPS, DecPlan, check, lib
    p = DecPlan()
    check(lib().hvae_decoder_plan(dt, nb, N, D, ws_bytes, C.byref(p)), "hvae_decoder_plan")
    return p, DEC_SWEEPS[p.sweep]


@pytest.mark.parametrize("nb", NBS)
@pytest.mark.parametrize("dtype,D", CASES)
def test_fwd_runs_the_plan(ops, hip_device, operands, dtype, D, nb):
    from hvae._lib import check, lib, ptr, stream_of
    img, enorm, Er = operands(dtype, D)
    U = torch.randn(nb, D, generator=torch.Generator().manual_seed(nb)) * 3.0
    Ud = U.to(hip_device)
    if dtype == "fp8":
        from test_gpu_fp8 import _o_envelope, _quantised
        Ur = _quantised(torch.ones(1, D), U)[1].double()
    else:
        Ur = (U.bfloat16() if dtype == "bf16" else U).double()
    S = Ur @ Er.t()
    lse_ref = torch.logsumexp(S, 1)
    O_ref = torch.softmax(S, 1) @ Er
    dt, _, Eh = ops._dec_operand(img)

    full, sweep = _plan(dt, nb, D, 2 ** 64 - 1)
    assert sweep == SWEEP.get((dtype, D), "bf16_v2")
    assert full.workspace == lib().hvae_decoder_workspace(dt, nb, N, D) and full.splits > 1
    if sweep == "bf16_v2":
        assert full.ds == (4 if D == 1024 else 2 if (D > 384 or nb <= 64) else 1)
    short, sweep_short = _plan(dt, nb, D, full.workspace - 1)
    assert sweep_short == sweep and 1 <= short.splits < full.splits

    for plan, ws_bytes in ((full, full.workspace), (short, full.workspace - 1)):
        ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device=hip_device)
        lse = torch.empty(nb, device=hip_device)
        O = torch.empty(nb, D, device=hip_device)
        check(lib().hvae_decoder_fwd(dt, ptr(Ud), Ud.stride(0), ptr(Eh), ptr(enorm), nb, N, D, ptr(lse), ptr(O),
                                     ptr(ws), ws_bytes, stream_of(Ud)), "hvae_decoder_fwd")
        if dtype != "f32":
            nflag = plan.splits * nb
            npad = -(-nflag * 4 // 256) * 64 - nflag
            assert (npad > 0) == (nb == 130), "the pad is empty exactly where a split's flags fill 256 bytes"
            words = ws[:(nflag + npad) * 4].view(torch.int32).cpu()
            assert int((words[:nflag] == 0).sum()) == nflag, "a (split, user) flag is unwritten, or a user is flagged"
            assert int((words[nflag:] == -1).sum()) == npad, "the sweep wrote flags past the plan's splits * nb"
        lse_err = float((lse.double().cpu() - lse_ref).abs().max())
        o_err = (O.double().cpu() - O_ref).abs()
        o_rel = float(o_err.max() / max(O_ref.abs().max().item(), 1e-30))
        print(f"{dtype} D {D} nb {nb} splits {plan.splits}: lse err {lse_err:.3g}, O maxrel {o_rel:.3g}")
        assert torch.isfinite(lse).all() and torch.isfinite(O).all()
        scale = max(1.0, lse_ref.abs().max().item())
        if dtype == "fp8":
            assert lse_err < 2e-4 * scale
            assert (o_err <= _o_envelope(S, Er)).all(), float((o_err / _o_envelope(S, Er)).max())
        else:
            assert lse_err < (1e-5 if dtype == "f32" else 2e-3) * scale
            assert o_rel < (1e-5 if dtype == "f32" else 1e-2)
