"""hvae_topk_fused run from its plan (hvae_topk_fused_plan) at every served width, over the shapes at which the plan
changes: one split (N = 31) and several (6 at N = 777, 32 at N = 4097), a partial user block on either side of the
block size (64 users at d = 1024, 128 elsewhere: R = 1, 33, 65, 129), a partial last tile (all three N). Each call
goes through ctypes with a workspace of exactly plan.workspace bytes, poisoned with 0xFF and followed by a 4 KiB 0xFF
guard in the same allocation: the guard stays untouched, no row is flagged, and the result passes
tests/test_gpu_topk.py's float64 check with that file's tolerance."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

from gen import synth_csr, synth_embeddings
from test_gpu_topk import _check

pytestmark = pytest.mark.gpu

WIDTHS = (64, 128, 256, 384, 512, 768, 1024)
RS, NS, K = (1, 33, 65, 129), (31, 777, 4097), 5
SPLITS = {31: 1, 777: 6, 4097: 32}  # min(cdiv(256, user blocks), max(1, tiles / 4)) of the rule
GUARD = 4096


@lru_cache(maxsize=None)
def _inputs(N, D):
    """E [N, D] and U [max(RS), D] on the host, shared by every case of (N, D): a case takes U's first R rows."""
    E = torch.as_tensor(synth_embeddings(N, D, seed=N + D))
    U = torch.randn(max(RS), D, generator=torch.Generator().manual_seed(N + D + 1)) * (4.0 / D ** 0.5)
    return E, U


def _run(dev, R, N, D, exclude=None):
    from hvae import ops
    from hvae._lib import TOPK_SCANS, TopkPlan, check, lib, ptr, stream_of
    E, U = _inputs(N, D)
    U = U[:R].contiguous()
    p = TopkPlan()
    check(lib().hvae_topk_fused_plan(R, N, D, K, C.byref(p)), "hvae_topk_fused_plan")
    bu = 64 if D == 1024 else 128
    assert TOPK_SCANS[p.scan] == ("global" if D == 64 else "lds_kh2" if D == 1024 else "lds") and p.wave_users == 1
    assert (p.block_users, p.splits, p.blocks) == (bu, SPLITS[N], -(-R // bu) * SPLITS[N])
    assert p.tiles_per_split * p.splits >= -(-N // 32) and N % 32 != 0
    assert p.full_splits * p.tiles_per_split + (p.splits - p.full_splits) * (p.tiles_per_split - 1) == -(-N // 32)
    assert p.workspace == lib().hvae_topk_fused_workspace(R, N, D, K)
    Ud, Ed = U.to(dev), E.to(dev)
    img, emax = ops.decoder_image(Ed), ops.row_norm_max(Ed)
    ws = torch.full((p.workspace + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    idx = torch.empty(R, K, dtype=torch.int32, device=dev)
    val = torch.empty(R, K, device=dev)
    flag = torch.empty(R, dtype=torch.int32, device=dev)
    check(lib().hvae_topk_fused(ptr(Ud), Ud.stride(0), ptr(img.bf16), ptr(Ed), ptr(emax), N, D,
                                exclude.ref if exclude is not None else None, R, K, ptr(idx), ptr(val), ptr(flag),
                                ptr(ws), p.workspace, stream_of(Ud)), "hvae_topk_fused")
    torch.cuda.synchronize()
    assert bool((ws[p.workspace:] == 0xFF).all()), "the call wrote past plan.workspace bytes"
    assert int(flag.sum()) == 0
    return idx, val, U, E


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("D", WIDTHS)
def test_topk_fused_runs_from_its_plan(hip_device, D, R, N):
    idx, val, U, E = _run(hip_device, R, N, D)
    _check(idx, val, U, E, K)


@pytest.mark.parametrize("D", WIDTHS)
def test_topk_fused_runs_from_its_plan_with_seen_items(hip_device, D):
    from hvae import ops
    R, N = 33, 777
    X = synth_csr(R, N, lam=10.0, seed=D)  # about 10 seen items per row
    csr = ops.csr_from_scipy(X, hip_device)
    ex = ops.Csr(csr.row_ptr, csr.col_idx, csr.vals, N, rows=torch.arange(R, dtype=torch.int32, device=hip_device))
    idx, val, U, E = _run(hip_device, R, N, D, exclude=ex)
    _check(idx, val, U, E, K, [torch.as_tensor(X[r].indices.astype(np.int64)) for r in range(R)])
