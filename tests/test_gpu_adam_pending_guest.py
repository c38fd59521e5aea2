"""hvae_adam_lazy_pending_guest (csrc/hvae_adam_guest.hip) against hvae_adam_lazy_pending: from one saved state -- p,
m, v, last_step, the step table and a recorded update -- each runs on its own copy, and p, m, v and last_step must be
bitwise equal. The state is written by hand, so that every branch is reached at the smallest shapes:

  H in {4, 260, 512}   two lanes of one pass; two passes and a partial third; four full passes (float2 columns)
  N in {257, 65536}    sweep period 8 and 32 (the large N at H = 4)
  recorded rows        0, 1, 65 (more than kGuestRows blocks' worth, not a multiple of it)
  staleness            0, 1, 4, 5 steps (across kTabAhead = 4) and the full period, of recorded rows and of the range
  p ahead              rows whose p the CSR catch-up moved ahead of m and v (weight decay 0 only: with weight decay
                       the catch-up never moves p alone)
  claimed              recorded rows a catch-up already took (no bit 30), and rows whose pend_slot names another slot:
                       neither may move
  weight decay         0 and 0.01

and, on the result, a second run (nothing moves) and a stale header (*step_dev != hdr->t: nothing moves); and with
max_rows below the recorded count (0, 1, 7, 64 of 65), where both kernels must still take every recorded row.

Then two tiny FusedTrainer runs (d = 768, bf16) with HVAE_DEFER_AT=guest and with "sweep", each in a fresh child
process, parameters, moments and losses bitwise equal: 3,000 items, B = 512, 6 graph-replayed steps; and a whole epoch
of two full batches of 2,048 and a deferring tail of 512 over 20,000 items, where the tail step applies the last full
batch's record with a grid hint smaller than the record.
"""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
STEP_MASK = (1 << 24) - 1
PEND_BIT = 1 << 30
T = 41  # the recorded step: past the longest period, so that every staleness has room
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8


def _state(dev, N, H, R, wd, seed):
    """The saved state: tensors on the device and the host-side lists the checks use."""
    from hvae import _lib
    L = _lib.lib()
    rng = np.random.default_rng(seed)
    period = int(L.hvae_adam_lazy_sweep_period(N))
    stales = [0, 1, 4, 5, period]
    f = dict(dtype=torch.float32, device=dev)
    p = torch.from_numpy(rng.standard_normal(N * H).astype(np.float32) * 0.1).to(dev)
    m = torch.from_numpy(rng.standard_normal(N * H).astype(np.float32) * 0.01).to(dev)
    v = torch.from_numpy((rng.standard_normal(N * H).astype(np.float32) * 0.01) ** 2).to(dev)
    # tab[s] = (lr / (1 - b1^s), 1 / sqrt(1 - b2^s)) in double, rounded to fp32 (adam_step_consts)
    tab = np.zeros((64, 2), dtype=np.float32)
    for s in range(1, 64):
        tab[s] = (LR / (1.0 - BETAS[0] ** s), 1.0 / np.sqrt(1.0 - BETAS[1] ** s))
    tab = torch.from_numpy(tab.reshape(-1)).to(dev)
    # every row current at T unless set otherwise below
    last = np.full(N, T, dtype=np.int64)
    chunk = (N + period - 1) // period
    r0 = ((T - 1) % period) * chunk
    r1 = min(N, r0 + chunk)
    # the sweep range: staleness cycles; every third stale row has p moved ahead (to T: the catch-up's p-only form)
    for i, j in enumerate(range(r0, r1)):
        st = stales[i % len(stales)]
        mv = T - st
        ahead = st if (wd == 0.0 and st and i % 3 == 0) else 0
        last[j] = mv | (ahead << 24)
    # the recorded rows: spread over the items, some inside the sweep range (which must skip them: bit 30)
    items = rng.choice(N, size=R, replace=False).astype(np.int64) if R else np.zeros(0, np.int64)
    if R > 2:
        items[0] = r0  # a recorded row inside the range
        items = np.unique(items)
        rng.shuffle(items)
    R = len(items)
    pend_item = np.zeros(N, dtype=np.int32)
    pend_slot = np.zeros(N, dtype=np.int32)
    kinds = []
    for s, j in enumerate(items):
        st = stales[s % len(stales)]
        mv = T - 1 - st
        ahead = st if (wd == 0.0 and st and s % 3 == 1) else 0  # p at T - 1: the last step's catch-up moved it
        kind = "claimed" if s % 7 == 5 else "other_slot" if s % 7 == 6 else "open"
        pend_item[s] = j
        pend_slot[j] = s if kind != "other_slot" else (s + 1) % max(R, 2)
        last[j] = T if kind == "claimed" else (mv | (ahead << 24) | PEND_BIT)
        kinds.append(kind)
    grad = torch.from_numpy(rng.standard_normal((max(R, 1), H)).astype(np.float32)).to(dev)
    coef = np.float32(0.37)
    hdr = np.zeros(4, dtype=np.int64)
    hdr[0], hdr[1], hdr[2] = T, grad.data_ptr(), H
    hdr[3] = (int(R) << 32) | int(np.frombuffer(coef.tobytes(), dtype=np.uint32)[0])
    return dict(N=N, H=H, R=R, wd=wd, period=period, p=p, m=m, v=v, tab=tab, grad=grad,
                last=torch.from_numpy(last.astype(np.int32)).to(dev), hdr=torch.from_numpy(hdr).to(dev),
                pend_item=torch.from_numpy(pend_item).to(dev), pend_slot=torch.from_numpy(pend_slot).to(dev),
                step=torch.full((1,), T, dtype=torch.int64, device=dev), items=items, kinds=kinds, range=(r0, r1))


def _run(S, fn_name, p, m, v, last, step=None, max_rows=None):
    from hvae import _lib, ops
    L = _lib.lib()
    cfg = ops.adam_config(LR, BETAS, EPS, S["wd"], S["step"] if step is None else step, None)
    pend = _lib.AdamPend(S["pend_slot"].data_ptr(), S["pend_item"].data_ptr(), S["hdr"].data_ptr())
    st = torch.cuda.current_stream(p.device).cuda_stream
    _lib.check(getattr(L, fn_name)(C.byref(cfg), S["tab"].data_ptr(), p.data_ptr(), m.data_ptr(), v.data_ptr(),
                                   last.data_ptr(), S["N"], S["H"], S["N"] if max_rows is None else max_rows,
                                   C.byref(pend), st), fn_name)
    torch.cuda.synchronize()


def _bits(t):
    return t.view(torch.int32)


CASES = [(257, H, R, wd) for H in (4, 260, 512) for R in (0, 1, 65) for wd in (0.0, 0.01)] + \
        [(65536, 4, R, wd) for R in (0, 1, 65) for wd in (0.0, 0.01)]


@pytest.mark.parametrize("N,H,R,wd", CASES)
def test_guest_is_bitwise_the_pending_kernel(hip_device, N, H, R, wd):
    S = _state(hip_device, N, H, R, wd, seed=N + 7 * H + 31 * R + (1 if wd else 0))
    ref = [S[k].clone() for k in ("p", "m", "v", "last")]
    got = [S[k].clone() for k in ("p", "m", "v", "last")]
    _run(S, "hvae_adam_lazy_pending", *ref, max_rows=max(S["R"], 1))
    _run(S, "hvae_adam_lazy_pending_guest", *got, max_rows=max(S["R"], 1))
    for name, a, b in zip(("p", "m", "v", "last_step"), ref, got):
        bad = int((_bits(a) != _bits(b)).sum())
        assert bad == 0, f"{name}: {bad} words differ from hvae_adam_lazy_pending's"
    # the state reached every branch it was written for, and the reference moved what it should
    last0, last1 = S["last"].cpu().numpy().astype(np.int64), got[3].cpu().numpy().astype(np.int64)
    r0, r1 = S["range"]
    moved = _bits(got[0]).view(N, H).ne(_bits(S["p"]).view(N, H)).any(1).cpu().numpy() | \
        _bits(got[1]).view(N, H).ne(_bits(S["m"]).view(N, H)).any(1).cpu().numpy()
    for s, (j, kind) in enumerate(zip(S["items"], S["kinds"])):
        if kind == "open":
            assert last1[j] == T and moved[j], (s, j, kind)
        else:  # claimed by a catch-up, or recorded under another slot: untouched
            assert last1[j] == last0[j] and not moved[j], (s, j, kind)
    rng = np.arange(r0, r1)
    plain = rng[(last0[rng] & PEND_BIT) == 0]
    assert np.all(last1[plain] == T)
    stale = plain[(last0[plain] & STEP_MASK) < T]
    assert len(stale) > 0 and np.all(moved[stale]), "no stale row in the sweep range moved"
    outside = np.setdiff1d(np.setdiff1d(np.arange(N), rng), S["items"])
    assert not moved[outside].any() and np.array_equal(last1[outside], last0[outside])
    # a second run finds nothing left to do
    again = [t.clone() for t in got]
    _run(S, "hvae_adam_lazy_pending_guest", *again, max_rows=max(S["R"], 1))
    for name, a, b in zip(("p", "m", "v", "last_step"), got, again):
        assert torch.equal(_bits(a), _bits(b)), f"a second run changed {name}"
    # a stale header (the counter has moved on): nothing moves
    idle = [S[k].clone() for k in ("p", "m", "v", "last")]
    _run(S, "hvae_adam_lazy_pending_guest", *idle, step=S["step"] + 1, max_rows=max(S["R"], 1))
    for name, k, b in zip(("p", "m", "v", "last_step"), ("p", "m", "v", "last"), idle):
        assert torch.equal(_bits(S[k]), _bits(b)), f"a stale record moved {name}"


@pytest.mark.parametrize("max_rows", [0, 1, 7, 64])
def test_guest_takes_rows_recorded_beyond_max_rows(hip_device, max_rows):
    """max_rows is a grid-size hint, as for hvae_adam_lazy_pending: with fewer row blocks than the 65 recorded rows
    need (none spare, one group, two groups with a partial one, one row short) the blocks stride over all of them."""
    S = _state(hip_device, 257, 260, 65, 0.0, seed=5)
    assert S["R"] > max_rows
    full = [S[k].clone() for k in ("p", "m", "v", "last")]
    _run(S, "hvae_adam_lazy_pending", *full)  # max_rows = N
    for fn in ("hvae_adam_lazy_pending", "hvae_adam_lazy_pending_guest"):
        got = [S[k].clone() for k in ("p", "m", "v", "last")]
        _run(S, fn, *got, max_rows=max_rows)
        for name, a, b in zip(("p", "m", "v", "last_step"), full, got):
            bad = int((_bits(a) != _bits(b)).sum())
            assert bad == 0, f"{fn}(max_rows={max_rows}) {name}: {bad} words differ from the full grid's"
    assert int((got[3] & PEND_BIT).ne(0).sum()) == S["kinds"].count("other_slot")  # only those keep bit 30


def test_guest_fits_beside_the_d768_bf16_sweep(hip_device):
    """The loaded code objects say the guest fits beside the flagship sweep (4096 x 1,000,000, d = 768, bf16), and
    the query says no where it cannot read the sweep's footprint (d = 384)."""
    from hvae import _lib
    L = _lib.lib()
    assert L.hvae_adam_pending_guest_fits(_lib.HVAE_BF16, 4096, 1_000_000, 768) == 1
    assert L.hvae_adam_pending_guest_fits(_lib.HVAE_BF16, 512, 3000, 768) == 1
    assert L.hvae_adam_pending_guest_fits(_lib.HVAE_BF16, 4096, 100_000, 384) == 0


_CHILD = r"""
import json, os, sys
import numpy as np, torch
sys.path[:0] = [{root!r}, {pkg!r}, {golden!r}]
from gen import synth_csr, synth_embeddings
from hvae.executor import ConstBeta, FusedTrainer
from src.ml.model import HybridVAE
dev = torch.device("cuda", 0)
cfg = json.loads(sys.argv[2])
n_users, n_items, d, B, steps = cfg["users"], cfg["items"], 768, cfg["B"], cfg["steps"]
X = synth_csr(n_users, n_items, seed=11)
E = synth_embeddings(n_items, d, seed=12)
torch.manual_seed(0)
model = HybridVAE(n_items, E, latent_dim=64, hidden_dims=[512], dropout=0.3, beta=0.2).to(dev)
fused = FusedTrainer(model, dev, lr=1e-3, precision="bf16", seed=1234, use_graphs=True)
data = fused.device_data(X, list(range(n_users)))
gen = torch.Generator(device=dev).manual_seed(0)
# steps None: the whole epoch in order, its tail batch included (no shuffle, so the test knows the batches)
out = fused.run_epoch(data, B, steps is not None, ConstBeta(0.2), 0.3, generator=gen, max_batches=steps)
fused.flush()
torch.cuda.synchronize()
np.savez(sys.argv[1], flat=fused.flat.cpu().numpy(), m=fused.m.cpu().numpy(), v=fused.v.cpu().numpy(),
         loss=np.array([out["total_loss"], out["recon_loss"], out["kl_loss"]], dtype=np.float64))
tail = n_users % B
n_full = n_users // B
last_full = X[(n_full - 1) * B:n_full * B]
print(json.dumps({{"defers": bool(fused._defers(B)), "guest": bool(fused._use_guest(B)),
                  "step": int(fused.step_dev.item()), "tail": tail,
                  "tail_defers": bool(tail and fused._defers(tail)), "tail_guest": bool(tail and fused._use_guest(tail)),
                  "tail_cap": int(data.max_batch_nnz(tail)) if tail else 0,
                  "last_full_unique": int(np.unique(last_full.indices).size)}}))
"""


def _children(tmp_path, cfg):
    code = _CHILD.format(root=str(ROOT), pkg=str(ROOT / "recommendation-system_amd"),
                         golden=str(ROOT / "tests" / "golden"))
    res, infos = {}, {}
    for at in ("guest", "sweep"):
        env = dict(os.environ, HVAE_DEFER_AT=at, HVAE_ADAM_DEFER="1", HVAE_MLP_ROWS="0")
        out = tmp_path / f"{at}.npz"
        r = subprocess.run([sys.executable, "-c", code, str(out), json.dumps(cfg)], env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, (at, r.returncode, r.stderr[-3000:])
        infos[at] = json.loads(r.stdout.strip().splitlines()[-1])
        res[at] = dict(np.load(out))
    return res, infos


def _same_results(res):
    for k in ("flat", "m", "v", "loss"):
        a, b = res["guest"][k], res["sweep"][k]
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{k} differs between the placements"


def test_trainer_with_guest_placement_is_bitwise_sweep_placement(hip_device, tmp_path):
    res, infos = _children(tmp_path, dict(users=6 * 512, items=3000, B=512, steps=6))
    for at, info in infos.items():
        assert info["defers"] and info["step"] == 6, info
        assert info["guest"] == (at == "guest"), info  # the guest arm really ran the guest kernel
    _same_results(res)


def test_trainer_tail_batch_takes_the_full_batch_record(hip_device, tmp_path):
    """An epoch whose user count is no multiple of the batch size: two full batches of 2,048 and a deferring tail of
    512. The tail step applies the last full batch's record with buffers sized for the tail, so the guest's max_rows
    (5,675, the 512 longest rows' entries) is below the rows recorded (7,248); every one must still be taken."""
    res, infos = _children(tmp_path, dict(users=2 * 2048 + 512, items=20000, B=2048, steps=None))
    for at, info in infos.items():
        assert info["defers"] and info["tail"] == 512 and info["tail_defers"] and info["step"] == 3, info
        assert info["guest"] == info["tail_guest"] == (at == "guest"), info
        # the case bites: more rows recorded by the last full batch than the tail step's grid hint
        assert info["last_full_unique"] > info["tail_cap"], info
    _same_results(res)
