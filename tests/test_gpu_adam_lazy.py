"""The lazy-Adam kernel family (csrc/hvae_optim.hip, csrc/hvae_adam.h) driven through the C ABI, without the trainer
and without the row-gradient plan: hvae_adam_lazy, hvae_adam_lazy_catchup, hvae_adam_lazy_catchup_csr and the
deferred trio hvae_adam_lazy_defer / hvae_adam_lazy_catchup_csr_pending / hvae_adam_lazy_pending.

A host-side schedule says which W1t rows get a gradient at which step (tests/adam_lazy_ref.py); the row-gradient
buffers (rows, item_of, slot_of, n_unique) and the catch-ups' CSR batches are filled by hand from it, earlier steps'
slot_of entries left in place (the kernels reject them through item_of[slot] == row). Every case runs three arms on
identical inputs:

  lazy    the code under test, in the trainer's order per step: catch-up of the batch (from its CSR, or from the row
          list), hvae_adam_lazy, step counter advanced -- by hvae_counter_add, or in half the cases by
          hvae_clip_grad_norm_step_adam before the update, so that tab[t] is pre-written instead of written by
          k_adam_lazy itself -- and a catch-up over all rows at the end;
  dense   hvae_adam_flat over every row every step: p, m, v must be bitwise the lazy arm's (include/hvae.h: "bitwise
          equal to updating eagerly") at the end and at two mid-run points (on clones of the lazy state caught up over
          all rows: the live state keeps its lags);
  anchor  torch's single-tensor Adam restated in float64 on the CPU, every row every step. Both GPU arms must stay
          within 4 x the deviation that torch.optim.Adam itself (CPU, float32) has from it, figure by figure.

last_step is checked structurally after every update: no row lags more than hvae_adam_lazy_sweep_period(N) steps,
bit 30 is set only on the rows of an open deferred record, and after the final catch-up every entry is the step count.
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import adam_lazy_ref as A  # noqa: E402

pytestmark = pytest.mark.gpu

STEP_MASK = (1 << 24) - 1
PEND_BIT = 1 << 30


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


class Harness:
    """The device state of one case: the lazy arm (p, m, v, last_step, step table, step counters, the deferred
    record), the dense arm (pd, md, vd, its own counter) and the shared row-gradient buffers."""

    def __init__(self, dev, N, H, n_dense=0, dense_mis=0, tab_len=256, defer=False, max_rows=None):
        from hvae import _lib, ops
        self.ops, self._lib, self.L = ops, _lib, _lib.lib()
        self.dev, self.N, self.H, self.nd = dev, N, H, n_dense
        self.NH = N * H
        self.dense_off = self.NH + dense_mis  # dense_mis = 1: the dense segment off 16-byte alignment
        total = self.dense_off + n_dense + 4
        f = dict(dtype=torch.float32, device=dev)
        self.p, self.m, self.v = (torch.zeros(total, **f) for _ in range(3))
        self.pd, self.md, self.vd = (torch.zeros(total, **f) for _ in range(3))
        self.last = torch.zeros(N, dtype=torch.int32, device=dev)
        self.tab_len = tab_len
        self.tab = torch.zeros(2 * tab_len, **f)
        i64 = dict(dtype=torch.int64, device=dev)
        self.step, self.snap, self.step_d = (torch.zeros(1, **i64) for _ in range(3))
        self.coef = torch.ones(1, **f)
        self.norm, self.coef_clip = torch.zeros(1, **f), torch.zeros(1, **f)
        self.ws = torch.zeros(8192, dtype=torch.uint8, device=dev)
        self.rg = ops.RowGradBuffers(N, H, N, dev)
        self.rg.rows_from_elsewhere()  # the rows are written here, not by the row-gradient apply
        self.gd = torch.zeros(max(n_dense, 4), **f)
        self.period = int(self.L.hvae_adam_lazy_sweep_period(N))
        self.defer = defer
        self.max_rows = N if max_rows is None else max_rows
        self.pend_open = False
        self.seen = {"claimed": 0, "left": 0, "p_only_in_sweep": 0}  # run(): what the deferred cases reached
        if defer:
            self.pend_slot = torch.zeros(N, dtype=torch.int32, device=dev)
            self.pend_item = torch.zeros(N, dtype=torch.int32, device=dev)
            self.pend_hdr = torch.zeros(4, **i64)
            self.pend = _lib.AdamPend(self.pend_slot.data_ptr(), self.pend_item.data_ptr(), self.pend_hdr.data_ptr())

    # ---- plumbing
    @property
    def st(self):
        return torch.cuda.current_stream(self.dev).cuda_stream

    def cfg(self, pb, step_t, coef=False):
        return self.ops.adam_config(pb.lr, pb.betas, pb.eps, pb.wd, step_t,
                                    self.coef if (coef and pb.coef is not None) else None)

    def ck(self, rc, what):
        self._lib.check(rc, what)

    def load(self, pb):
        """Both arms at pb's start state, every row current at step pb.t0."""
        p0, m0, v0 = pb.start()
        for dst2, src in (((self.p, self.pd), p0), ((self.m, self.md), m0), ((self.v, self.vd), v0)):
            s = torch.from_numpy(src).to(self.dev)
            for d in dst2:
                d.zero_()
                d[:self.NH] = s[:self.NH]
                d[self.dense_off:self.dense_off + self.nd] = s[self.NH:]
        self.last.fill_(pb.t0)
        for c in (self.step, self.snap, self.step_d):
            c.fill_(pb.t0)
        self.coef.fill_(float(pb.coef32))
        self.pend_open = False

    def flat(self, t):
        """[W1t rows | dense segment] of a state buffer, on the host."""
        return torch.cat([t[:self.NH], t[self.dense_off:self.dense_off + self.nd]]).cpu().numpy()

    def csr(self, users, rows=None, rows_offset=0):
        """A CSR batch of `users` (lists of item ids), by hand; with `rows`, the batch is those matrix rows from
        rows_offset on (hvae_csr_batch.rows / rows_offset)."""
        ptr_ = np.zeros(len(users) + 1, dtype=np.int64)
        ptr_[1:] = np.cumsum([len(u) for u in users])
        col = np.array([j for u in users for j in u], dtype=np.int32)
        row_ptr = torch.from_numpy(ptr_).to(self.dev)
        col_idx = torch.from_numpy(col if col.size else np.zeros(1, np.int32)).to(self.dev)
        vals = torch.ones(max(col.size, 1), dtype=torch.float32, device=self.dev)
        if rows is None:
            x = self.ops.Csr(row_ptr, col_idx, vals, self.N)
            batch = users
        else:
            r = torch.tensor(rows, dtype=torch.int32, device=self.dev)
            off = torch.tensor([rows_offset], dtype=torch.int64, device=self.dev)
            x = self.ops.Csr(row_ptr, col_idx, vals, self.N, rows=r, nb=len(rows) - rows_offset, rows_offset=off)
            batch = [users[i] for i in rows[rows_offset:]]
        x.listed = np.array(sorted({j for u in batch for j in u}), dtype=np.int64)  # the items the batch lists
        return x

    def set_rows(self, pb, s):
        rows = np.zeros(0, np.int32) if s in pb.no_update else pb.sched[s]
        k = len(rows)
        if k:
            r = torch.from_numpy(np.ascontiguousarray(rows)).to(self.dev)
            self.rg.item_of[:k] = r
            self.rg.slot_of[r.long()] = torch.arange(k, dtype=torch.int32, device=self.dev)
            self.rg.rows[:k] = torch.from_numpy(pb.row_grads(s)).to(self.dev)
        self.rg.n_unique.fill_(k)
        if self.nd and s not in pb.no_update:
            self.gd[:self.nd] = torch.from_numpy(pb.dense_grads(s)).to(self.dev)

    # ---- the kernels
    def catchup_all(self, pb, p, m, v, last):
        self.ck(self.L.hvae_adam_lazy_catchup(C.byref(self.cfg(pb, self.step)), self.tab.data_ptr(), p.data_ptr(),
                                              m.data_ptr(), v.data_ptr(), last.data_ptr(), None, self.N, self.H,
                                              self.st), "adam_lazy_catchup(all)")

    def pending(self, pb, p, m, v, last, max_rows=None):
        self.ck(self.L.hvae_adam_lazy_pending(C.byref(self.cfg(pb, self.step)), self.tab.data_ptr(), p.data_ptr(),
                                              m.data_ptr(), v.data_ptr(), last.data_ptr(), self.N, self.H,
                                              self.max_rows if max_rows is None else max_rows, C.byref(self.pend),
                                              self.st), "adam_lazy_pending")

    def catchup_batch(self, pb, kind, x):
        a = (C.byref(self.cfg(pb, self.step)), self.tab.data_ptr(), self.p.data_ptr(), self.m.data_ptr(),
             self.v.data_ptr(), self.last.data_ptr())
        if kind == "rows":
            self.ck(self.L.hvae_adam_lazy_catchup(*a, self.rg.ref, self.N, self.H, self.st), "adam_lazy_catchup")
        elif self.defer:
            self.ck(self.L.hvae_adam_lazy_catchup_csr_pending(*a, x.ref, self.H, C.byref(self.pend), self.st),
                    "adam_lazy_catchup_csr_pending")
        else:
            self.ck(self.L.hvae_adam_lazy_catchup_csr(*a, x.ref, self.H, self.st), "adam_lazy_catchup_csr")
        if kind == "csr":  # every listed row's p is at the step count now, whoever claimed it
            ls = self.last.cpu().numpy().astype(np.int64)[x.listed]
            p_at = (ls & STEP_MASK) + ((ls >> 24) & 63)
            assert np.all(p_at == int(self.step.item())), "a listed row was not caught up"

    def clip_step(self, pb):
        """hvae_clip_grad_norm_step_adam: snap = step, step += 1, tab[step] written (its own clip multiplier goes to a
        scratch scalar: the case's coef_dev is fixed, so that the anchor knows it)."""
        self.ck(self.L.hvae_clip_grad_norm_step_adam(None, 0, self.rg.ref, self.H, 5.0, self.norm.data_ptr(),
                                                     self.coef_clip.data_ptr(), self.step.data_ptr(),
                                                     self.snap.data_ptr(), None, 0, C.byref(self.cfg(pb, self.snap)),
                                                     self.tab.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                                                     self.st), "clip_grad_norm_step_adam")

    def update(self, pb, use_clip):
        if use_clip:
            self.clip_step(pb)
        cfg = self.cfg(pb, self.snap if use_clip else self.step, coef=True)
        a = (C.byref(cfg), self.tab.data_ptr(), self.tab_len, self.p.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
             self.last.data_ptr(), self.rg.ref, self.H, self.gd.data_ptr() if self.nd else None, self.dense_off,
             self.nd)
        if self.defer:
            self.ck(self.L.hvae_adam_lazy_defer(*a, C.byref(self.pend), self.st), "adam_lazy_defer")
            self.pend_open = True
        else:
            self.ck(self.L.hvae_adam_lazy(*a, self.st), "adam_lazy")
        if not use_clip:
            self.ops.counter_add(self.step, 1)

    def dense_step(self, pb):
        self.ck(self.L.hvae_adam_flat(C.byref(self.cfg(pb, self.step_d, coef=True)), self.pd.data_ptr(),
                                      self.md.data_ptr(), self.vd.data_ptr(), self.rg.ref, self.N, self.H,
                                      self.gd.data_ptr() if self.nd else None, self.dense_off, self.nd, self.st),
                "adam_flat")
        self.ops.counter_add(self.step_d, 1)

    # ---- checks
    def check_stamps(self, t, open_rows=None, lag=True):
        ls = self.last.cpu().numpy().astype(np.int64)
        mv = ls & STEP_MASK
        pa = (ls >> 24) & 63
        assert np.all(mv + pa <= t), "a row is stamped with a future step"
        if lag:  # include/hvae.h: no replay is longer than the sweep period
            assert int((t - mv).max()) <= self.period, (t, int((t - mv).max()), self.period)
        pend = (ls & PEND_BIT) != 0
        want = np.zeros(self.N, dtype=bool)
        if open_rows is not None:
            want[open_rows] = True
        assert np.array_equal(pend, want), "bit 30 outside the open deferred record's rows"

    def check_against_dense(self, pb, where):
        """Clones of the lazy state, resolved and caught up over all rows, are bitwise the dense arm."""
        p, m, v, last = self.p.clone(), self.m.clone(), self.v.clone(), self.last.clone()
        if self.pend_open:
            self.pending(pb, p, m, v, last)
        self.catchup_all(pb, p, m, v, last)
        for name, a, b in (("p", p, self.pd), ("m", m, self.md), ("v", v, self.vd)):
            assert _same(a, b), f"{where}: lazy {name} is not bitwise the dense arm's " \
                                f"(max |d| {float((a - b).abs().max()):.3e})"
        assert int(self.step.item()) == int(self.step_d.item())
        assert torch.equal(last, self.step.to(torch.int32).expand_as(last))

    def run(self, pb, catch="csr", use_clip=False, plan=None, lag=True, idem_at=()):
        """pb's steps on both GPU arms from the loaded state. catch: the per-step catch-up of the step's own rows
        (None, "rows", "csr"); plan[s], where given, overrides it with {"catch": .., "users": [[items]..] or a Csr,
        "clip_only": True (the counter and tab[t] advance, nothing else runs), "after_catch": f(self)}.
        idem_at: step indices at which a second hvae_adam_lazy_pending must change nothing."""
        T = pb.T
        mids = {T // 3, (2 * T) // 3} if T >= 6 else set()
        for s in range(T):
            t = pb.t0 + s + 1
            ps = (plan or {}).get(s, {})
            kind = ps.get("catch", catch)
            if ps.get("clip_only"):
                assert s in pb.no_update and self.nd == 0 and not self.defer
                self.set_rows(pb, s)
                self.clip_step(pb)
                self.dense_step(pb)
                if s + 1 in mids:
                    self.check_against_dense(pb, f"after step {s + 1}")
                continue
            if not self.defer:
                self.set_rows(pb, s)
            if kind is not None:
                x = None
                if kind == "csr":
                    users = ps.get("users")
                    x = users if isinstance(users, self.ops.Csr) else self.csr(
                        users if users is not None else A.users_from_rows(pb.sched[s], seed=pb.seed + s))
                ls0 = self.last.cpu().numpy().astype(np.int64) if self.defer else None
                self.catchup_batch(pb, kind, x)
                if self.defer and t > 1:
                    # what the catch-up did to the open record (step t - 1): pending rows it took, pending rows it
                    # left to hvae_adam_lazy_pending, and rows of that step's sweep range it moved p-only to t - 1
                    ls1 = self.last.cpu().numpy().astype(np.int64)
                    was = (ls0 & PEND_BIT) != 0
                    self.seen["claimed"] += int((was & ((ls1 & PEND_BIT) == 0)).sum())
                    self.seen["left"] += int((ls1 & PEND_BIT != 0).sum())
                    chunk = -(-self.N // self.period)
                    r0 = ((t - 2) % self.period) * chunk
                    seg = ls1[r0:min(self.N, r0 + chunk)]
                    pa = (seg >> 24) & 63
                    self.seen["p_only_in_sweep"] += int(((pa > 0) & ((seg & STEP_MASK) + pa == t - 1)).sum())
                if "after_catch" in ps:
                    ps["after_catch"](self)
            if self.defer:
                if s in idem_at:
                    self.pending(pb, self.p, self.m, self.v, self.last)
                    before = [x.clone() for x in (self.p, self.m, self.v, self.last)]
                self.pending(pb, self.p, self.m, self.v, self.last)
                if s in idem_at:
                    assert all(_same(a, b) for a, b in zip(before, (self.p, self.m, self.v, self.last))), \
                        "a second hvae_adam_lazy_pending changed something"
                self.pend_open = False
                self.check_stamps(t - 1, lag=lag)  # the record is resolved: no bit 30, the recorded step's sweep done
                self.set_rows(pb, s)  # only now: the recorded rows had to stay until hvae_adam_lazy_pending
            self.update(pb, use_clip)
            self.dense_step(pb)
            self.check_stamps(t, open_rows=pb.sched[s].astype(np.int64) if self.defer else None,
                              lag=lag and not self.defer)
            if s + 1 in mids:
                self.check_against_dense(pb, f"after step {s + 1}")
        if self.pend_open:
            self.pending(pb, self.p, self.m, self.v, self.last)
            self.pend_open = False
        self.catchup_all(pb, self.p, self.m, self.v, self.last)
        t_end = pb.t0 + T
        assert int(self.step.item()) == t_end
        assert torch.equal(self.last, torch.full_like(self.last, t_end)), "final last_step != step_dev (bits 24-30?)"
        for name, a, b in (("p", self.p, self.pd), ("m", self.m, self.md), ("v", self.v, self.vd)):
            assert _same(a, b), f"end: lazy {name} is not bitwise the dense arm's " \
                                f"(max |d| {float((a - b).abs().max()):.3e})"


# The GPU arms' bars are 4 x torch.optim.Adam's own float32 deviation from the float64 anchor (A.bars), computed per
# case, never from the kernels. The margin is for adam_elem's unfused products and 1-ulp v_sqrt_f32 / v_rcp_f32
# (csrc/hvae_adam.h) against torch's fused, correctly rounded ones.
# Measured on MI355X over the 62 cases of this file (lazy and dense arm alike: they are bitwise equal), GPU deviation
# against torch's own: p 8.0e-6 .. 2.3e-3 lr, at most 1.4 x torch's (rewind, wd = 0: 7.72e-5 against 5.58e-5 lr;
# equal to torch's in most cases, where p's own ulp dominates); m 4.9e-8 .. 1.5e-7, at most 2.2 x (N = 96, 40 steps:
# 1.46e-7 against 6.61e-8); v 1.4e-7 .. 1.5e-6, at most 1.03 x (N = 65,537, 70 steps: 6.91e-7 against 6.70e-7).
# The bars catch a row that is one step short: tests/test_adam_reference_cpu.py drops one g = 0 step of one row from
# the anchor, on these schedules with Problem's own gradients, and p moves by >= 14 x its bar, v by >= 25 x.


def _check_anchor(h, pb, label):
    f64 = A.adam_f64(pb)
    t32 = A.adam_torch32(pb)
    dev32 = A.deviation(t32, f64, pb.lr)
    bar = tuple(A.BAR_FACTOR * x for x in dev32)
    for arm, bufs in (("lazy", (h.p, h.m, h.v)), ("dense", (h.pd, h.md, h.vd))):
        dev = A.deviation(tuple(h.flat(b) for b in bufs), f64, pb.lr)
        print(f"{label} {arm}: p {dev[0]:.2e} lr, m {dev[1]:.2e}, v {dev[2]:.2e} | torch32 p {dev32[0]:.2e} lr, "
              f"m {dev32[1]:.2e}, v {dev32[2]:.2e}")
        for fig, d, b in zip("pmv", dev, bar):
            assert d <= b, f"{label}: {arm} arm's {fig} deviates {d:.3e} from the float64 anchor, bar {b:.3e}"


def _run_case(dev, pb, label, catch="csr", use_clip=False, plan=None, lag=True, defer=False, max_rows=None,
              dense_mis=0, tab_len=None, idem_at=()):
    h = Harness(dev, pb.N, pb.H, n_dense=pb.n_dense, dense_mis=dense_mis,
                tab_len=tab_len or pb.t0 + pb.T + 8, defer=defer, max_rows=max_rows)
    h.load(pb)
    h.run(pb, catch=catch, use_clip=use_clip, plan=plan, lag=lag, idem_at=idem_at)
    _check_anchor(h, pb, label)
    return h


# ------------------------------------------------------- period boundary and range arithmetic --
@pytest.mark.parametrize("sched", ["gaps", "extremes"])
@pytest.mark.parametrize("N", [1, 5, 13, 65535, 65536, 65537])
def test_period_boundary_and_ranges(hip_device, N, sched):
    """N below the period (empty sweep ranges, r0 >= N), N not a multiple of it (a short last range), either side of
    the 8 -> 32 switch at 65,536; 70 steps from N = 65,535 on (the 32-range sweep wraps twice, and 65,535 meets the
    revisit gaps of 31 .. 33 at period 8 too), 20 at the small N. gaps: rows that only the sweep moves, a row with a
    gradient every step, exact revisit gaps;
    extremes: a step with n_unique = 0 and a step with all N rows."""
    T = 70 if N >= 65535 else 20
    gen = A.gap_schedule if sched == "gaps" else A.extremes_schedule
    pb = A.Problem(N, 4, gen(N, T, seed=N % 97), seed=N % 89)
    i = [1, 5, 13, 65535, 65536, 65537].index(N) + (sched == "gaps")
    h = _run_case(hip_device, pb, f"N={N} {sched}", catch=("csr", "rows", None)[i % 3], use_clip=bool(i % 2))
    assert h.period == (32 if N >= 65536 else 8)


# ----------------------------------------------------------------------------- RowMap shapes --
@pytest.mark.parametrize("H", [4, 12, 128, 600, 1024, 1028, 2048])
def test_rowmap_shapes(hip_device, H):
    """H = 12: h4s = 3, 85 rows per block, one idle thread; 600: one row per block, idle threads; 1028 / 2048: the
    column loop, once with a ragged last pass."""
    pb = A.Problem(300, H, A.gap_schedule(300, 20, seed=H), seed=H)
    _run_case(hip_device, pb, f"H={H}", catch="csr" if H % 8 else "rows", use_clip=H in (12, 600, 1028))


# ------------------------------------------------------------- weight decay, coef, lr / beta2 --
@pytest.mark.parametrize("lr,b2", [(1e-3, 0.999), (3e-3, 0.99)])
@pytest.mark.parametrize("coef", [None, 0.37])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_weight_decay_coef_and_rates(hip_device, wd, coef, lr, b2):
    """wd = 0: the CSR catch-up's p-only replays and adam_elem0 / adam_mv0; wd != 0: the full store and the
    adam_elem(g = 0) replay with g + wd p. Against the float64 anchor, not only against the dense arm (which runs the
    same adam_elem)."""
    pb = A.Problem(96, 16, A.gap_schedule(96, 40, seed=5), lr=lr, betas=(0.9, b2), wd=wd, coef=coef, seed=11)
    _run_case(hip_device, pb, f"wd={wd} coef={coef} lr={lr}", catch="csr", use_clip=coef is not None)


# ------------------------------------------------------------------------ CSR catch-up claims --
def _claim_batch(h, kind, N):
    rng = np.random.default_rng(3)
    if kind == "one_user":  # nb = 1: 64 slices of one user's entries
        return h.csr([sorted(rng.choice(N, 200, replace=False).tolist())])
    if kind == "long_user":  # nb = 1024: one slice per user, one user of 300 items (a second claim group of 256)
        users = [sorted(rng.choice(N, int(rng.integers(1, 4)), replace=False).tolist()) for _ in range(1024)]
        users[500] = sorted(rng.choice(N, 300, replace=False).tolist())
        return h.csr(users)
    if kind == "shared_item":  # one item listed by 50 users: claimed once
        return h.csr([sorted({7} | set(rng.choice(N, 2, replace=False).tolist())) for _ in range(50)])
    # rows / rows_offset: the batch is matrix rows rows[2:] = 5, 17, 3, 38, 21, 5 of a larger CSR (row 5 twice: a
    # user listed twice in one batch, every one of its items a duplicate claim)
    users = [sorted(rng.choice(N, 5, replace=False).tolist()) for _ in range(40)]
    return h.csr(users, rows=[39, 0, 5, 17, 3, 38, 21, 5], rows_offset=2)


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("kind", ["one_user", "long_user", "shared_item", "rows_indirection"])
def test_csr_catchup_claims(hip_device, kind, wd):
    """The same hand-built batch caught up before every step's update (its rows need not have a gradient: p may move
    ahead without an update in the same step). A row listed several times is claimed, and replayed, once."""
    N = 400 if kind == "long_user" else 300
    pb = A.Problem(N, 8, A.random_schedule(N, 14, seed=9), wd=wd, seed=21)
    h = Harness(hip_device, N, 8, tab_len=64)
    x = _claim_batch(h, kind, N)
    plan = {s: {"catch": "csr", "users": x} for s in range(pb.T)}
    if kind == "rows_indirection":
        # the indirection is used: after step 1 (its gradient rows and sweep range 0 = rows 0 .. 37 are current) the
        # catch-up moves the items of matrix rows 5, 17, 3, 38, 21, 5 (five distinct users) and no others
        assert x.listed.size <= 25

        def only_listed(hh):
            ls = hh.last.cpu().numpy().astype(np.int64)
            cur = np.nonzero((ls & STEP_MASK) + ((ls >> 24) & 63) == 1)[0]
            want = sorted(set(x.listed.tolist()) | set(pb.sched[0].tolist()) | set(range(38)))
            assert cur.tolist() == want
        plan[1]["after_catch"] = only_listed
    h.load(pb)
    h.run(pb, plan=plan, use_clip=kind in ("one_user", "shared_item"))
    _check_anchor(h, pb, f"{kind} wd={wd}")


# ------------------------------------------------- p ahead without an update in the same step --
@pytest.mark.parametrize("found_by", ["sweep", "row_update"])
def test_p_ahead_without_update(hip_device, found_by):
    """include/hvae.h allows the CSR catch-up on rows that get no gradient in that step: p moves ahead alone (wd = 0)
    and m, v stay behind, twice over, until the sweep reaches the row (it must move m, v alone through the steps p
    already has) or a later row update finds it with p ahead of m, v."""
    N, H = 300, 8  # period 8, 38 rows per sweep range: row 5 is swept at t = 1, 9, 17; row 299 at t = 8, 16
    R = 5 if found_by == "sweep" else 299
    T = 18
    sched = A.random_schedule(N, T, seed=4, frac=0.1)
    sched = [r[r != R] for r in sched]
    put = lambda s: np.array(sorted(set(sched[s].tolist()) | {R}), dtype=np.int32)  # noqa: E731
    sched[1] = put(1)  # t = 2: R's moments become non-zero
    state = {}

    def stamp(key):
        return lambda h: state.__setitem__(key, int(h.last[R].item()))
    plan = {s: {"catch": None} for s in range(T)}
    plan[3] = {"catch": "csr", "users": [[R, 100, 101]], "after_catch": stamp("a")}   # t = 4: p -> 3
    if found_by == "sweep":
        plan[6] = {"catch": "csr", "users": [[R], [R, 102]], "after_catch": stamp("b")}  # t = 7: p -> 6; swept at 9
    else:
        plan[5] = {"catch": "csr", "users": [[R], [R, 102]], "after_catch": stamp("b")}  # t = 6: p -> 5
        sched[6] = put(6)  # t = 7: the row update finds m, v at 2, p at 5
    pb = A.Problem(N, H, sched, seed=31)
    _run_case(hip_device, pb, f"p ahead, found by {found_by}", plan=plan, use_clip=found_by == "sweep")
    assert state["a"] == (2 | (1 << 24)), hex(state["a"])
    assert state["b"] == (2 | ((4 if found_by == "sweep" else 3) << 24)), hex(state["b"])


# -------------------------------------------------------------------------- p-ahead saturation --
@pytest.mark.parametrize("K", [62, 63, 64, 100])
def test_p_ahead_saturation(hip_device, K):
    """K steps in which only hvae_clip_grad_norm_step_adam runs (tab[t] written, no sweep), then the CSR catch-up: up
    to 63 steps behind it stamps p alone (6 bits), from 64 it must fall back to storing p, m and v (kPAheadMax)."""
    N, H, t0 = 300, 8, 5
    sched = [np.zeros(0, np.int32)] * K + A.random_schedule(N, 3, seed=K, frac=0.2)
    pb = A.Problem(N, H, sched, t0=t0, moments=True, seed=K, no_update=set(range(K)))
    listed = list(range(0, 120))

    def after(h):
        ls = h.last.cpu().numpy().astype(np.int64)
        want = (t0 | (K << 24)) if K <= 63 else t0 + K
        assert np.all(ls[:120] == want) and np.all(ls[120:] == t0), (hex(int(ls[0])), hex(want))
    plan = {s: {"clip_only": True} for s in range(K)}
    plan[K] = {"catch": "csr", "users": [listed[i::7] for i in range(7)], "after_catch": after}
    _run_case(hip_device, pb, f"saturation K={K}", plan=plan, lag=False, catch=None)


# ---------------------------------------------------------------------------- high step counts --
@pytest.mark.parametrize("mode", ["csr", "csr_clip", "defer"])
def test_high_step_counts(hip_device, mode):
    """Steps 2^24 - 47 .. 2^24 - 8 with a full-length (2^24-entry) step table: the stamps carry all 24 low bits
    together with the p-ahead field and the pending bit."""
    t0 = (1 << 24) - 48
    pb = A.Problem(64, 8, A.gap_schedule(64, 40, seed=2), t0=t0, moments=True, seed=41)
    _run_case(hip_device, pb, f"high steps {mode}", catch="csr", use_clip=mode != "csr", defer=mode == "defer",
              tab_len=1 << 24)


def test_step_table_length_is_checked(hip_device):
    """hvae_adam_lazy refuses a step table longer than last_step's 24 bits can index, or shorter than 2 entries, with
    an error code (a host-side check, nothing is launched)."""
    pb = A.Problem(8, 4, A.random_schedule(8, 1, seed=1))
    h = Harness(hip_device, 8, 4, tab_len=16)
    h.load(pb)
    h.set_rows(pb, 0)
    before = [x.clone() for x in (h.p, h.m, h.v, h.last)]
    for bad in ((1 << 24) + 1, 1, 0):
        rc = h.L.hvae_adam_lazy(C.byref(h.cfg(pb, h.step)), h.tab.data_ptr(), bad, h.p.data_ptr(), h.m.data_ptr(),
                                h.v.data_ptr(), h.last.data_ptr(), h.rg.ref, 4, None, h.dense_off, 0, h.st)
        assert rc != h._lib.HVAE_OK and "step table" in h._lib.last_error(), (bad, rc, h._lib.last_error())
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(before, (h.p, h.m, h.v, h.last)))


# ------------------------------------------------------------------------------- dense segment --
@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("n_dense", [0, 1, 7, 4096 + 3])
def test_dense_segment(hip_device, n_dense, mis):
    """The small dense parameters behind W1t in the same launch: float4 body and scalar tail where the segment is
    16-byte aligned (dense_off a multiple of 4 floats), the scalar path where it is not (dense_off = 1 mod 4)."""
    pb = A.Problem(96, 16, A.gap_schedule(96, 12, seed=8), n_dense=n_dense, wd=0.01 if n_dense == 7 else 0.0,
                   coef=0.37 if mis else None, seed=51)
    _run_case(hip_device, pb, f"n_dense={n_dense} off%4={mis}", catch="csr", use_clip=bool(mis), dense_mis=mis)


# ------------------------------------------------------------------------------- deferred trio --
@pytest.mark.parametrize("max_rows", ["N", 1])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("N", [300, 65537])
def test_deferred_trio(hip_device, N, wd, max_rows):
    """40 steps, every one deferring: hvae_adam_lazy_defer records step t; the next step's
    hvae_adam_lazy_catchup_csr_pending lists some of the pending rows (row 2 has a gradient every step and is listed
    by every user) and rows of step t's sweep range without a pending update, which it moves p-only to t (wd = 0), so
    that hvae_adam_lazy_pending must replay their m, v alone; then hvae_adam_lazy_pending with a grid for N rows, or
    for one (a single strided block); a second run of it changes nothing."""
    H = 4 if N > 300 else 8
    pb = A.Problem(N, H, A.gap_schedule(N, 40, seed=6), wd=wd, coef=0.37 if wd else None, seed=61)
    h = _run_case(hip_device, pb, f"defer N={N} wd={wd} max_rows={max_rows}", catch="csr", use_clip=max_rows == 1,
                  defer=True, max_rows=N if max_rows == "N" else 1, idem_at=(1, 17, 33))
    print("reached:", h.seen)
    # the next batch overlapped the pending rows partly, and (wd = 0) moved rows of the recorded step's sweep range
    # p-only before hvae_adam_lazy_pending swept them
    assert h.seen["claimed"] >= 39 and h.seen["left"] >= 39
    assert (h.seen["p_only_in_sweep"] > 0) == (wd == 0.0)


# -------------------------------------------------------------------------------------- rewind --
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_rewind_leaves_no_live_record(hip_device, wd):
    """A loaded optimizer state moves step_dev backwards (HipAdam.load_state_dict: step_dev and last_step set to the
    loaded step, fresh p, m, v) while the header of the last deferred step, long resolved, still sits in device
    memory. hvae_adam_lazy_pending before anything is recorded again must change nothing: the record is live only
    while step_dev is its step. Without that check the old step's sweep range is replayed through the old step and
    stamped with it, 13 steps in the future. Then 15 more deferring steps must be bitwise the dense arm's."""
    N, H = 300, 8
    h = Harness(hip_device, N, H, tab_len=64, defer=True)
    pb1 = A.Problem(N, H, A.gap_schedule(N, 20, seed=7), wd=wd, seed=71)
    h.load(pb1)
    h.run(pb1, catch="csr", use_clip=True)  # steps 1 .. 20, every record resolved; hdr.t = 20 stays behind
    assert int(h.pend_hdr[0].item()) == 20
    pb2 = A.Problem(N, H, A.gap_schedule(N, 15, seed=8), wd=wd, t0=7, moments=True, seed=72)
    h.load(pb2)  # step_dev = 7, last_step all 7 (mark_all_current), fresh p, m, v; rg.rows stays allocated
    before = [x.clone() for x in (h.p, h.m, h.v, h.last)]
    h.pending(pb2, h.p, h.m, h.v, h.last)
    torch.cuda.synchronize()
    moved = int((h.last != before[3]).sum().item())
    assert all(_same(a, b) for a, b in zip(before, (h.p, h.m, h.v, h.last))), \
        f"hvae_adam_lazy_pending replayed a stale record: {moved} rows restamped, " \
        f"max |dp| {float((h.p - before[0]).abs().max()) / pb2.lr:.3e} lr, last_step max {int(h.last.max().item())}"
    h.run(pb2, catch="csr", use_clip=True)
    _check_anchor(h, pb2, f"rewind wd={wd}")
