"""Host-side anchors and schedules of the lazy-Adam kernel tests (not collected: no test_ prefix).

tests/test_gpu_adam_lazy.py drives hvae_adam_lazy and its catch-ups from a hand-written schedule (which W1t rows
get a gradient at which step) and compares three arms on identical inputs; this module holds what needs no GPU:

  adam_f64        a float64 restatement of torch's single-tensor Adam (torch/optim/adam.py _single_tensor_adam),
                  applied to every element every step with g = 0 outside the schedule, clip multiplier and
                  weight decay included -- the anchor;
  adam_torch32    torch.optim.Adam itself on the CPU in float32 over the same dense gradients -- the optimiser
                  the reference trainer calls (src/ml/train.py:63); its deviation from the anchor (`deviation`)
                  sets the bars of the GPU arms, so no bar is hard-coded or taken from the kernels;
  Problem         one case's sizes, hyper-parameters, start state and per-step gradients, reproducible from
                  a seed (the gradients are generated per step, not stored);
  *_schedule      the schedule generators.

tests/test_adam_reference_cpu.py checks here, without a GPU, that the bars stay meaningful: dropping a single
g = 0 step of a single row from the anchor moves it by many times the bar.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

GAPS = (1, 4, 5, 8, 9, 31, 32, 33)  # revisit gaps: across the 4-entry table prefetch rounds and both sweep periods


# ------------------------------------------------------------------ schedules --
def gap_schedule(N: int, T: int, seed: int, frac: float = 0.15) -> list[np.ndarray]:
    """Rows by role, as far as N has rows for them: row 1 never gets a gradient (nor does the last row, nor every
    17th from row 28 on), row 2 gets one every step, row 3 + i is revisited at gaps of exactly GAPS[i] (from step
    index 2 on), and every other row gets one with probability `frac` per step. Row 0 is an ordinary random row, so
    that N = 1 still has gradients."""
    rng = np.random.default_rng([seed, N, T])
    never = {r for r in (1, N - 1) if 0 < r < N} | set(range(28, N, 17))
    every = {2} if N > 2 else set()
    gap_rows = {3 + i: g for i, g in enumerate(GAPS) if 3 + i < N - 1}
    other = np.array([r for r in range(N) if r not in never and r not in every and r not in gap_rows], dtype=np.int64)
    sched = []
    for s in range(T):
        rows = set(every)
        rows |= {r for r, g in gap_rows.items() if s >= 2 and (s - 2) % g == 0}
        if other.size:
            rows |= set(other[rng.random(other.size) < (frac if N > 1 else 0.5)].tolist())
        sched.append(np.array(sorted(rows), dtype=np.int32))
    return sched


def never_rows(N: int) -> np.ndarray:
    return np.array(sorted({r for r in (1, N - 1) if 0 < r < N} | set(range(28, N, 17))), dtype=np.int64)


def extremes_schedule(N: int, T: int, seed: int, frac: float = 0.15) -> list[np.ndarray]:
    """Random rows with probability `frac`, but step index 3 has no gradient row at all (n_unique = 0) and step
    index T // 2 has all N."""
    rng = np.random.default_rng([seed, N, T, 1])
    sched = [np.nonzero(rng.random(N) < frac)[0].astype(np.int32) for _ in range(T)]
    sched[min(3, T - 1)] = np.zeros(0, dtype=np.int32)
    sched[T // 2] = np.arange(N, dtype=np.int32)
    return sched


def random_schedule(N: int, T: int, seed: int, frac: float = 0.15) -> list[np.ndarray]:
    rng = np.random.default_rng([seed, N, T, 2])
    return [np.nonzero(rng.random(N) < frac)[0].astype(np.int32) for _ in range(T)]


def users_from_rows(rows: np.ndarray, seed: int, per_user: int = 6, shared: int = 2) -> list[list[int]]:
    """A batch whose item set is exactly `rows`: users of `per_user` items each, and the first `shared` rows listed
    by every user as well (rows that several CSR entries claim at once)."""
    rows = [int(r) for r in rows]
    if not rows:
        return [[]]
    rng = np.random.default_rng([seed, len(rows)])
    perm = [rows[i] for i in rng.permutation(len(rows))]
    users = []
    for i in range(0, len(perm), per_user):
        u = set(perm[i:i + per_user]) | set(rows[:shared])
        users.append(sorted(u))
    return users


# --------------------------------------------------------------------- problem --
@dataclass
class Problem:
    N: int
    H: int
    sched: list  # per step: int32 array of the rows with a gradient
    lr: float = 1e-3
    betas: tuple = (0.9, 0.999)
    eps: float = 1e-8
    wd: float = 0.0
    coef: float | None = None  # the clip multiplier (coef_dev): None = NULL (1)
    n_dense: int = 0           # dense segment behind W1t (gradient every step)
    t0: int = 0                # completed steps at the start
    seed: int = 0
    no_update: set = field(default_factory=set)  # step indices that only advance the counter (g = 0 for all)
    moments: bool = False      # start from non-zero m, v (t0 > 0) instead of zeros
    _scale: np.ndarray | None = field(default=None, repr=False, compare=False)  # row_scale()'s cache

    @property
    def T(self) -> int:
        return len(self.sched)

    @property
    def n(self) -> int:
        return self.N * self.H + self.n_dense

    @property
    def coef32(self) -> np.float32:
        return np.float32(1.0 if self.coef is None else self.coef)

    def start(self):
        """(p, m, v) float32 flat [N * H + n_dense]: p weight-like (0.05 N(0, 1): a step of ~lr is then well above
        p's own ulp), m = v = 0 or, with `moments`, what a few steps of such gradients leave."""
        rng = np.random.default_rng([self.seed, 7])
        p = (0.05 * rng.standard_normal(self.n)).astype(np.float32)
        if self.moments:
            m = (0.01 * rng.standard_normal(self.n)).astype(np.float32)
            v = (1e-4 * rng.standard_normal(self.n) ** 2).astype(np.float32)
        else:
            m = np.zeros(self.n, np.float32)
            v = np.zeros(self.n, np.float32)
        return p, m, v

    def row_scale(self) -> np.ndarray:
        """The gradient scale of each row [N]: 0.05 sqrt(c_med / c_r), c_r the number of steps that give row r a
        gradient and c_med the median of the non-zero c_r. Every row's v then ends near the same size whether it is
        visited once or every step (v ~ c_r scale_r^2 (1 - b2)), which the anchor's v and m figures need: they are
        relative to the largest |v| and |m| of the whole state, so a row whose v sat far below the largest could be
        a step short without moving them (tests/test_adam_reference_cpu.py proves the sensitivity for exactly these
        gradients). The scales still span sqrt(T): 8 x at 70 steps."""
        if self._scale is None:
            c = np.zeros(self.N)
            for s, rows in enumerate(self.sched):
                if s not in self.no_update:
                    c[np.asarray(rows, dtype=np.int64)] += 1
            med = np.median(c[c > 0]) if np.any(c > 0) else 1.0
            self._scale = 0.05 * np.sqrt(med / np.maximum(c, 1.0))
        return self._scale

    def row_grads(self, s: int) -> np.ndarray:
        """Step index s's gradient rows [len(sched[s]), H] float32, before the clip multiplier: N(0, 1) times the
        row's scale (row_scale)."""
        rng = np.random.default_rng([self.seed, 11, s])
        rows = np.asarray(self.sched[s], dtype=np.int64)
        return (rng.standard_normal((len(rows), self.H)) * self.row_scale()[rows, None]).astype(np.float32)

    def dense_grads(self, s: int) -> np.ndarray:
        rng = np.random.default_rng([self.seed, 13, s])
        return (0.02 * rng.standard_normal(self.n_dense)).astype(np.float32)

    def flat_grad(self, s: int) -> np.ndarray:
        """The step's dense gradient over the flat state, float32, zero outside the schedule."""
        g = np.zeros(self.n, np.float32)
        if s in self.no_update:
            return g
        rows = np.asarray(self.sched[s], dtype=np.int64)
        if rows.size:
            g[:self.N * self.H].reshape(self.N, self.H)[rows] = self.row_grads(s)
        if self.n_dense:
            g[self.N * self.H:] = self.dense_grads(s)
        return g


# --------------------------------------------------------------------- anchors --
def adam_f64(pb: Problem, steps: int | None = None, skip: tuple | None = None, snapshots=()):
    """torch's single-tensor Adam in float64 over every element every step. skip = (row, step index): that row
    alone misses that step (p, m, v stay) -- a lazy replay one step short. Returns (p, m, v) float64 flat, or with
    `snapshots` (step counts) a dict {steps done: (p, m, v)} that includes the end."""
    p0, m0, v0 = pb.start()
    p, m, v = p0.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64)
    b1, b2 = pb.betas
    coef = float(pb.coef32)
    T = pb.T if steps is None else steps
    out = {}
    for s in range(T):
        t = pb.t0 + s + 1
        g = pb.flat_grad(s).astype(np.float64) * coef
        if skip is not None and skip[1] == s:
            r = slice(skip[0] * pb.H, (skip[0] + 1) * pb.H)
            keep = (p[r].copy(), m[r].copy(), v[r].copy())
        if pb.wd != 0.0:
            g = g + pb.wd * p
        m = m + (1.0 - b1) * (g - m)
        v = b2 * v + (1.0 - b2) * g * g
        bc1 = 1.0 - b1 ** t
        bc2 = 1.0 - b2 ** t
        denom = np.sqrt(v) / np.sqrt(bc2) + pb.eps
        p = p - (pb.lr / bc1) * (m / denom)
        if skip is not None and skip[1] == s:
            p[r], m[r], v[r] = keep
        if s + 1 in snapshots:
            out[s + 1] = (p.copy(), m.copy(), v.copy())
    if snapshots:
        out[T] = (p, m, v)
        return out
    return p, m, v


def adam_torch32(pb: Problem, snapshots=()):
    """torch.optim.Adam on the CPU in float32 over the same dense gradients (clip multiplier applied to the
    gradient in float32, as clip_grad_norm_ does). Same return shape as adam_f64."""
    p0, m0, v0 = pb.start()
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([p], lr=pb.lr, betas=pb.betas, eps=pb.eps, weight_decay=pb.wd)
    if pb.t0 > 0 or pb.moments:
        opt.state[p] = {"step": torch.tensor(float(pb.t0)), "exp_avg": torch.from_numpy(m0.copy()),
                        "exp_avg_sq": torch.from_numpy(v0.copy())}
    out = {}

    def snap():
        st = opt.state[p]
        return (p.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy())

    for s in range(pb.T):
        p.grad = torch.from_numpy(pb.flat_grad(s) * pb.coef32)
        opt.step()
        if s + 1 in snapshots:
            out[s + 1] = snap()
    if snapshots:
        out[pb.T] = snap()
        return out
    return snap()


def deviation(got, ref, lr: float) -> tuple:
    """(p: max |d| in units of lr, m: max |d| / max |ref|, v: max |d| / max |ref|) of a (p, m, v) triple against
    the float64 anchor's."""
    d = [np.abs(np.asarray(g, dtype=np.float64) - r).max() if r.size else 0.0 for g, r in zip(got, ref)]
    scale = [lr] + [max(float(np.abs(r).max()) if r.size else 0.0, 1e-300) for r in ref[1:]]
    return tuple(float(x / s) for x, s in zip(d, scale))


BAR_FACTOR = 4.0  # the GPU arms' bar: this times torch's own float32 deviation from the anchor, per figure


def bars(pb: Problem, f64, t32) -> tuple:
    return tuple(BAR_FACTOR * x for x in deviation(t32, f64, pb.lr))
