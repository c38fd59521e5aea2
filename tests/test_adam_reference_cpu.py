"""The float64 Adam anchor of the lazy-Adam kernel tests (tests/adam_lazy_ref.py), checked without a GPU.

tests/test_gpu_adam_lazy.py bars the kernels at 4 x the deviation of torch.optim.Adam (CPU, float32) from the float64
anchor. Those bars mean something only if the defect they exist to catch -- a row replayed one step too few -- moves
the anchor by much more: here one g = 0 step of one row is dropped from the float64 arm, and p and v must move by at
least 10 x their bars for every (row, step) of a fixed sample.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import adam_lazy_ref as A  # noqa: E402

MIN_FACTOR = 10.0
GENERATORS = {"random": A.random_schedule, "gaps": A.gap_schedule, "extremes": A.extremes_schedule}
# (schedule, N, H, T, wd): the three generators at the size the bars were first measured at, with and without weight
# decay, and the 20-step cases at the GPU file's N = 300
CASES = [(g, 96, 16, 80, wd) for g in GENERATORS for wd in (0.0, 0.01)] + [("gaps", 300, 8, 20, 0.0),
                                                                           ("extremes", 300, 8, 20, 0.01)]


def _problem(gen, N, H, T, wd):
    # built as tests/test_gpu_adam_lazy.py builds its cases: the generators' schedules, Problem's own gradients
    return A.Problem(N, H, GENERATORS[gen](N, T, seed=1), wd=wd, seed=1)


def _sample(pb):
    """(row, step index) pairs, fixed: from a quarter of the run on, at 12 evenly spaced steps, the first two rows --
    counted from a row that moves with the step -- that have no gradient at that step but had one before it."""
    out = []
    for s in sorted({pb.T // 4 + (i * (pb.T - pb.T // 4)) // 12 for i in range(12)}):
        before = np.zeros(pb.N, dtype=np.int64)
        for q in range(s):
            before[pb.sched[q]] += 1
        now = set(pb.sched[s].tolist())
        order = [(7 * s + i) % pb.N for i in range(pb.N)]
        out += [(r, s) for r in order if before[r] >= 1 and r not in now][:2]
    return out


@pytest.mark.parametrize("gen,N,H,T,wd", CASES)
def test_anchor_agrees_with_torch_adam(gen, N, H, T, wd):
    """torch.optim.Adam in float32 stays within float32 rounding of the float64 restatement (the same operation,
    not a different one): p within 1e-3 lr, m and v within 1e-5 of their largest value."""
    pb = _problem(gen, N, H, T, wd)
    dev32 = A.deviation(A.adam_torch32(pb), A.adam_f64(pb), pb.lr)
    print("dev32 (p / lr, m rel, v rel):", dev32)
    assert dev32[0] < 1e-3 and dev32[1] < 1e-5 and dev32[2] < 1e-5
    assert min(dev32) > 0.0


@pytest.mark.parametrize("gen,N,H,T,wd", CASES)
def test_one_dropped_step_is_far_above_the_bars(gen, N, H, T, wd):
    """One g = 0 step of one row dropped from the float64 arm moves p and v by at least 10 x the bars the GPU arms
    are held to, for every (row, step) of the sample, on the schedules and gradients the GPU cases run."""
    pb = _problem(gen, N, H, T, wd)
    f64 = A.adam_f64(pb)
    bar = A.bars(pb, f64, A.adam_torch32(pb))
    sample = _sample(pb)
    assert len(sample) >= 16
    worst = [np.inf] * 3
    for row, s in sample:
        dev = A.deviation(A.adam_f64(pb, skip=(row, s)), f64, pb.lr)
        worst = [min(w, d / b) for w, d, b in zip(worst, dev, bar)]
        assert dev[0] >= MIN_FACTOR * bar[0], (row, s, dev[0], bar[0])
        assert dev[2] >= MIN_FACTOR * bar[2], (row, s, dev[2], bar[2])
    print(f"{gen} N={N} T={T} wd={wd}: bars p {bar[0]:.2e} lr, m {bar[1]:.2e}, v {bar[2]:.2e}; smallest move in bars: "
          f"p {worst[0]:.1f}, m {worst[1]:.1f}, v {worst[2]:.1f}")


def test_schedules_reach_what_they_are_named_for():
    """The generators' promises: rows that never get a gradient, one with a gradient every step, exact revisit gaps,
    an empty step and an all-rows step."""
    Tn, Nn = 70, 300
    sched = A.gap_schedule(Nn, Tn, seed=3)
    hit = np.zeros((Tn, Nn), dtype=bool)
    for s, rows in enumerate(sched):
        assert np.all(np.diff(rows) > 0) and rows.dtype == np.int32
        hit[s, rows] = True
    assert not hit[:, A.never_rows(Nn)].any() and A.never_rows(Nn).size > 3
    assert hit[:, 2].all()
    for i, g in enumerate(A.GAPS):
        steps = np.nonzero(hit[:, 3 + i])[0]
        assert steps[0] == 2 and np.all(np.diff(steps) == g) and steps.size >= 3, (g, steps)
    for n_small in (1, 5, 13):
        s_small = A.gap_schedule(n_small, 20, seed=3)
        assert all(r.size == 0 or (r.min() >= 0 and r.max() < n_small) for r in s_small)
        assert sum(r.size for r in s_small) > 0
    ex = A.extremes_schedule(Nn, 20, seed=3)
    assert ex[3].size == 0 and np.array_equal(ex[10], np.arange(Nn))
    users = A.users_from_rows(sched[5], seed=1)
    assert sorted({j for u in users for j in u}) == sched[5].tolist()
    assert all(int(sched[5][0]) in u for u in users) and len(users) > 1
