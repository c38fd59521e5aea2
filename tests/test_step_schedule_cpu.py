"""The train step's schedule (hvae.executor.step_schedule): which batch gets which arrangement of the row-gradient
plan, the lazy-Adam catch-up, the side stream and the deferred update. A pure function of plain values: no library,
no device."""
import itertools

import pytest

from hvae._lib import PLAN_SMALL_CAP
from hvae.executor import StepSchedule, step_schedule

BASE = dict(B=64, train=True, dp=False, lazy_adam=True, adam_defer=False, enc_lazy_read=True, rows_ok=True,
            one_hidden_512=True, side_min_batch=512, cap=1000)


def sched(**kw) -> StepSchedule:
    return step_schedule(**{**BASE, **kw})


def S(rows, fused_enc, enc_lazy, plan, catchup, wgrad_side, defer) -> StepSchedule:
    return StepSchedule(rows=rows, fused_enc=fused_enc, enc_lazy=enc_lazy, plan=plan, catchup=catchup,
                        wgrad_side=wgrad_side, defer=defer)


def test_plan_small_cap_is_the_librarys():
    assert PLAN_SMALL_CAP == 4096


@pytest.mark.parametrize("B", [2, 64, 512, 4096])
@pytest.mark.parametrize("adam_defer", [False, True])
def test_eval_step_has_no_plan_catchup_side_or_defer(B, adam_defer):
    s = sched(B=B, train=False, adam_defer=adam_defer)
    assert (s.plan, s.catchup, s.wgrad_side, s.defer, s.enc_lazy) == (None, None, False, False, False)
    assert s.rows and s.fused_enc  # the forward's own arrangement does not depend on training


ROWS = [
    # small batch, row-parallel MLP with the fused encoder reading W1t through lazy Adam
    (dict(), S(True, True, True, "in_rows", None, False, False)),
    (dict(enc_lazy_read=False), S(True, True, False, "in_rows", "csr", False, False)),
    (dict(cap=5000), S(True, True, True, "inline", None, False, False)),
    (dict(rows_ok=False), S(False, False, False, "inline", "rowgrad", False, False)),
    (dict(one_hidden_512=False), S(True, False, False, "in_rows", "csr", False, False)),
    # the side-stream threshold
    (dict(B=512, adam_defer=True), S(True, True, True, "stream", None, True, False)),
    (dict(B=511, adam_defer=True), S(True, True, True, "in_rows", None, False, False)),
    # large batches: the plan on its stream, the CSR catch-up, the deferred update
    (dict(B=4096, rows_ok=False, adam_defer=False), S(False, False, False, "stream", "csr", True, False)),
    (dict(B=4096, rows_ok=False, adam_defer=True), S(False, False, False, "stream", "csr_pending", True, True)),
    # data parallel
    (dict(dp=True, adam_defer=True), S(True, True, False, "dp", "csr_pending", False, True)),
    (dict(dp=True, adam_defer=False), S(True, True, False, "dp", "csr", False, False)),
    # dense Adam: nothing to catch up, nothing to defer
    (dict(lazy_adam=False, adam_defer=True, B=4096), S(True, True, False, "stream", None, True, False)),
    # the threshold out of reach: a large batch with its plan in line
    (dict(B=4096, side_min_batch=1000000, rows_ok=False, cap=60000),
     S(False, False, False, "inline", "rowgrad", False, False)),
]


@pytest.mark.parametrize("kw,want", ROWS, ids=[",".join(f"{k}={v}" for k, v in kw.items()) or "base"
                                               for kw, _ in ROWS])
def test_schedule_rows(kw, want):
    assert sched(**kw) == want


def test_one_block_plan_bounds():
    """"in_rows" needs the batch and its row gradient to fit the one-block plan: both bounds are inclusive."""
    assert sched(B=64, cap=PLAN_SMALL_CAP).plan == "in_rows"
    assert sched(B=64, cap=PLAN_SMALL_CAP + 1).plan == "inline"
    big = dict(side_min_batch=1 << 20, cap=100)
    assert sched(B=PLAN_SMALL_CAP, **big).plan == "in_rows"
    assert sched(B=PLAN_SMALL_CAP + 1, **big).plan == "inline"


BOOLS = ["train", "dp", "lazy_adam", "adam_defer", "enc_lazy_read", "rows_ok", "one_hidden_512"]


def test_invariants_over_every_input():
    for B in (2, 64, 511, 512, 4096):
        for cap in (1000, 5000):
            for bits in itertools.product([False, True], repeat=len(BOOLS)):
                kw = dict(zip(BOOLS, bits))
                s = sched(B=B, cap=cap, **kw)
                assert not s.defer or s.catchup == "csr_pending", (B, kw)
                assert not s.enc_lazy or (s.catchup is None and not s.defer), (B, kw)
                assert s.rows == kw["rows_ok"] and s.fused_enc == (kw["rows_ok"] and kw["one_hidden_512"])
                assert (s.catchup == "csr_pending") == s.defer, (B, kw)
                if not kw["train"]:
                    assert (s.plan, s.catchup, s.wgrad_side, s.defer, s.enc_lazy) == (None, None, False, False, False)
                else:
                    assert s.plan in ("dp", "stream", "in_rows", "inline")
                    assert s.wgrad_side == (B >= 512)
