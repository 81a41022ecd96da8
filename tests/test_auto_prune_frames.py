"""The frames of test_gpu_auto_prune.py have the window shares their cases rely on, by the numpy restatement of
the tiled form's window rule (auto_prune_frames.predict), on the CPU: the pruning frames at most a quarter of
kAutoPruneBudget, the i.i.d. noise frames exactly 1, the smooth frames of this size over the budget by half of
it or more."""
import numpy as np
import pytest

import auto_prune_frames as A

SIZES = [(256, 256, 8), (264, 248, 8), (264, 248, 4)]


def test_levels_leave_mixed_domains_between_them():
    import itertools

    for lv in A.LEVELS:
        others = [sum(c) for c in itertools.combinations_with_replacement(A.LEVELS, 4) if set(c) != {lv}]
        assert min(abs(s - 4 * lv) for s in others) >= 31


@pytest.mark.parametrize("W,H,dstep", SIZES)
@pytest.mark.parametrize("amp", [0, 2])
def test_mosaic_predicts_a_quarter_of_the_budget_or_less(W, H, dstep, amp):
    r = A.predict(A.mosaic(W, H, amp=amp), dstep)
    assert 0 < r["share"] <= A.BUDGET / 4, r["share"]
    assert r["evals"] + r["seed_evals"] < r["eligible"]


@pytest.mark.parametrize("W,H,dstep", SIZES)
def test_noise_predicts_every_window_open(W, H, dstep):
    r = A.predict(A.noise(W, H), dstep)
    assert r["pairs"] == r["full"] and r["share"] == 1.0 and r["evals"] == r["eligible"]


def test_smooth_frames_of_this_size_are_over_the_budget():
    from fractencode_amd.synth import value_noise

    shares = [A.predict(value_noise(256, 256, 77))["share"], A.predict(value_noise(264, 248, 77))["share"],
              A.predict(A.ramp(256, 256))["share"]]
    assert all(1.5 * A.BUDGET <= s < 1.0 for s in shares), shares


@pytest.mark.parametrize("W,H", [(256, 256), (264, 248)])
def test_shard_keeps_one_level_per_group(W, H):
    idx = A.mosaic_shard(W, H)
    for p in (A.mosaic(W, H), A.mosaic(W, H, amp=3, noise_seed=99)):
        r = A.predict(p, ranges=idx)
        assert [len(g[0]) for g in r["groups"]] == [256, 256, 256, 32]
        assert r["share"] <= A.BUDGET / 4
    assert A.predict(A.noise(W, H), ranges=idx)["share"] == 1.0


def test_budget_is_the_library_s():
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fractencode_amd", "csrc",
                            "fracenc_plan.hip")).read()
    m = re.search(r"kAutoPruneBudgetNum = (\d+), kAutoPruneBudgetDen = (\d+);", src)
    assert m and np.isclose(int(m.group(1)) / int(m.group(2)), A.BUDGET)
