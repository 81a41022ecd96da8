"""The rate rule's numpy restatement (quadtree_rate_ref.py) against the reference alone, on the CPU: at a
candidate t the closed-form size equals len(codec.pack_quadtree_stream(oracle.quadtree(t))) and the leaves equal
the oracle's, bit for bit — no tolerance anywhere.  Every candidate of m98x74_16_4; of the other cases at least
8 spread over the sorted list with both ends (every candidate of t342x278_16_4 would cost minutes of oracle
time).  The guards show that the cases are not vacuous for the engines' test (test_gpu_quadtree_rate.py)."""
import numpy as np
import pytest

import quadtree_frames as Q
import quadtree_rate_ref as R
from fractencode_amd import codec


def _ids(c):
    return c.name


def _oracle_at(oracle, case, t):
    src, tgt = case.planes()
    recs, sizes = oracle.quadtree(src, case.max_size, case.min_size, t, T=case.T, use_classifier=case.cls,
                                  thr=case.thr, tgt=tgt)
    return Q.as_items(recs, sizes)


def _check_at(oracle, case, tree, t):
    items = _oracle_at(oracle, case, float(t))
    stream = codec.pack_quadtree_stream(items, case.W, case.H, case.max_size, case.min_size, transforms=case.T,
                                        use_classifier=case.cls)
    size, leaves, _ = tree.size(float(t))
    assert len(stream) == size, (case.name, t)
    assert leaves == len(items), (case.name, t)
    np.testing.assert_array_equal(tree.leaves(float(t)), Q.leaves_from_records(items, case.W), err_msg=f"{case.name} {t}")


def test_every_candidate_of_the_full_case(oracle):
    tree = R.tree(oracle, R.FULL)
    cands = tree.candidates()
    assert cands[0] == 0.0 and len(cands) > 100
    for t in cands:
        _check_at(oracle, R.FULL, tree, t)
    # between two neighbouring candidates, below the first and above the last, nothing changes
    for t in (-1.0, 0.5 * (cands[3] + cands[4]), float("inf")):
        _check_at(oracle, R.FULL, tree, t)


@pytest.mark.parametrize("case", R.SPREAD, ids=_ids)
def test_a_spread_of_candidates(oracle, case):
    tree = R.tree(oracle, case)
    cands = tree.candidates()
    picked = R.spread(cands, 8)
    assert len(picked) == min(len(cands), 8) and picked[0] == cands[0] and picked[-1] == cands[-1]
    for t in picked:
        _check_at(oracle, case, tree, t)
    # other record widths: the closed form follows the layout, not the default widths
    items = _oracle_at(oracle, case, float(picked[len(picked) // 2]))
    for cb, bb in ((2, 2), (16, 16)):
        stream = codec.pack_quadtree_stream(items, case.W, case.H, case.max_size, case.min_size, transforms=case.T,
                                            use_classifier=case.cls, contrast_bits=cb, brightness_bits=bb)
        assert len(stream) == tree.size(float(picked[len(picked) // 2]), cb, bb)[0]


@pytest.mark.parametrize("case", [c for c in [R.FULL] + R.SPREAD if c in Q.MIXED], ids=_ids)
def test_mixed_cases_have_many_distinct_sizes(oracle, case):
    # (the MIXED cases checked above; the smallest frame at (16, 4), m70x58_16_4, has 49 candidates in all)
    tree = R.tree(oracle, case)
    sizes = tree.sizes()
    assert len(np.unique(sizes)) > 100, case.name
    assert len(np.unique(sizes)) == len(tree.candidates())  # every candidate a size of its own
    assert np.all(np.diff(sizes) < 0)  # monotone here; the fit's definition does not rely on it


@pytest.mark.parametrize("case", [c for c in Q.MIXED + Q.EMPTY + [Q.HIT_THR, Q.TWO_PLANES, Q.TILE_CARRY] if c.cls],
                         ids=_ids)
def test_classifier_cases_have_tied_keys(oracle, case):
    tree = R.tree(oracle, case)
    keys = np.concatenate(tree.e)
    assert len(np.unique(keys)) < len(keys), case.name  # e.g. several default records at 1e5


@pytest.mark.parametrize("case", Q.MIXED + [Q.HIT_THR, Q.TWO_PLANES, Q.TILE_CARRY], ids=_ids)
def test_fit_budgets_hit_five_different_candidates(oracle, case):
    tree = R.tree(oracle, case)
    budgets = R.fit_budgets(tree)
    fits = [tree.fit(b) for b, ok in budgets if ok]
    assert all(f is not None for f in fits)
    assert [tree.fit(b) for b, ok in budgets if not ok] == [None]
    assert len({f[0] for f in fits}) >= 5, case.name
    for (b, _), f in zip([x for x in budgets if x[1]], fits):
        assert f[1] <= b
    # the largest size and anything above it: the smallest candidate
    assert tree.fit(budgets[2][0])[0] == tree.fit(budgets[3][0])[0] == 0.0


def test_no_range_and_no_domain_cases(oracle):
    t = R.tree(oracle, Q.BY_NAME["z15x15"])
    assert list(t.candidates()) == [0.0] and t.size(0.0)[:2] == (64, 0) and t.fit(64) == (0.0, 64, 0)
    t = R.tree(oracle, Q.BY_NAME["d31x31_16_4"])
    assert t.ndoms[0] == 0 and np.all(t.recs[0]["dist"] == 1e5)
