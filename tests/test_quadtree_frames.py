"""The cases of quadtree_frames.py have the properties test_gpu_quadtree_shapes.py relies on, checked on the
CPU with the oracle alone: a GPU test on them cannot pass vacuously.  These are conditions on the inputs
(the seeds and split distances in quadtree_frames.py were picked so that the oracle satisfies them), not
tolerances."""
import numpy as np
import pytest

import quadtree_frames as Q


@pytest.fixture(scope="module")
def run(oracle):
    cache = {}

    def get(case):
        if case.name not in cache:
            cache[case.name] = Q.run_oracle(oracle, case)
        return cache[case.name]

    return get


def _levels(case):
    n, out = case.max_size, []
    while n >= case.min_size:
        out.append(n)
        n //= 2
    return out


def _coverage(recs, sizes, W, H):
    cov = np.zeros((H, W), np.int32)
    for r, s in zip(recs, sizes):
        cov[r["y"]:r["y"] + s, r["x"]:r["x"] + s] += 1
    return cov


def _searched_and_split(oracle, recs, sizes, case, level):
    """The ranges the level searched, in search order, and which of them split: rebuilt from the leaves (a
    searched range that is no leaf of its size was split; its quadrants follow in parent order)."""
    pending = [(int(r["x"]), int(r["y"])) for r in oracle.uniform_grid(case.W, case.H, case.max_size, case.max_size)]
    n = case.max_size
    while True:
        leaf = {(int(r["x"]), int(r["y"])) for r in recs[sizes == n]}
        flags = np.array([xy not in leaf for xy in pending])
        if n == level:
            return pending, flags
        h = n // 2
        pending = [q for (x, y), f in zip(pending, flags) if f
                   for q in ((x, y), (x + h, y), (x, y + h), (x + h, y + h))]
        n = h


def test_frames_have_odd_sides():
    sides = {(c.W, c.H) for c in Q.MIXED}
    assert len(sides) >= 3
    assert all(w % 16 and h % 16 and w % 8 and h % 8 for w, h in sides)
    assert any(w % 4 and h % 4 for w, h in sides)  # the first-level grid leaves a strip on both sides
    p = Q.mixed(98, 74)
    assert p.shape == (74, 98) and p.dtype == np.uint8
    assert set(np.unique(p[74 - 74 // 3:])) == {0, 60, 120}
    assert not np.array_equal(p, Q.mixed(98, 74, Q.TGT_SEED))
    # the classifier at T = 4 for (16, 4) and (8, 2), none at T = 8 (the Fourier form's flipped copies) for (16, 2)
    kinds = {(c.max_size, c.min_size, c.cls, c.T) for c in Q.MIXED}
    assert kinds == {(16, 4, True, 4), (8, 2, True, 4), (16, 2, False, 8)}


@pytest.mark.parametrize("case", Q.MIXED, ids=lambda c: c.name)
def test_mixed_levels_have_leaves_and_splits(run, case):
    recs, sizes, st, _ = run(case)
    for n in _levels(case):
        assert int((sizes == n).sum()) >= 3, f"level {n}: fewer than 3 leaves"
        if n > case.min_size:
            assert st["split"][n] >= 3, f"level {n}: fewer than 3 splits"
        assert st["searched"][n] == int((sizes == n).sum()) + st["split"][n]
    # the leaves tile the first-level grid's area once and leave the strip beyond it uncovered
    cov = _coverage(recs, sizes, case.W, case.H)
    m = case.max_size
    gw, gh = case.W // m * m, case.H // m * m
    assert gw < case.W and gh < case.H
    assert (cov[:gh, :gw] == 1).all() and cov[gh:].sum() == 0 and cov[:, gw:].sum() == 0
    # fewer leaves than the buffer bound (W/min)·(H/min)
    assert len(recs) < (case.W // case.min_size) * (case.H // case.min_size)
    if case.cls:
        assert st["rejected"] > 0
    else:
        assert st["rejected"] == 0 and st["empty"] == 0


@pytest.mark.parametrize("case", Q.EMPTY, ids=lambda c: c.name)
def test_empty_bucket_case(run, case):
    recs, sizes, st, _ = run(case)
    assert case.cls and st["empty"] > 0
    # no level is without domains here: the empty records are ranges whose own bucket is empty
    assert case.W >= 2 * case.max_size and case.H >= 2 * case.max_size


@pytest.mark.parametrize("case", Q.NODOM_SPLIT, ids=lambda c: c.name)
def test_no_domain_level_splits_every_range(oracle, run, case):
    recs, sizes, st, _ = run(case)
    assert min(case.W, case.H) < 2 * case.max_size
    nr0 = (case.W // 16) * (case.H // 16)
    if nr0 == 0:  # 15×40: a side below max_size, no range at all
        assert len(recs) == 0 and st["searched"] == {}
        return
    assert st["searched"][16] == st["split"][16] == nr0
    assert st["empty"] >= nr0 and (sizes < 16).all() and len(recs) > 0
    assert st["searched"][8] == 4 * nr0  # the later levels have domains: real records among the leaves
    assert (recs["dw"] != 0).any()


@pytest.mark.parametrize("case", Q.NODOM_LEAF, ids=lambda c: c.name)
def test_no_domain_level_leaves_are_default_records(run, case):
    recs, sizes, st, _ = run(case)
    nr0 = (case.W // 16) * (case.H // 16)
    assert len(recs) == nr0 == st["empty"]
    if nr0 == 0:
        return
    assert (sizes == 16).all() and st["split"][16] == 0
    for k, v in (("dx", 0), ("dy", 0), ("dw", 0), ("dh", 0), ("t", 0), ("dist", 1e5), ("s", 0.0), ("o", 0.0)):
        assert (recs[k] == v).all(), k


def test_no_domain_cases_cover_both_outcomes():
    assert {(c.W, c.H) for c in Q.NODOM_SPLIT} == {(c.W, c.H) for c in Q.NODOM_LEAF if c.min_size == 16} \
        == {(16, 16), (20, 20), (31, 31), (15, 40)}
    assert any(c.split > 1e5 and c.min_size < c.max_size for c in Q.NODOM_LEAF)
    assert {c.cls for c in Q.NODOM_SPLIT} == {c.cls for c in Q.NODOM_LEAF} == {False, True}


@pytest.mark.parametrize("case", Q.NORANGE, ids=lambda c: c.name)
def test_frame_below_max_size_has_no_leaves(run, case):
    recs, sizes, st, _ = run(case)
    assert min(case.W, case.H) < case.max_size
    assert len(recs) == 0 and len(sizes) == 0
    assert st == {"rejected": 0, "empty": 0, "searched": {}, "split": {}}


def test_split_extremes(oracle, run):
    recs, sizes, st, _ = run(Q.SPLIT_NONE)
    assert (sizes == 16).all() and len(recs) == (98 // 16) * (74 // 16) and st["split"] == {16: 0}
    recs, sizes, st, _ = run(Q.SPLIT_ZERO)
    lo = Q.SPLIT_ZERO.min_size
    assert (recs["dist"][sizes > lo] == 0.0).all()  # only exact matches stop above min_size …
    assert int((sizes > lo).sum()) >= 3 and (recs["dist"][sizes == lo] > 0.0).any()  # … and some do (the band)
    assert all(st["split"][n] > 0 for n in (16, 8, 4))
    assert all(st["split"][n] == st["searched"][n] for n in (16, 8))  # levels where everything splits
    split, d0 = Q.one_split_distance(oracle, Q.SPLIT_ONE)
    d = np.sort(d0)
    assert d[-2] < split < d[-1]
    recs, sizes, st, used = run(Q.SPLIT_ONE)
    assert used == split and st["split"][16] == 1 and st["searched"][8] == 4
    assert int((sizes == 16).sum()) == len(d0) - 1


def test_tile_carry(oracle, run):
    case = Q.TILE_CARRY
    recs, sizes, st, _ = run(case)
    big = [n for n in _levels(case) if st["searched"][n] > 1024 and st["split"][n] > 0]
    assert big, "no level searches more than 1,024 ranges and splits"
    n = big[0]
    pending, flags = _searched_and_split(oracle, recs, sizes, case, n)
    assert len(pending) == st["searched"][n] and int(flags.sum()) == st["split"][n]
    assert flags[:1024].any() and flags[1024:].any()
    # … and a leaf after a split in both tiles: the leaf offsets carry too
    assert (~flags[:1024]).any() and (~flags[1024:]).any()


def test_hit_threshold_case(run):
    recs, sizes, st, _ = run(Q.HIT_THR)
    assert Q.HIT_THR.thr > 0 and int((recs["dist"] <= Q.HIT_THR.thr).sum()) > 0
    # the threshold changes the search (first hit wins): other records than without it
    base, bsizes, _, _ = run(Q.BY_NAME["m98x74_16_4"])
    assert Q.HIT_THR._replace(name="m98x74_16_4", thr=0.0) == Q.BY_NAME["m98x74_16_4"]
    assert len(base) != len(recs) or any(not np.array_equal(base[k], recs[k]) for k in ("dx", "dy", "t", "dist"))


def test_two_planes_case(oracle, run):
    case = Q.TWO_PLANES
    src, tgt = case.planes()
    assert tgt is not None and src.shape == tgt.shape and not np.array_equal(src, tgt)
    recs, sizes, st, _ = run(case)
    both = [n for n in _levels(case) if st["split"][n] > 0 and int((sizes == n).sum()) > 0]
    assert both, "no level with both leaves and splits"
    # the target matters: other leaves than the source against itself
    one, osizes, _, _ = Q.run_oracle(oracle, case._replace(two_planes=False))
    assert len(one) != len(recs) or not np.array_equal(one["dist"], recs["dist"])
    # … and so does which plane the classifier reads the ranges on
    n = case.max_size
    rngs = oracle.uniform_grid(case.W, case.H, n, n)
    assert not np.array_equal(oracle.classify(src, rngs)["category"], oracle.classify(tgt, rngs)["category"])


def test_oracle_quadtree_keywords_are_compatible(oracle):
    # stats=False / tgt=None: the two-tuple of before; tgt = the plane itself: the same records
    case = Q.BY_NAME["m98x74_16_4"]
    src, _ = case.planes()
    a = oracle.quadtree(src, 16, 4, case.split, T=4, use_classifier=True)
    assert len(a) == 2
    b = oracle.quadtree(src, 16, 4, case.split, T=4, use_classifier=True, tgt=src.copy(), stats=True)
    assert len(b) == 3
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    with pytest.raises(ValueError):
        oracle.quadtree(src, 16, 4, case.split, tgt=src[:-1])


def test_sea_tiled_case(run):
    case = Q.SEA_TILED
    recs, sizes, st, _ = run(case)
    assert (case.T, case.min_size) == (4, 8) and case.cls
    assert st["split"][16] >= 3 and st["searched"][8] == 4 * st["split"][16]
    assert int((sizes == 16).sum()) >= 3 and int((sizes == 8).sum()) >= 3
    # the 8-level's ranges are no grid in raster order: quadrants in parent order
    r8 = recs[sizes == 8]
    order = np.lexsort((r8["x"], r8["y"]))
    assert not np.array_equal(order, np.arange(len(r8)))


def test_domain_count_is_the_grid_count(oracle):
    for W, H, n in ((98, 74, 16), (98, 74, 2), (130, 66, 8), (33, 47, 16), (342, 278, 4)):
        assert Q.domain_count(W, H, n) == len(oracle.uniform_grid(W, H, 2 * n, n))
    assert Q.domain_count(31, 31, 16) == 0 and Q.domain_count(15, 40, 8) == 0


def test_sequence_frames():
    assert [(c.W, c.H) for c in Q.SEQUENCE] == [(98, 74), (15, 15), (31, 31), (130, 66), (98, 74)]
    assert all(c.cls and (c.max_size, c.min_size) == (16, 4) for c in Q.SEQUENCE)
