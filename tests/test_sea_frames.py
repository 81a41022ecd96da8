"""The frames of sea_frames.py have the properties test_gpu_sea.py relies on, checked on the CPU against the
oracle: a GPU test on them cannot pass vacuously.  These are conditions on the inputs (the seeds in
sea_frames.py were picked so that the oracle alone satisfies them), not tolerances."""
import numpy as np
import pytest

import sea_frames as SF

S = 256
THR = 1.5
H_THR = 6144  # the largest S16 with (S16/16)/256 <= 1.5


def _oracle_run(oracle, src, tgt, thr):
    doms = oracle.uniform_grid(src.shape[1], src.shape[0], 16, 8)
    rngs = oracle.uniform_grid(tgt.shape[1], tgt.shape[0], 8, 8)
    want, _, _ = oracle.estimate(src, doms, rngs, T=4, thr=thr, tgt=tgt, threads=16)
    return doms, rngs, want


def _domain_index(doms, want):
    key = {(int(d["x"]), int(d["y"])): i for i, d in enumerate(doms)}
    return np.array([key[(int(x), int(y))] for x, y in zip(want["dx"], want["dy"])])


def _sorted_chunk(sd):
    """128-domain chunk (4 tiles of 32) of every domain in the ΣD4-sorted order (stable: equal sums keep the
    domain order, as the engine's radix sort of (ΣD4, position) does)."""
    order = np.argsort(sd, kind="stable")
    chunk = np.empty(len(sd), np.int64)
    chunk[order] = np.arange(len(sd)) // 128
    return chunk


@pytest.fixture(scope="module")
def lv():
    src, tgt = SF.levels(SF.LEVELS_SEED)
    E, a, sd, const = SF.constant_errors(src, tgt)
    present = np.unique(src).astype(np.int64)
    delta = np.abs(a[:, None] - present[None, :]).min(1)
    return dict(src=src, tgt=tgt, E=E, a=a, sd=sd, const=const, delta=delta, chunk=_sorted_chunk(sd))


def test_levels_geometry(lv):
    src, tgt = lv["src"], lv["tgt"]
    assert src.shape == tgt.shape == (S, S) and not np.array_equal(src, tgt)
    assert set(np.unique(src)) <= set(range(20, 221, 10))
    assert lv["E"].shape == (1024, 961)  # 31 tiles of 32, 8 chunks of 4 tiles
    assert lv["chunk"].max() == 7
    assert set(np.unique(lv["delta"])) == {0, 1, 2, 3, 4, 5}
    # the analysis of sea_frames.levels: the least error is 1024·δ², attained by constant domains only
    np.testing.assert_array_equal(lv["E"].min(1), 1024 * lv["delta"] ** 2)
    assert lv["const"][np.nonzero(lv["E"] == lv["E"].min(1)[:, None])[1]].all()
    assert lv["E"].min(1).max() < (1 << 24)


def test_levels_winners_are_constant_domains_on_the_window_edge(oracle, lv):
    doms, rngs, want = _oracle_run(oracle, lv["src"], lv["tgt"], 0.0)
    d = _domain_index(doms, want)
    assert lv["const"][d].all(), "every range's winner is a constant domain"
    np.testing.assert_array_equal(want["dist"], 1024.0 * lv["delta"] ** 2 / 4096.0)
    # the oracle's winner is the first domain attaining the least error of the numpy model
    np.testing.assert_array_equal(d, (lv["E"] == lv["E"].min(1)[:, None]).argmax(1))
    # exact copies take the first transform (a hit at thr = 0), the other ties the last
    assert (want["t"][lv["delta"] == 0] == 0).all() and (want["t"][lv["delta"] > 0] == 3).all()


def test_levels_ties_fall_in_different_chunks(lv):
    E, chunk, delta = lv["E"], lv["chunk"], lv["delta"]
    att = E == E.min(1)[:, None]
    spread = np.array([len(set(chunk[np.flatnonzero(row)])) for row in att])
    for dv in range(6):
        assert (spread[delta == dv] >= 2).any(), f"|δ| = {dv}: no range with ties in two chunks"
    # … and for some range the winner (least domain index) is not in the first of those chunks
    first = att.argmax(1)
    later = [chunk[first[r]] > chunk[np.flatnonzero(att[r])].min() for r in range(len(att))]
    assert any(later)
    # |δ| = 5 ties two levels: attaining domains on both sides of ΣR
    two = [len(set(lv["sd"][np.flatnonzero(att[r])])) == 2 for r in np.flatnonzero(delta == 5)]
    assert any(two)


def test_levels_hit_set_at_thr_1_5(oracle, lv):
    doms, rngs, want = _oracle_run(oracle, lv["src"], lv["tgt"], THR)
    np.testing.assert_array_equal(want["dist"] <= THR, lv["delta"] <= 2)
    hits = lv["E"] <= H_THR
    np.testing.assert_array_equal(hits.any(1), lv["delta"] <= 2)
    d = _domain_index(doms, want)
    h = lv["delta"] <= 2
    np.testing.assert_array_equal(d[h], hits.argmax(1)[h])  # the first hit in domain order
    assert (want["t"][h] == 0).all()
    # all hits of a range share one ΣD4 here, and the stable sort keeps their domain order: the first hit is
    # always in the first chunk that holds one.  close_levels (below) is the frame where it is not.
    for r in np.flatnonzero(h):
        assert len(set(lv["sd"][np.flatnonzero(hits[r])])) == 1


def test_close_levels_first_hit_is_in_a_later_chunk(oracle):
    src, tgt = SF.close_levels(SF.CLOSE_LEVELS_SEED)
    E, a, sd, const = SF.constant_errors(src, tgt)
    chunk = _sorted_chunk(sd)
    doms, rngs, want = _oracle_run(oracle, src, tgt, THR)
    assert (want["dist"] <= THR).all()  # every range is a hit
    hits = E <= H_THR
    assert const[np.nonzero(hits)[1]].all()
    first = hits.argmax(1)
    np.testing.assert_array_equal(_domain_index(doms, want), first)
    later = np.array([chunk[first[r]] > chunk[np.flatnonzero(hits[r])].min() for r in range(len(hits))])
    assert later.any(), "no range whose first hit (domain order) sorts into a later chunk than another hit"
    # at thr = 0 the δ = ±2 ranges tie two levels, one on each edge of the window
    att = E == E.min(1)[:, None]
    assert any(len(set(sd[np.flatnonzero(att[r])])) == 2 for r in range(len(att)))


def test_outliers_close_one_side_and_stay_exact(oracle):
    src, tgt, kinds = SF.outliers(SF.OUTLIERS_SEED)
    assert src.min() == 64 and src.max() == 192
    doms, rngs, want = _oracle_run(oracle, src, tgt, 0.0)
    s = src.astype(np.int64)
    sd = np.array([s[int(d["y"]):int(d["y"]) + 16, int(d["x"]):int(d["x"]) + 16].sum() for d in doms])
    t = tgt.astype(np.int64)
    sr = np.array([4 * t[int(r["y"]):int(r["y"]) + 8, int(r["x"]):int(r["x"]) + 8].sum() for r in rngs])
    k = kinds.reshape(-1)
    assert (k < 0).sum() >= 8 and (k > 0).sum() >= 8 and (k == 0).sum() >= 100
    assert (sr[k < 0] < sd.min()).all() and (sr[k > 0] > sd.max()).all()
    assert ((sr[k == 0] >= sd.min()) & (sr[k == 0] <= sd.max())).all()
    assert (want["dist"] * 4096.0 < (1 << 24)).all(), "every range in the exact regime"
    assert (want["dist"][k != 0] * 4096.0 >= 64 * (4 * 63) ** 2).all()


def test_bright_blocks_are_in_the_fp32_regime(oracle):
    p = SF.bright_blocks()
    doms, rngs, want = _oracle_run(oracle, p, p, 0.0)
    bright = np.array([p[int(r["y"]), int(r["x"])] == 255 for r in rngs])
    assert bright.sum() == 64
    assert (want["dist"][bright] * 4096.0 >= (1 << 24)).all() and (want["dist"][~bright] == 0.0).all()
