"""The cases of sampled_frames.py have the properties test_gpu_sampled_form.py relies on, checked on the CPU
against the oracle: a GPU test on them cannot pass vacuously.  These are conditions on the inputs (seeds and
thresholds in sampled_frames.py were picked so that the oracle alone satisfies them), not tolerances."""
import numpy as np
import pytest

import sampled_frames as SF

K_GEN_CHUNK = 4096      # fracenc_gen.hip kGenChunk
K_GEN_FB_LDS = 128 * 128  # kGenFbLds


def _est(oracle, p, doms, rngs, cls=False, tgt=None, **kw):
    if cls:
        doms, rngs = oracle.classify(p, doms), oracle.classify(p if tgt is None else tgt, rngs)
    want, rej, _ = oracle.estimate(p, doms, rngs, use_classifier=cls, tgt=tgt, threads=16, **kw)
    return want, rej


# --- A ---------------------------------------------------------------------------------------------------

def test_chunked_cases_cover_every_size_class():
    px = {c.name: c.rng[0] * c.rng[1] for c in SF.CHUNKED}
    assert px == {"65x65": 4225, "96x48": 4608, "128x128": 16384, "130x127": 16510, "256x256": 65536, "33x31": 1023}
    assert px["65x65"] % K_GEN_CHUNK == 129 and px["65x65"] // K_GEN_CHUNK == 1  # two chunks, odd tail
    assert (K_GEN_CHUNK % 96) != 0                                               # the border falls inside a row
    assert px["128x128"] == K_GEN_FB_LDS and px["130x127"] > K_GEN_FB_LDS          # the LDS / plane border
    assert px["256x256"] == 16 * K_GEN_CHUNK and px["33x31"] % 2 == 1
    for c in SF.CHUNKED:
        p, doms, rngs = SF.chunked_case(c)
        assert p.shape == (c.plane[1], c.plane[0]) and len(rngs) <= 48
        assert len(doms) * 4 == c.rows
        # every rotation of a domain samples inside the plane: max(w, h) from its origin on both axes
        M = max(2 * c.rng[0], 2 * c.rng[1])
        assert (doms["x"] + M <= c.plane[0]).all() and (doms["y"] + M <= c.plane[1]).all()
    rows = {c.name: c.rows for c in SF.CHUNKED}
    # more than 64 rows: a second, partial group of lanes in gen_search
    assert rows["65x65"] == 80 and rows["96x48"] == 100 and rows["256x256"] == 100


@pytest.mark.parametrize("case", SF.CHUNKED, ids=lambda c: c.name)
def test_chunked_cases_have_both_regimes_and_flipped_winners(oracle, case):
    p, doms, rngs = SF.chunked_case(case)
    area = 4 * case.rng[0] * case.rng[1]
    want, _ = _est(oracle, p, doms, rngs, T=4)
    found, fp32 = SF.regime(want, area)
    assert found.all()
    mix = (int((found & ~fp32).sum()), int(fp32.sum()))
    assert mix == case.mix and min(mix) >= 4
    # the exact regime's distances are whole S16 / 16 / area, below 2^24; the fp32 regime's at or above
    s16 = (want["dist"] * float(area)).astype(np.float32).astype(np.float64) * 16.0  # 16·F, as SF.regime
    assert (s16[~fp32] == np.round(s16[~fp32])).all() and (s16[~fp32] < SF.EXACT_LIMIT).all()
    assert (s16[fp32] >= SF.EXACT_LIMIT).all()
    # T = 8 with the classifier: a flipped transform wins somewhere, some range in each regime is found
    w8, _ = _est(oracle, p, doms, rngs, cls=True, T=8)
    f8, fp8 = SF.regime(w8, area)
    assert (w8["t"][f8] >= 4).any()
    assert (f8 & ~fp8).any() and fp8.any()


def test_threshold_case_has_hits_and_misses(oracle):
    case = next(c for c in SF.CHUNKED if c.name == SF.THR_CASE)
    p, doms, rngs = SF.chunked_case(case)
    area = 4 * case.rng[0] * case.rng[1]
    want, _ = _est(oracle, p, doms, rngs, T=4)
    found, fp32 = SF.regime(want, area)
    exact = np.sort(want["dist"][found & ~fp32])
    thr = SF.chunked_threshold(want, area)
    assert exact[0] < thr < exact[-1], "the threshold lies inside the exact regime's distances"
    hit, _ = _est(oracle, p, doms, rngs, T=4, thr=thr)
    assert int((hit["dist"] <= thr).sum()) >= 3 and int((hit["dist"] > thr).sum()) >= 3


def test_tail_case_is_decided_by_the_last_pixel(oracle):
    src, tgt, doms, rngs, expect = SF.tail_case()
    assert len(doms) == 9 and len(rngs) == 36 and set(expect.tolist()) == set(range(9))
    want, _, _ = oracle.estimate(src, doms, rngs, T=4, tgt=tgt, threads=16)
    np.testing.assert_array_equal(want["dx"], doms["x"][expect])
    np.testing.assert_array_equal(want["dy"], doms["y"][expect])
    assert (want["t"] == 0).all()
    delta = np.array([SF.TAIL_DELTAS[r % 4] for r in range(len(rngs))], np.float64)
    np.testing.assert_array_equal(want["dist"], (delta * delta) / (130.0 * 130.0))
    # nothing else decides: with only that pixel changed to the next domain's level, the next domain wins
    moved = tgt.copy()
    nxt = (expect + 1) % 9
    for r, it in enumerate(rngs):
        moved[int(it["y"]) + 64, int(it["x"]) + 64] = SF.TAIL_LEVELS[nxt[r]]
    other, _, _ = oracle.estimate(src, doms, rngs, T=4, tgt=moved, threads=16)
    np.testing.assert_array_equal(other["dx"], doms["x"][nxt])
    np.testing.assert_array_equal(other["dy"], doms["y"][nxt])
    assert (other["dist"] == 0.0).all()


# --- B ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", SF.TEMPLATED, ids=lambda g: "%dfrom%d" % g[:2])
def test_templated_modes(oracle, geom):
    n, S, side = geom
    assert side % n == 0 and (n, S) != (n, 2 * n)  # not the ratio-2 path
    # T = 8 on uniform noise: flipped transforms win
    p, doms, rngs, T, cls, thr = SF.templated_case(n, S, side, "t8_uniform")
    want, _ = _est(oracle, p, doms, rngs, T=T)
    assert (want["t"] >= 4).any() and (want["t"] < 4).any()
    # T = 4 with the classifier on value noise: ranges are found, mappings are rejected
    p, doms, rngs, T, cls, thr = SF.templated_case(n, S, side, "t4_cls_noise")
    want, rej = _est(oracle, p, doms, rngs, cls=True, T=T)
    assert (want["dw"] != 0).any() and rej > 0
    # the flat plane with a threshold: hits and misses, and a hit that is not the thr = 0 winner (first, not best)
    p, doms, rngs, T, cls, thr = SF.templated_case(n, S, side, "t4_thr_flat")
    assert thr > 0.0
    want, _ = _est(oracle, p, doms, rngs, T=T, thr=thr)
    best, _ = _est(oracle, p, doms, rngs, T=T)
    h = want["dist"] <= thr
    assert h.any() and (~h).any()
    np.testing.assert_array_equal(h, best["dist"] <= thr)
    # thr = 0 on the flat plane: the n = 2 geometries have exact copies (distance 0: the H = 0 path); an 8×8
    # or 16×16 range covers 4 or 16 random cells and has none
    p0, doms, rngs, T, cls, thr0 = SF.templated_case(n, S, side, "t4_thr0_flat")
    assert thr0 == 0.0
    if n == 2:
        z, _ = _est(oracle, p0, doms, rngs, T=T)
        assert (z["dist"] == 0.0).any()
    # every candidate hits at thr = 1e9: the first domain, the first transform
    p, doms, rngs, T, cls, thr = SF.templated_case(n, S, side, "t8_all_fallback")
    want, _ = _est(oracle, p, doms, rngs, T=T, thr=thr)
    assert (want["t"] == 0).all() and (want["dx"] == 0).all() and (want["dy"] == 0).all()


def test_the_plain_flat_plane_leaves_no_miss_at_2from3_and_2from5(oracle):
    """Why sampled_frames.SPECKLED exists: on the flat plane itself every range of these geometries has an exact
    copy, so a threshold mode on it would have no miss."""
    for n, S, side in SF.TEMPLATED:
        if (n, S) in SF.SPECKLED:
            p = SF.plane_of("flat", side, side, 7000 + 100 * n + S)
            doms, rngs = SF.grid(side, side, S, max(1, S // 2)), SF.grid(side, side, n, n)
            want, _ = _est(oracle, p, doms, rngs, T=4)
            assert (want["dist"] == 0.0).all()


# --- C ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", SF.OFFGRID, ids=lambda c: c.name)
def test_offgrid_cases(oracle, case):
    src, tgt, doms, rngs = SF.offgrid_case(case)
    assert src.shape[1] != tgt.shape[1] and src.shape != tgt.shape
    assert len(rngs) == case.keep
    # off every 2-, 4- and 8-pixel grid, inside their planes, not in grid order
    assert (doms["x"] % 2 == 1).any() and (doms["y"] % 2 == 1).any() and (doms["x"] % 4 != 0).any()
    assert (rngs["x"] % 2 == 1).any() and (rngs["y"] % 2 == 0).any()
    assert (doms["x"] + case.S <= src.shape[1]).all() and (doms["y"] + case.S <= src.shape[0]).all()
    assert (rngs["x"] + case.n <= tgt.shape[1]).all() and (rngs["y"] + case.n <= tgt.shape[0]).all()
    order = rngs["y"].astype(np.int64) * 4096 + rngs["x"]
    assert (np.diff(order) < 0).any()
    want, _ = _est(oracle, src, doms, rngs, T=4, tgt=tgt)
    assert (want["dw"] != 0).all()
    assert len(set(zip(want["dx"].tolist(), want["dy"].tolist()))) >= 5, "the winners are spread over the domains"
    # the records depend on which plane is which: the same grids on the source plane alone give others
    if tgt.shape[0] <= src.shape[0] and tgt.shape[1] <= src.shape[1]:
        same, _ = _est(oracle, src, doms, rngs, T=4)
        assert not np.array_equal(same["dist"], want["dist"])
    w8, rej = _est(oracle, src, doms, rngs, cls=True, T=8, tgt=tgt)
    assert (w8["dw"] != 0).any() and rej > 0 and (w8["t"] >= 4).any()
    if case.n >= 32:
        found, fp32 = SF.regime(want, case.S * case.S)
        assert fp32.sum() >= 3 and (found & ~fp32).sum() >= 3


# --- D ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", [False, True])
@pytest.mark.parametrize("geom", SF.TIE_GEOMETRIES, ids=lambda g: "%dto%d" % g)
@pytest.mark.parametrize("kind", SF.TIE_KINDS)
def test_tie_frames_are_in_the_fp32_regime_with_shared_distances(oracle, kind, geom, cls):
    """Every found range of the 0/255 frames is in the fp32 regime.  On "blocks8" at least a quarter of the
    ranges have a winner whose fp32 error another candidate shares (a float32 replay of every candidate in
    numpy, which reproduces the oracle's distances).  On "binary" no candidate shares it (measured: 0 of 64
    and 0 of 36, with and without the classifier — the 392 / 200 sums of i.i.d. pixels are all different):
    that kind pins the fp32 replay at the operands' bounds, not the ties."""
    S, n = geom
    p, doms, rngs = SF.tie_case(kind, S, n)
    if cls:
        doms, rngs = oracle.classify(p, doms), oracle.classify(p, rngs)
    want, _, _ = oracle.estimate(p, doms, rngs, T=8, use_classifier=cls, threads=16)
    found, fp32 = SF.regime(want, S * S)
    assert found.sum() >= len(rngs) - 1 and np.array_equal(found, fp32)
    F = SF.fp32_candidate_errors(p, p, doms, rngs, 8).astype(np.float64)
    if cls:
        F[rngs["category"][:, None] != doms["category"][None, :]] = np.inf
    F = F.reshape(len(rngs), -1)
    least = F.min(1)
    np.testing.assert_array_equal((least / (S * S))[found], want["dist"][found])
    shared = ((F == least[:, None]).sum(1) >= 2) & found
    if kind == "blocks8":
        assert 4 * int(shared.sum()) >= len(rngs)
        # the tie rule is visible: among equal errors of one domain the later transform wins
        assert (want["t"] >= 4).any()
