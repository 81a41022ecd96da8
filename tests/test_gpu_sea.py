"""The SEA engine's two forms — tiled (fracenc_tp.hip + search_dft CHUNKED + resolve_dft<true>) and per-range
(sea_search, FRAC_FLAG_SEA_PER_RANGE) — against the oracle where pruning decides: winners on the edge of the
elimination window, ties and hits spread over ΣD4-sorted tiles and chunks, closed sides, whole-bucket windows
in the fp32 regime, and the seed / step / tile / chunk / block / group boundaries.

Bar: every field of FIELDS bit-exact against oracle.estimate, plus rejected_mappings, hit_ranges and
empty_ranges; search_form is asserted in every case, so a reroute to another form fails.  The frames are
sea_frames.py's; test_sea_frames.py shows on the CPU that they have the properties named here.
"""
import numpy as np
import pytest

import fractencode_amd as F
import sea_frames as SF
from golden_util import FIELDS

pytestmark = pytest.mark.gpu

FORMS = {"tiled": (0, F.FORM_SEA_MFMA), "per_range": (F.FLAG_SEA_PER_RANGE, F.FORM_SEA)}
form_param = pytest.mark.parametrize("form", list(FORMS))

_cache = {}


def _expected(oracle, key, src, tgt, n, T, cls, thr, dom_cut=None, rng_cut=None, rng_step=None, rng_every=None,
              drop_cat=False):
    """(domains, ranges, records, rejected) of the oracle, computed once per key and shared by the forms.
    Grids: domains 2n at stride n on src, ranges n at stride rng_step (n by default) on tgt, cut to their first
    dom_cut / rng_cut items or thinned to every rng_every-th; with the classifier the oracle's categories (the
    engine gets the same items); drop_cat removes the domains of the first range's category."""
    if key in _cache:
        return _cache[key]
    t = src if tgt is None else tgt
    doms = oracle.uniform_grid(src.shape[1], src.shape[0], 2 * n, n)[:dom_cut]
    rngs = oracle.uniform_grid(t.shape[1], t.shape[0], n, rng_step or n)[:rng_cut][::rng_every]
    if cls:
        doms, rngs = oracle.classify(src, doms), oracle.classify(t, rngs)
        if drop_cat:
            doms = doms[doms["category"] != rngs["category"][0]]
    want, rej, _ = oracle.estimate(src, doms, rngs, T=T, thr=thr, use_classifier=cls, tgt=tgt, threads=16)
    _cache[key] = (doms, rngs, want, rej)
    return _cache[key]


def _run(form, src, tgt, doms, rngs, T=4, cls=False, thr=0.0, engine=F.ENGINE_SEA):
    flags, want_form = FORMS[form] if form in FORMS else form
    with F.Engine(0, T, cls, thr, -1.0, engine, flags=flags) as e:
        if tgt is None:
            e.set_frame(src)
        else:
            e.set_planes(src, tgt)
        e.set_domains(doms.astype(F.GRID_ITEM))
        out, st = e.search(rngs.astype(F.GRID_ITEM))
    if engine == F.ENGINE_SEA:
        assert st["engine"] == F.ENGINE_SEA and st["search_form"] == want_form, (st["engine"], st["search_form"])
    return out, st


def _check(out, st, want, rej, thr, what):
    got = {"x": out["x"], "y": out["y"], "dx": out["dx"], "dy": out["dy"], "dw": out["sw"], "dh": out["sh"],
           "t": out["transform"], "dist": out["distance"], "s": out["contrast"], "o": out["brightness"]}
    for k in FIELDS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: field {k}")
    assert st["rejected_mappings"] == rej, what
    found = want["dw"] != 0
    assert st["empty_ranges"] == int((~found).sum()), what
    assert st["hit_ranges"] == int((found & (want["dist"] <= thr)).sum()), what


@form_param
@pytest.mark.parametrize("thr", [0.0, 1.5])
@pytest.mark.parametrize("cls", [False, True])
@pytest.mark.parametrize("frame", ["levels", "close_levels"])
def test_levels(oracle, frame, cls, thr, form):
    """Constant ranges against constant domains: the winner's error is all mean term, so it sits exactly on the
    edge of the window (tp_windows' D, sea_search's survivor and side-close tests); the least error is attained
    by many domains of one ΣD4 spread over tiles and chunks (the earliest domain must win, resolve_dft<true>
    over every chunk attaining the maximum), by two levels at both edges for |δ| = 5; δ = 0 is a hit at
    H = 0 (the HITS = false search, the first (domain, t = 0)); at thr = 1.5 the hits are |δ| ≤ 2.  On
    close_levels a range's hits have two ΣD4 values: the first in domain order can lie in a later chunk."""
    src, tgt = SF.levels(SF.LEVELS_SEED) if frame == "levels" else SF.close_levels(SF.CLOSE_LEVELS_SEED)
    doms, rngs, want, rej = _expected(oracle, (frame, cls, thr), src, tgt, 8, 4, cls, thr)
    assert len(doms) == 961 and len(rngs) == 1024
    out, st = _run(form, src, tgt, doms, rngs, cls=cls, thr=thr)
    _check(out, st, want, rej, thr, f"{frame} cls={cls} thr={thr} {form}")
    assert st["fallback_ranges"] == 0


@form_param
@pytest.mark.parametrize("thr", [0.0, 40.0, 300.0])
@pytest.mark.parametrize("cls", [False, True])
def test_flat_256(oracle, cls, thr, form):
    """The "flat" kind (4×4 cells at three levels) at 256×256, one plane, n = 8: the errors take few values, so
    nearly every range's least error is attained by many domains over 31 tiles / 8 chunks.  At n = 8 no
    range has an exact copy and the least errors are 169 and up, so thr = 40 sets H without any hit; thr = 300
    makes most ranges hits and leaves some misses."""
    p = SF.flat(SF.FLAT_SEED, 256, 256)
    doms, rngs, want, rej = _expected(oracle, ("flat", cls, thr), p, None, 8, 4, cls, thr)
    out, st = _run(form, p, None, doms, rngs, cls=cls, thr=thr)
    _check(out, st, want, rej, thr, f"flat cls={cls} thr={thr} {form}")
    assert (st["hit_ranges"] > 0) == (thr == 300.0)
    if thr == 300.0:
        assert st["hit_ranges"] < len(rngs)


@form_param
def test_smooth_partial_blocks_and_pruning(oracle, form):
    """248×200 value noise with the classifier: partial blocks at the right and bottom, several buckets with
    partial tiles, blocks and groups, narrow windows — and pruning demonstrably happened: fewer (range, domain)
    pairs evaluated than the classifier leaves eligible.  (The tiled form windows a group of 256 ranges at a
    time: here only bucket 1, with 266 ranges, has a second group, whose window is 49 of 209 domains.)"""
    p = SF.smooth(SF.SMOOTH_PRUNE_SEED, 248, 200)
    doms, rngs, want, rej = _expected(oracle, "smooth248", p, None, 8, 4, True, 0.0)
    assert len(set(doms["category"])) > 1
    out, st = _run(form, p, None, doms, rngs, cls=True)
    _check(out, st, want, rej, 0.0, f"smooth 248x200 {form}")
    assert 0 < st["evaluated_mappings"] < st["total_mappings"] - st["rejected_mappings"]


@form_param
def test_outliers_close_a_side_from_the_start(oracle, form):
    """All-0 and all-255 ranges among ordinary ones: ΣR below / above every ΣD4 (sea_search starts with one
    side closed and takes the whole seed and every step from the other; tp_seed_work picks the first / last
    tile and the window lies at one end of the bucket), still in the exact regime."""
    src, tgt, kinds = SF.outliers(SF.OUTLIERS_SEED)
    doms, rngs, want, rej = _expected(oracle, "outliers", src, tgt, 8, 4, False, 0.0)
    out, st = _run(form, src, tgt, doms, rngs)
    _check(out, st, want, rej, 0.0, f"outliers {form}")
    assert st["fallback_ranges"] == 0


@form_param
def test_fp32_regime_whole_bucket_windows(oracle, form):
    """Isolated bright blocks on black (S = 256): the bright ranges' best S16 is at least 2^24, so
    tp_seed_reduce gives up its bound (u = 0xffffffff) and their groups search the whole bucket; the records
    come from fallback_grid.  fallback_ranges equals the VALU engine's."""
    p = SF.bright_blocks(256, 8)
    doms, rngs, want, rej = _expected(oracle, "bright", p, None, 8, 4, False, 0.0)
    out, st = _run(form, p, None, doms, rngs)
    _check(out, st, want, rej, 0.0, f"bright blocks {form}")
    vout, vst = _run((0, None), p, None, doms, rngs, engine=F.ENGINE_VALU)
    assert st["fallback_ranges"] == vst["fallback_ranges"] == 64
    assert out.tobytes() == vout.tobytes()


# (first k domains, first m ranges) of a 128×128 smooth frame; the ranges come from the 8×8 grid at stride 4
# (961 of them), so that m can pass 256.  k: sea_search's 16-candidate seed and 128-candidate steps, the
# 32-domain tile and the 128-domain chunk; m: the 32-range block and the 8-block group (and sea_search's
# 4 ranges per workgroup).
EDGES = [(1, 1), (15, 31), (16, 32), (17, 33), (31, 255), (32, 256), (33, 257), (63, 33), (64, 1), (65, 257),
         (128, 32), (129, 256), (160, 257)]


@form_param
@pytest.mark.parametrize("k,m", EDGES)
def test_structural_edges(oracle, k, m, form):
    p = SF.smooth(SF.SMOOTH_SEED + 1, 128, 128)
    doms, rngs, want, rej = _expected(oracle, ("edges", k, m), p, None, 8, 4, False, 0.0, dom_cut=k, rng_cut=m,
                                      rng_step=4)
    assert len(doms) == k and len(rngs) == m
    out, st = _run(form, p, None, doms, rngs)
    _check(out, st, want, rej, 0.0, f"k={k} m={m} {form}")


@form_param
def test_empty_bucket_beside_a_large_one(oracle, form):
    """Classifier on, no domain of the first range's category, more than 128 domains (a second chunk) in
    another bucket: the empty bucket's ranges keep the default record (no group / kKeyNone)."""
    p = SF.smooth(SF.SMOOTH_SEED + 2, 256, 256)
    doms, rngs, want, rej = _expected(oracle, "emptybucket", p, None, 8, 4, True, 0.0, drop_cat=True)
    assert np.unique(doms["category"], return_counts=True)[1].max() > 128
    out, st = _run(form, p, None, doms, rngs, cls=True)
    _check(out, st, want, rej, 0.0, f"empty bucket {form}")
    assert st["empty_ranges"] > 0


@form_param
def test_second_frame_rebuilds_sort_tiles_and_windows(oracle, form):
    """set_planes(levels) then set_frame(smooth) on one engine: each run against the oracle (not against
    another SEA run), so the ΣD4 sort, the tiles and the windows of the first frame must not survive."""
    src, tgt = SF.levels(SF.LEVELS_SEED)
    p2 = SF.smooth(SF.SMOOTH_SEED + 3, 256, 256)
    doms, rngs, want1, rej1 = _expected(oracle, ("levels", False, 0.0), src, tgt, 8, 4, False, 0.0)
    _, _, want2, rej2 = _expected(oracle, "second", p2, None, 8, 4, False, 0.0)
    flags, want_form = FORMS[form]
    with F.Engine(0, 4, False, 0.0, -1.0, F.ENGINE_SEA, flags=flags) as e:
        e.set_planes(src, tgt)
        e.set_domains(doms.astype(F.GRID_ITEM))
        e.set_ranges(rngs.astype(F.GRID_ITEM))
        e.run()
        first, st1 = e.fetch()
        e.set_frame(p2)
        e.run()
        second, st2 = e.fetch()
    assert st1["search_form"] == st2["search_form"] == want_form
    _check(first, st1, want1, rej1, 0.0, f"first frame {form}")
    _check(second, st2, want2, rej2, 0.0, f"second frame {form}")


# --- per-range form only ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["flat", "smooth"])
@pytest.mark.parametrize("T", [4, 8])
@pytest.mark.parametrize("n", [2, 4])
def test_per_range_binary_search_second_iteration(oracle, n, T, kind):
    """67² = 4489 domains in one segment (n = 2 on 136², n = 4 on 272²): above 65·64 entries the 65-way search
    for ΣR takes a second iteration before the ballot."""
    S = 68 * n
    p = SF.flat(SF.FLAT_SEED + n, S, S) if kind == "flat" else SF.smooth(SF.SMOOTH_SEED + 10 + n, S, S)
    # n = 4: every 4th range keeps the oracle's share of the test near a second (the search is per range)
    doms, rngs, want, rej = _expected(oracle, ("bs", n, T, kind), p, None, n, T, False, 0.0,
                                      rng_every=4 if n == 4 else None)
    assert len(doms) == 4489 > 65 * 64
    out, st = _run((0, F.FORM_SEA), p, None, doms, rngs, T=T)
    _check(out, st, want, rej, 0.0, f"n={n} T={T} {kind}")


def test_per_range_t8_levels_hits(oracle):
    """n = 8, T = 8 runs the per-range form whatever the flags (the tiled form is T = 4 only): the levels
    frame with thr = 1.5 through sea_search<8, 8>."""
    src, tgt = SF.levels(SF.LEVELS_SEED)
    doms, rngs, want, rej = _expected(oracle, "levels_t8", src, tgt, 8, 8, False, 1.5)
    out, st = _run((0, F.FORM_SEA), src, tgt, doms, rngs, T=8, thr=1.5)
    _check(out, st, want, rej, 1.5, "levels T=8 thr=1.5")
