"""The sampled form (fracenc_gen.hip) against the oracle where its own paths decide: gen_search's chunked
ranges, gen_fallback's two pixel sources, the templated engines over virtual rows (Teff = 1) at n = 2, 8 and 16,
gen_fit's move to the first hitting transform, origins off the grid on two planes, and fp32-regime ties.

The bar is the project's: x, y, dx, dy, dw, dh, t, dist, s, o bit-equal to oracle.estimate and
rejected_mappings equal.  The other assertions are counts derived from the oracle's records.
test_sampled_frames.py checks on the CPU that the inputs (sampled_frames.py) reach those paths.
"""
import numpy as np
import pytest

import fractencode_amd as F
import sampled_frames as SF

pytestmark = pytest.mark.gpu

ENGINES = [F.ENGINE_VALU, F.ENGINE_MFMA, F.ENGINE_SEA]
ENGINE_IDS = {F.ENGINE_AUTO: "auto", F.ENGINE_VALU: "valu", F.ENGINE_MFMA: "mfma", F.ENGINE_SEA: "sea"}


def assert_same(got, want, what):
    g = {"x": got["x"], "y": got["y"], "dx": got["dx"], "dy": got["dy"], "dw": got["sw"], "dh": got["sh"],
         "t": got["transform"], "dist": got["distance"], "s": got["contrast"], "o": got["brightness"]}
    for k in SF.FIELDS:
        np.testing.assert_array_equal(g[k], want[k], err_msg=f"{what}: field {k}")


def run(src, doms, rngs, T, cls, thr, engine, tgt=None, smax=-1.0, again=False):
    """One search through the C ABI; with `again` a second search on the same context, whose bytes must equal
    the first's."""
    with F.Engine(0, T, cls, thr, smax, engine) as e:
        if tgt is None:
            e.set_frame(src)
        else:
            e.set_planes(src, tgt)
        e.set_domains(doms.astype(F.GRID_ITEM))
        out, st = e.search(rngs.astype(F.GRID_ITEM))
        if again:
            out2, st2 = e.search(rngs.astype(F.GRID_ITEM))
            assert out.tobytes() == out2.tobytes(), "a second search on the context differs"
            assert st2["rejected_mappings"] == st["rejected_mappings"]
    return out, st


def classified(oracle, src, doms, rngs, tgt=None):
    """Categories by the oracle (domains on the source plane, ranges on the target), checked against the
    engine's preclassify so both sides search the same buckets."""
    d, r = oracle.classify(src, doms), oracle.classify(src if tgt is None else tgt, rngs)
    np.testing.assert_array_equal(F.preclassify(src, doms.astype(F.GRID_ITEM))["category"], d["category"])
    np.testing.assert_array_equal(F.preclassify(src if tgt is None else tgt, rngs.astype(F.GRID_ITEM))["category"],
                                  r["category"])
    return d, r


# --- A. chunked and large generic ranges -----------------------------------------------------------------

_chunk_cache = {}


def _chunk_reference(oracle, case, T, cls, thr_mode):
    """The case's inputs and the oracle's records, computed once and shared by the engines' tests."""
    key = (case.name, T, cls, thr_mode)
    if key not in _chunk_cache:
        p, doms, rngs = SF.chunked_case(case)
        area = 4 * case.rng[0] * case.rng[1]
        if cls:
            doms, rngs = classified(oracle, p, doms, rngs)
        thr = 0.0
        if thr_mode:
            best, _, _ = oracle.estimate(p, doms, rngs, T=T, use_classifier=cls, threads=16)
            thr = SF.chunked_threshold(best, area)
        want, rej, _ = oracle.estimate(p, doms, rngs, T=T, thr=thr, use_classifier=cls, threads=16)
        for a in (p, doms, rngs, want):
            a.setflags(write=False)
        _chunk_cache[key] = (p, doms, rngs, area, thr, want, rej)
    return _chunk_cache[key]


def _check_chunked(oracle, case, T, cls, thr_mode, engine):
    p, doms, rngs, area, thr, want, rej = _chunk_reference(oracle, case, T, cls, thr_mode)
    out, st = run(p, doms, rngs, T, cls, thr, engine)
    what = f"{case.name} T={T} cls={cls} thr={thr} {ENGINE_IDS[engine]}"
    assert st["search_form"] == F.FORM_SAMPLED, what
    assert_same(out, want, what)
    assert st["rejected_mappings"] == rej, what
    # Derived, not measured.  A sequential fp32 sum of non-negative multiples of 1/16 is exact below 2^24 (in
    # S16 units) and stays at or above 2^24 once the true sum is: so the engine's regime test on the exact S16
    # of its least-error candidate and the oracle's winner agree on the regime.  (A hit is never in the fp32
    # regime here: the threshold lies inside the exact regime.)
    found, fp32 = SF.regime(want, area)
    assert st["fallback_ranges"] == int(fp32.sum()), what
    assert st["empty_ranges"] == int((~found).sum()), what
    return st, want, thr, found


@pytest.mark.parametrize("engine", [F.ENGINE_AUTO, F.ENGINE_VALU], ids=lambda e: ENGINE_IDS[e])
@pytest.mark.parametrize("T,cls", SF.CHUNK_MODES)
@pytest.mark.parametrize("case", SF.CHUNKED, ids=lambda c: c.name)
def test_chunked_and_large_generic_ranges(oracle, case, T, cls, engine):
    """gen_search streaming a range of more than 4096 pixels through LDS in chunks (odd tail, a border in
    mid-row, 4 and 16 whole chunks, a partial last group of rows), gen_fit's regime test and list, and
    gen_fallback reading the range from LDS (up to 128·128 pixels) or from the plane (above)."""
    _check_chunked(oracle, case, T, cls, False, engine)


@pytest.mark.parametrize("engine", [F.ENGINE_AUTO, F.ENGINE_VALU], ids=lambda e: ENGINE_IDS[e])
def test_chunked_range_with_a_hit_threshold(oracle, engine):
    """65×65 with a threshold inside the exact regime's distances: gen_search's hit keys over two chunks,
    gen_fit's first hitting transform, and the hit count (the oracle's ranges with dist ≤ thr; thr > 0)."""
    case = next(c for c in SF.CHUNKED if c.name == SF.THR_CASE)
    st, want, thr, found = _check_chunked(oracle, case, 4, False, True, engine)
    assert thr > 0.0
    assert st["hit_ranges"] == int((found & (want["dist"] <= thr)).sum())


@pytest.mark.parametrize("engine", [F.ENGINE_AUTO, F.ENGINE_VALU], ids=lambda e: ENGINE_IDS[e])
def test_last_pixel_of_the_odd_tail_decides(oracle, engine):
    """65×65 ranges that differ from every domain in their last pixel only (sampled_frames.tail_case): gen_search's
    second chunk ends in a pair with one pixel (q + 1 < ce), and that pixel alone picks the domain.  The other
    chunked cases reach this pair too, but there 4224 other pixels outvote it."""
    src, tgt, doms, rngs, expect = SF.tail_case()
    want, rej, _ = oracle.estimate(src, doms, rngs, T=4, tgt=tgt, threads=16)
    out, st = run(src, doms, rngs, 4, False, 0.0, engine, tgt=tgt)
    assert st["search_form"] == F.FORM_SAMPLED
    assert_same(out, want, f"tail {ENGINE_IDS[engine]}")
    np.testing.assert_array_equal(out["dx"], doms["x"][expect])
    np.testing.assert_array_equal(out["dy"], doms["y"][expect])
    assert st["fallback_ranges"] == 0 and st["empty_ranges"] == 0


# --- B. templated sizes in the sampled form --------------------------------------------------------------

_templ_cache = {}


def _templ_reference(oracle, geom, mode):
    key = (geom, mode)
    if key not in _templ_cache:
        n, S, side = geom
        p, doms, rngs, T, cls, thr = SF.templated_case(n, S, side, mode)
        if cls:
            doms, rngs = classified(oracle, p, doms, rngs)
        want, rej, _ = oracle.estimate(p, doms, rngs, T=T, thr=thr, use_classifier=cls, threads=16)
        for a in (p, doms, rngs, want):
            a.setflags(write=False)
        _templ_cache[key] = (p, doms, rngs, T, cls, thr, want, rej)
    return _templ_cache[key]


@pytest.mark.parametrize("engine", ENGINES, ids=lambda e: ENGINE_IDS[e])
@pytest.mark.parametrize("mode", list(SF.MODES))
@pytest.mark.parametrize("geom", SF.TEMPLATED, ids=lambda g: "%dfrom%d" % g[:2])
def test_templated_sizes_in_the_sampled_form(oracle, geom, mode, engine):
    """n = 2, 8, 16 with domains that are not 2n: gen_pool_build's rows at (x·⌊S/n⌋, y·⌊S/n⌋), the engines'
    Teff = 1 searches over them, gen_fit's fit at ((x·S)/n, (y·S)/n) and its move of a hit to the first
    transform of its domain that meets the threshold, and gen_fallback alone at thr = 1e9."""
    n, S, side = geom
    p, doms, rngs, T, cls, thr, want, rej = _templ_reference(oracle, geom, mode)
    out, st = run(p, doms, rngs, T, cls, thr, engine)
    what = f"{n} from {S}, {mode}, {ENGINE_IDS[engine]}"
    assert_same(out, want, what)
    assert st["rejected_mappings"] == rej, what
    found = want["dw"] != 0
    assert st["empty_ranges"] == int((~found).sum()), what
    if mode == "t8_all_fallback":
        assert st["fallback_ranges"] == int(found.sum()), what  # every range through gen_fallback
    else:
        # SEA covers n ≤ 8: n = 16 runs the exhaustive MFMA search
        assert st["engine"] == (F.ENGINE_MFMA if engine == F.ENGINE_SEA and n == 16 else engine), what
    # the oracle's ranges with dist ≤ thr; at thr = 0 those are the exact copies (H = 0)
    assert st["hit_ranges"] == int((found & (want["dist"] <= thr)).sum()), what


# --- C. off the grid -------------------------------------------------------------------------------------

def _offgrid_params():
    out = []
    for c in SF.OFFGRID:
        for eng in (ENGINES if c.n in (2, 4, 8, 16) else [F.ENGINE_AUTO]):
            for cls in (False, True):
                out.append(pytest.param(c, eng, cls, id=f"{c.name}-{ENGINE_IDS[eng]}-{'cls' if cls else 'nocls'}"))
    return out


@pytest.mark.parametrize("case,engine,cls", _offgrid_params())
def test_off_the_grid_on_two_planes(oracle, case, engine, cls):
    """Domains from (3, 5) and ranges from (1, 2) with odd steps, a source and a target plane of different
    widths (categories per plane), a permuted and truncated range list (records in the caller's order) and a
    second search on the context: gen_sample, gen_s16 and gen_search's loader with their own strides."""
    src, tgt, doms, rngs = SF.offgrid_case(case)
    T = 8 if cls else 4
    if cls:
        doms, rngs = classified(oracle, src, doms, rngs, tgt)
    want, rej, _ = oracle.estimate(src, doms, rngs, T=T, use_classifier=cls, tgt=tgt, threads=16)
    out, st = run(src, doms, rngs, T, cls, 0.0, engine, tgt=tgt, again=True)
    what = f"{case.name} cls={cls} {ENGINE_IDS[engine]}"
    np.testing.assert_array_equal(out["x"], rngs["x"], err_msg=what)
    np.testing.assert_array_equal(out["y"], rngs["y"], err_msg=what)
    assert_same(out, want, what)
    assert st["rejected_mappings"] == rej, what
    found, fp32 = SF.regime(want, case.S * case.S)
    assert st["fallback_ranges"] == int(fp32.sum()) and st["empty_ranges"] == int((~found).sum()), what


# --- D. fp32-regime ties ---------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", [False, True], ids=["nocls", "cls"])
@pytest.mark.parametrize("geom", SF.TIE_GEOMETRIES, ids=lambda g: "%dto%d" % g)
@pytest.mark.parametrize("kind", SF.TIE_KINDS)
def test_fp32_regime_ties(oracle, kind, geom, cls):
    """0/255 frames at 48→24 and 64→32, T = 8: every found range is settled by gen_fallback, where candidates
    share their fp32 error on "blocks8" — the earliest domain wins, then the later transform."""
    S, n = geom
    p, doms, rngs = SF.tie_case(kind, S, n)
    if cls:
        doms, rngs = classified(oracle, p, doms, rngs)
    want, rej, _ = oracle.estimate(p, doms, rngs, T=8, use_classifier=cls, threads=16)
    out, st = run(p, doms, rngs, 8, cls, 0.0, F.ENGINE_AUTO)
    what = f"{kind} {S}→{n} cls={cls}"
    assert st["search_form"] == F.FORM_SAMPLED
    assert_same(out, want, what)
    assert st["rejected_mappings"] == rej, what
    found = want["dw"] != 0
    assert st["fallback_ranges"] == int(found.sum()) and st["empty_ranges"] == int((~found).sum()), what
