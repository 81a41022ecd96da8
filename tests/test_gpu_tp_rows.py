"""The tiled form reads the planes once, before its sort: tp_keys forms every pool row, −ΣD4² and both sides' sort
keys in pool and range order and copies every range's 64 pixels (rpix); after the sort tp_prep builds a tile per wave
from one gathered pool row per tile row and a block from one gathered rpix row per slot, with the tile guards and the
fast epilogue's thresholds from a wave reduction (fracenc_tp.hip).

Every case runs on ENGINE_SEA and on AUTO | FLAG_PRUNE and compares the records field for field and byte for byte
with ENGINE_VALU (another writer, which never sorts) or the oracle, hit_ranges and fallback_ranges with that run's,
and — where a context is reused — every statistic, evaluated_mappings included, with a fresh context's on the same
route.  The tie frames also hold evaluated_mappings and matrix_flops to the restated window rule
(test_gpu_tp_records._check).

  tile and workgroup edges   domain lists of 1, 31, 32, 33, 127, 128 and 129 domains (partial tiles, padding rows, a
                             workgroup of four tiles partly empty) on 64×64 and 70×58, range lists of 1, 31, 32, 33
                             and 129, an empty domain list and an empty range list;
  both load branches         origins on the 8-pixel grid; odd origins on 70×58 and 264×248 (the byte-wise branch of the
                             pool rows and of rpix); separate source and target planes of different widths;
  buckets                    the classifier on; one category's domains left out (an empty bucket: ranges with no
                             eligible domain); a bucket of fewer than 32 domains;
  pool and −ΣD4²             fallback_probe.frame(6, 512)'s fp32-regime ranges (distance ≥ 4,096), which fallback_grid
                             fits from the rows the pixel pass now writes before the sort;
  equal keys                 every tp_tie_frames case, and a constant frame (all ΣD4 equal: one window holds all);
  reuse                      two frames alternating, a changed domain list then a changed range list, and a noise
                             frame (over AUTO's budget: the exhaustive search in the same run) before and after a frame
                             that prunes, each run against a fresh context.

test_keys_are_the_sums (CPU) holds the two identities the kernels rely on, for every plane and list above."""
import numpy as np
import pytest

import auto_prune_frames as A
import fractencode_amd as F
import test_gpu_sink_stores as SS
import test_gpu_tp_records as TR
import tp_tie_frames as T

gpu = pytest.mark.gpu

ROUTES = {"sea": TR.SEA, "auto_prune": TR.AUTO_PRUNE}
route_param = pytest.mark.parametrize("route", list(ROUTES))
STATS = ("hit_ranges", "fallback_ranges", "evaluated_mappings")

_planes, _refs = {}, {}


def _plane(name):
    if name not in _planes:
        _planes[name] = {
            "m64": lambda: A.mosaic(64, 64, amp=2),
            "m70": lambda: A.mosaic(70, 58, amp=2, noise_seed=3),
            "m64b": lambda: A.mosaic(64, 58, amp=3, noise_seed=7),
            "n70": lambda: A.noise(70, 58),
            "const64": lambda: np.full((64, 64), 93, np.uint8),
            "noise256": lambda: A.noise(256, 256),
        }.get(name, lambda: SS._plane(name))()
    return _planes[name]


def _grid(W, H, size, step, x0=0, y0=0):
    """size × size items at (x0 + i·step, y0 + j·step) inside W × H, row-major."""
    ys, xs = np.meshgrid(np.arange(y0, H - size + 1, step), np.arange(x0, W - size + 1, step), indexing="ij")
    g = np.zeros(xs.size, dtype=F.GRID_ITEM)
    g["x"], g["y"], g["w"], g["h"] = xs.ravel(), ys.ravel(), size, size
    return g


def _lists(name, odd=False, step=8):
    H, W = _plane(name).shape
    o = 1 if odd else 0
    return _grid(W, H, 16, step, o, o), _grid(W, H, 8, 8, o, o)


def _run(route, src, tgt, doms, rngs, cls=False, thr=0.0):
    """(records, stats, tuples) of a fresh context on a route."""
    engine, flags = route
    with F.Engine(0, 4, cls, thr, -1.0, engine, flags=flags) as e:
        e.set_planes(src, tgt) if tgt is not None else e.set_frame(src)
        e.set_domains(doms)
        e.set_ranges(rngs)
        e.run()
        out, st = e.fetch()
        return out, st, e.fetch_tuples()


def _reference(key, src, tgt, doms, rngs, cls=False, thr=0.0):
    """ENGINE_VALU's records, stats and tuples of a case, once."""
    if key not in _refs:
        _refs[key] = _run((F.ENGINE_VALU, 0), src, tgt, doms, rngs, cls, thr)
    return _refs[key]


def _same_records(out, want, what):
    for k in F.ENCODE_ITEM.names:
        np.testing.assert_array_equal(out[k], want[k], err_msg=f"{what}: field {k}")
    assert out.tobytes() == want.tobytes(), what


def _agree(got, ref, what):
    out, st, tuples = got
    want, wst, wtuples = ref
    _same_records(out, want, what)
    np.testing.assert_array_equal(tuples["domain"], wtuples["domain"], err_msg=f"{what}: tuple domain")
    assert (st["hit_ranges"], st["fallback_ranges"]) == (wst["hit_ranges"], wst["fallback_ranges"]), what


def _case(route, key, name, doms, rngs, cls=False, thr=0.0, tgt=None):
    src = _plane(name)
    ref = _reference((key, cls, thr), src, tgt, doms, rngs, cls, thr)
    got = _run(ROUTES[route], src, tgt, doms, rngs, cls, thr)
    _agree(got, ref, f"{key} {route}")
    return got, ref


# ---- 1: tile and workgroup edges -------------------------------------------------------------------------------------

def _many_domains(name, nd):
    """nd domains: the stride-8 grid, then the stride-4 grid's further origins (129 is more than either frame's
    stride-8 grid holds)."""
    H, W = _plane(name).shape
    a, b = _grid(W, H, 16, 8), _grid(W, H, 16, 4)
    extra = b[(b["x"] % 8 != 0) | (b["y"] % 8 != 0)]
    d = np.concatenate([a, extra])[:nd]
    assert len(d) == nd
    return np.ascontiguousarray(d)


def _many_ranges(name, nr):
    """nr ranges: the 8-grid, then the grids shifted by (4, 2) and (2, 4) (129 is more than the 8-grid holds)."""
    H, W = _plane(name).shape
    r = np.concatenate([_grid(W, H, 8, 8), _grid(W, H, 8, 8, 4, 2), _grid(W, H, 8, 8, 2, 4)])[:nr]
    assert len(r) == nr
    return np.ascontiguousarray(r)


@gpu
@route_param
@pytest.mark.parametrize("name", ["m64", "m70"])
@pytest.mark.parametrize("nd", [1, 31, 32, 33, 127, 128, 129])
def test_domain_list_edges(nd, name, route):
    _, rngs = _lists(name)
    _case(route, ("doms", name, nd), name, _many_domains(name, nd), rngs)


@gpu
@route_param
@pytest.mark.parametrize("name", ["m64", "m70"])
@pytest.mark.parametrize("nr", [1, 31, 32, 33, 129])
def test_range_list_edges(nr, name, route):
    doms, _ = _lists(name)
    rngs = _many_ranges(name, nr)
    _case(route, ("rngs", name, nr), name, doms, rngs)


@gpu
@route_param
@pytest.mark.parametrize("empty", ["domains", "ranges"])
def test_empty_lists(empty, route):
    doms, rngs = _lists("m64")
    if empty == "domains":
        doms = doms[:0]
    else:
        rngs = rngs[:0]
    (out, st, tuples), _ = _case(route, ("empty", empty), "m64", doms, rngs)
    assert len(out) == len(rngs)
    assert bool((tuples["domain"] == F.NO_DOMAIN).all())


# ---- 2: both load branches -------------------------------------------------------------------------------------------

@gpu
@route_param
@pytest.mark.parametrize("name,odd", [("m70", False), ("m70", True), ("n70", True), ("mosaic264", False),
                                      ("mosaic264", True)])
def test_load_branches(name, odd, route):
    doms, rngs = _lists(name, odd)
    assert bool(((doms["x"] % 2 == 1) == odd).all()) and bool(((rngs["x"] % 2 == 1) == odd).all())
    _case(route, ("branch", name, odd), name, doms, rngs)


@gpu
@route_param
@pytest.mark.parametrize("odd", [False, True])
def test_separate_planes_of_different_strides(odd, route):
    """Source 70 wide, target 64 wide: the pool rows come through one stride, rpix through another."""
    src, tgt = _plane("m70"), _plane("m64b")
    o = 1 if odd else 0
    doms, rngs = _grid(70, 58, 16, 8, o, o), _grid(64, 58, 8, 8, o, o)
    _case(route, ("planes", odd), "m70", doms, rngs, tgt=tgt)


# ---- 3: buckets ------------------------------------------------------------------------------------------------------

_bucket_cases = {}


def _buckets(oracle, what):
    if what not in _bucket_cases:
        p = _plane("mosaic264")
        doms, rngs = _lists("mosaic264")
        doms = oracle.classify(p, doms).astype(F.GRID_ITEM)
        rngs = oracle.classify(p, rngs).astype(F.GRID_ITEM)
        cats, counts = np.unique(doms["category"], return_counts=True)
        if what == "left_out":  # the most frequent range category that has domains loses them
            rc = [int((rngs["category"] == c).sum()) for c in cats]
            gone = cats[int(np.argmax(rc))]
            assert bool((rngs["category"] == gone).any())
            doms = np.ascontiguousarray(doms[doms["category"] != gone])
        elif what == "small":   # the largest bucket is cut to 20 domains: fewer than a tile
            big = cats[int(np.argmax(counts))]
            keep = np.ones(len(doms), bool)
            keep[np.flatnonzero(doms["category"] == big)[20:]] = False
            doms = np.ascontiguousarray(doms[keep])
            assert int((doms["category"] == big).sum()) == 20
        _bucket_cases[what] = (doms, rngs)
    return _bucket_cases[what]


@gpu
@route_param
@pytest.mark.parametrize("what", ["all", "left_out", "small"])
def test_buckets(oracle, what, route):
    doms, rngs = _buckets(oracle, what)
    (out, st, tuples), (_, wst, _) = _case(route, ("buckets", what), "mosaic264", doms, rngs, cls=True)
    assert st["empty_ranges"] == wst["empty_ranges"]
    if what == "left_out":
        assert st["empty_ranges"] > 0


# ---- 4: the pool rows and −ΣD4² as fallback_grid reads them ----------------------------------------------------------

@gpu
@route_param
def test_fp32_regime_ranges_read_the_early_rows(route):
    p = _plane("fallback512")
    doms, rngs = SS._grids(p)
    want, wst = SS._reference("fallback512")
    out, st, _ = _run(ROUTES[route], p, None, doms, rngs)
    far = want["distance"] * 4096.0 >= float(1 << 24)
    assert int(far.sum()) > 0 and wst["fallback_ranges"] == int(far.sum())
    _same_records(out, want, f"fallback512 {route}")
    _same_records(out[far], want[far], f"fallback512 {route}: the fp32-regime ranges")
    assert (st["hit_ranges"], st["fallback_ranges"]) == (wst["hit_ranges"], wst["fallback_ranges"])


# ---- 5: equal keys ---------------------------------------------------------------------------------------------------

@gpu
@route_param
@pytest.mark.parametrize("name", list(T.CASES))
def test_tie_frames(oracle, name, route):
    src, tgt, thr = TR._frame(name)
    doms, rngs = TR._items(oracle, src, tgt, False)
    ref = TR._reference(oracle, (name, False, thr, None), src, tgt, doms, rngs, False, thr)
    r = ROUTES[route]
    with F.Engine(0, 4, False, thr, -1.0, r[0], flags=r[1]) as e:
        e.set_planes(src, tgt)
        e.set_domains(doms.astype(F.GRID_ITEM))
        e.set_ranges(rngs.astype(F.GRID_ITEM))
        out, st, tuples = TR._run(e, len(rngs), None)
    TR._check(out, st, tuples, ref, r, f"{name} route={route}")


@gpu
@route_param
def test_constant_frame(route):
    """All ΣD4 and all ΣR equal: the stable sort keeps the list order and one window holds every tile."""
    doms, rngs = _lists("const64")
    (out, st, tuples), _ = _case(route, ("const",), "const64", doms, rngs)
    assert bool((out["distance"] == 0).all())


# ---- 6: reuse on one context -----------------------------------------------------------------------------------------

def _fresh(route, key, name, doms, rngs):
    k = ("fresh", route, key)
    if k not in _refs:
        _refs[k] = _run(ROUTES[route], _plane(name), None, doms, rngs)
    return _refs[k]


def _step(e, route, key, name, doms, rngs, what):
    """The context's current state, run, against ENGINE_VALU and against a fresh context on the same route."""
    e.run()
    out, st = e.fetch()
    got = (out, st, e.fetch_tuples())
    _agree(got, _reference((key, False, 0.0), _plane(name), None, doms, rngs), what)
    fout, fst, ftuples = _fresh(route, key, name, doms, rngs)
    assert out.tobytes() == fout.tobytes() and got[2].tobytes() == ftuples.tobytes(), what
    for k in STATS + ("search_form", "empty_ranges", "matrix_flops"):
        assert st[k] == fst[k], f"{what}: {k} {st[k]} against a fresh context's {fst[k]}"
    return st


@gpu
@route_param
def test_two_frames_alternate(route):
    names = ["mosaic256", "mosaic256b"]
    doms, rngs = SS._grids(_plane(names[0]))
    engine, flags = ROUTES[route]
    with F.Engine(0, 4, False, 0.0, -1.0, engine, flags=flags) as e:
        e.set_domains(doms)
        e.set_ranges(rngs)
        for k in range(4):
            e.set_frame(_plane(names[k & 1]))
            _step(e, route, ("alt", names[k & 1]), names[k & 1], doms, rngs, f"{route} frame {k}")


@gpu
@route_param
def test_changed_lists(route):
    name = "m70"
    doms, rngs = _lists(name)
    fewer_doms, odd_rngs = _many_domains(name, 33), _lists(name, odd=True)[1]
    engine, flags = ROUTES[route]
    with F.Engine(0, 4, False, 0.0, -1.0, engine, flags=flags) as e:
        e.set_frame(_plane(name))
        e.set_domains(doms)
        e.set_ranges(rngs)
        _step(e, route, ("lists", 0), name, doms, rngs, f"{route}: first lists")
        e.set_domains(fewer_doms)
        _step(e, route, ("lists", 1), name, fewer_doms, rngs, f"{route}: changed domains")
        e.set_ranges(odd_rngs)
        _step(e, route, ("lists", 2), name, fewer_doms, odd_rngs, f"{route}: changed ranges")
        e.set_domains(doms)
        _step(e, route, ("lists", 3), name, doms, odd_rngs, f"{route}: the first domains again")


@gpu
@route_param
@pytest.mark.parametrize("order", [("noise256", "mosaic256", "noise256"), ("mosaic256", "noise256", "mosaic256")],
                         ids=["noise_first", "mosaic_first"])
def test_fallback_and_pruned_runs_alternate(order, route):
    """Under AUTO | FLAG_PRUNE the noise frame's windows are over the budget: launch_dft rebuilds every frame-derived
    buffer after tp_keys and tp_prep wrote theirs, and the next frame prunes on the same context (and the reverse)."""
    doms, rngs = SS._grids(_plane("mosaic256"))
    engine, flags = ROUTES[route]
    with F.Engine(0, 4, False, 0.0, -1.0, engine, flags=flags) as e:
        e.set_domains(doms)
        e.set_ranges(rngs)
        for k, name in enumerate(order):
            e.set_frame(_plane(name))
            st = _step(e, route, ("alt", name), name, doms, rngs, f"{route} run {k} ({name})")
            if route == "auto_prune":
                assert st["search_form"] == (F.FORM_FOURIER if name == "noise256" else F.FORM_SEA_MFMA)
            else:
                assert st["search_form"] == F.FORM_SEA_MFMA


# ---- CPU: the two identities the pixel pass relies on ----------------------------------------------------------------

def _every_case(oracle):
    """(source, target, domains, ranges) of every case above."""
    for name in ("m64", "m70"):
        for nd in (1, 31, 32, 33, 127, 128, 129):
            yield _plane(name), _plane(name), _many_domains(name, nd), _lists(name)[1]
        yield _plane(name), _plane(name), _lists(name)[0], _many_ranges(name, 129)
    for name, odd in (("m70", False), ("m70", True), ("n70", True), ("mosaic264", False), ("mosaic264", True)):
        yield (_plane(name), _plane(name)) + _lists(name, odd)
    for o in (0, 1):
        yield _plane("m70"), _plane("m64b"), _grid(70, 58, 16, 8, o, o), _grid(64, 58, 8, 8, o, o)
    for name in ("fallback512", "const64", "mosaic256", "mosaic256b", "noise256"):
        yield (_plane(name), _plane(name)) + _lists(name)
    for name in T.CASES:
        src, tgt, _ = TR._frame(name)
        yield (src, tgt) + tuple(g.astype(F.GRID_ITEM) for g in TR._items(oracle, src, tgt, False))


def test_keys_are_the_sums(oracle):
    """No GPU.  The domain key, the sum of the 2×2 cell sums the pool row holds, is the domain's pixel sum (what the
    key was read from the plane as before) and fits 16 bits with every cell in the pool's u16; the range key 4Σr
    fits 16 bits.  The lists are the oracle's grids and classes where the cases use them."""
    for src, tgt, doms, rngs in _every_case(oracle):
        s = src.astype(np.int64)
        for d in doms:
            x, y = int(d["x"]), int(d["y"])
            box = s[y:y + 16, x:x + 16]
            cells = box[0::2, 0::2] + box[0::2, 1::2] + box[1::2, 0::2] + box[1::2, 1::2]
            assert cells.shape == (8, 8) and int(cells.max()) <= 1020  # a cell fits the pool's u16
            assert int(cells.sum()) == int(box.sum()) < (1 << 16)
        t = tgt.astype(np.int64)
        for r in rngs:
            x, y = int(r["x"]), int(r["y"])
            box = t[y:y + 8, x:x + 8]
            assert box.shape == (8, 8)
            assert 4 * int(box.sum()) == int((4 * box).sum()) < (1 << 16)
