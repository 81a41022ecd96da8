"""The tiled form's route end to end on its own sort (fracenc_tpsort.hip, launch_tp).

(a) A frame larger than one sort chunk: 640×512 is the smallest frame with sides a multiple of 8 whose 5,120
    ranges and 79×63 = 4,977 domains both exceed two chunks of C = 2,048 without being a multiple of C, so each
    side sorts in three chunks, the last partial.  The frame is auto_prune_frames.mosaic, whose flat cells give
    many equal sums.  Without the classifier: one bucket, 16-bit keys, two passes.  With it the classifier's
    seven domain buckets make 19-bit keys (a third pass); mosaic's flat ranges are all category −1 and its
    smallest domain bucket holds 61, so the case moves items between categories by hand (as
    test_gpu_tp_records' stale-record case does): 20 domains stay in category 5 and 40 ranges join them (a
    bucket smaller than a tile, its last block partial), 300 ranges go to category 2.  Records and tuples field
    for field against the oracle, evaluated_mappings and matrix_flops from tp_tie_frames.layout, on ENGINE_SEA
    and on AUTO with FRAC_FLAG_PRUNE, without a sink and into a pinned one.
(b) Both outcomes of the budget test at 256×256 under AUTO | FRAC_FLAG_PRUNE: mosaic is predicted under the
    budget (the windowed search runs), i.i.d. noise over it (the exhaustive search runs instead).  Records,
    search_form and the counters; every phase time finite and ≥ 0, and ms_search > 0 on both routes (on the
    fallback it spans the exhaustive search).
(c) One context alternating the two frames, under → over → under and over → under → over, with a pinned sink in
    a guarded buffer and without: every run equals a fresh context's byte for byte.  A run that falls back leaves
    the previous run's records in place; a run that read them would differ here."""
import numpy as np
import pytest

import auto_prune_frames as A
import fractencode_amd as F
import tp_tie_frames as T
from golden_util import FIELDS
from test_gpu_parity import as_oracle_fields
from test_gpu_sink_stores import Sink
from test_gpu_tp_records import AUTO_PRUNE, FLOPS, SEA, _run

pytestmark = pytest.mark.gpu

C = F.TP_SORT_CHUNK
W, H = 640, 512
_cache = {}


def _tuples(want, doms):
    index = {(int(d["x"]), int(d["y"])): i for i, d in enumerate(doms)}
    tup = np.zeros(len(want), dtype=F.TUPLE)
    tup["domain"] = [index[(int(x), int(y))] if w else F.NO_DOMAIN for x, y, w in zip(want["dx"], want["dy"], want["dw"])]
    tup["transform"], tup["contrast"], tup["brightness"], tup["distance"] = want["t"], want["s"], want["o"], want["dist"]
    return tup


def _reference(oracle, key, p, doms, rngs, cls):
    """(oracle records, rejected, oracle tuples, the model's layout), once per key."""
    if key not in _cache:
        want, rej, _ = oracle.estimate(p, doms, rngs, T=4, thr=0.0, use_classifier=cls, threads=16)
        cats = dict(rcat=rngs["category"], dcat=doms["category"]) if cls else {}
        _cache[key] = (want, rej, _tuples(want, doms), T.layout(p, p, -1, **cats))
    return _cache[key]


def _check(out, st, tuples, ref, route, what, fallback=False):
    """Records and tuples field for field, the route and its counters from the model (test_gpu_tp_records' check;
    fallback: the case has ranges whose least error leaves the exact fp32 regime, settled by the fp32 fallback)."""
    want, rej, tup, lay = ref
    got = as_oracle_fields(out)
    for k in FIELDS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: field {k}")
    np.testing.assert_array_equal(tuples["domain"], tup["domain"], err_msg=f"{what}: tuple domain")
    found = tup["domain"] != F.NO_DOMAIN
    for k in ("transform", "contrast", "brightness", "distance"):
        np.testing.assert_array_equal(tuples[k][found], tup[k][found], err_msg=f"{what}: tuple {k}")
    print(f"{what}: share {lay['share']:.4f}, form {st['search_form']}, flops {st['matrix_flops']}, evaluated "
          f"{st['evaluated_mappings']} of {lay['eligible']}, fallback ranges {st['fallback_ranges']}")
    assert st["rejected_mappings"] == rej, what
    assert (st["fallback_ranges"] > 0) == fallback, what
    seed = route is not SEA  # AUTO counts its seed search; ENGINE_SEA the windows alone
    if route is SEA or lay["pairs"] <= A.BUDGET * lay["full"]:
        assert st["search_form"] == F.FORM_SEA_MFMA, what
        assert st["matrix_flops"] == (seed * lay["seed_pairs"] + lay["pairs"]) * FLOPS, what
        assert st["evaluated_mappings"] == seed * lay["seed_evals"] + lay["evals"], what
    else:  # over the budget: the seed, then the exhaustive search
        assert st["search_form"] == F.FORM_FOURIER, what
        assert st["matrix_flops"] == (lay["seed_pairs"] + lay["full"]) * FLOPS, what
        assert st["evaluated_mappings"] == lay["seed_evals"] + lay["eligible"], what
    assert st["engine"] == (F.ENGINE_SEA if route is SEA else F.ENGINE_MFMA), what


# ---- (a) more than one chunk per side ---------------------------------------------------------------------------

def _big_items(oracle, p, cls):
    doms, rngs = oracle.uniform_grid(W, H, 16, 8), oracle.uniform_grid(W, H, 8, 8)
    if cls:
        doms, rngs = oracle.classify(p, doms), oracle.classify(p, rngs)
        five = np.flatnonzero(doms["category"] == 5)
        assert len(five) > 20 and bool((rngs["category"] == -1).all())
        doms["category"][five[20:]] = 4
        rngs["category"][:40] = 5
        rngs["category"][40:340] = 2
    return doms, rngs


@pytest.mark.parametrize("route", [SEA, AUTO_PRUNE], ids=["sea", "auto_prune"])
@pytest.mark.parametrize("cls", [False, True], ids=["plain", "classifier"])
def test_frame_larger_than_one_chunk(oracle, cls, route):
    p = A.mosaic(W, H)
    doms, rngs = _big_items(oracle, p, cls)
    for n in (len(doms), len(rngs)):
        assert n > 2 * C and n % C != 0
    assert (len(rngs), len(doms)) == (5120, 79 * 63)
    if cls:
        dcount = np.bincount(doms["category"] + 1, minlength=7)
        rcount = np.bincount(rngs["category"] + 1, minlength=7)
        assert int((dcount > 0).sum()) > 4  # more than four buckets: 19-bit keys, a third pass
        assert dcount[6] == 20 and rcount[6] == 40  # a bucket smaller than a tile, with ranges
    ref = _reference(oracle, ("mosaic", W, H, cls), p, doms, rngs, cls)
    assert len(np.unique(T._box(p, *T.grid(W, H, 8, 8), 8))) <= 4  # many equal sums
    for sink in (None, "pinned"):
        with F.Engine(0, 4, cls, 0.0, -1.0, route[0], flags=route[1]) as e:
            e.set_frame(p)
            e.set_domains(doms.astype(F.GRID_ITEM))
            e.set_ranges(rngs.astype(F.GRID_ITEM))
            out, st, tuples = _run(e, len(rngs), sink)
        # the flat ranges moved to categories 2 and 5 meet only domains of four different levels: the least
        # error of many of them is 2^24 or more, so the case also takes the fp32 fallback after either search
        _check(out, st, tuples, ref, route, f"mosaic {W}x{H} cls={cls} route={route} sink={sink}", fallback=cls)


# ---- (b) both outcomes of the budget test -----------------------------------------------------------------------

_small = {"under": lambda: A.mosaic(256, 256), "over": lambda: A.noise(256, 256)}


def _small_reference(oracle, name):
    p = _small[name]()
    doms, rngs = oracle.uniform_grid(256, 256, 16, 8), oracle.uniform_grid(256, 256, 8, 8)
    return p, doms, rngs, _reference(oracle, (name, 256, 256, False), p, doms, rngs, False)


@pytest.mark.parametrize("name", ["under", "over"])
def test_both_outcomes_of_the_budget_test(oracle, name):
    p, doms, rngs, ref = _small_reference(oracle, name)
    lay = ref[3]
    if name == "under":
        assert lay["share"] <= A.BUDGET / 4
    else:
        assert lay["share"] == 1.0
    with F.Engine(0, 4, False, 0.0, -1.0, F.ENGINE_AUTO, timing=True, flags=F.FLAG_PRUNE) as e:
        e.set_frame(p)
        e.set_domains(doms.astype(F.GRID_ITEM))
        e.set_ranges(rngs.astype(F.GRID_ITEM))
        out, st, tuples = _run(e, len(rngs), None)
        hist = e.timing_history()
    _check(out, st, tuples, ref, AUTO_PRUNE, name)  # records, tuples, and the counters per the model
    assert st["search_form"] == (F.FORM_SEA_MFMA if name == "under" else F.FORM_FOURIER)
    assert len(hist) == 1
    for k in ("ms_prep", "ms_search", "ms_finish"):
        print(f"{name}: {k} = {hist[k][0]:.4f}")
        assert np.isfinite(hist[k][0]) and hist[k][0] >= 0, k
    assert hist["ms_search"][0] > 0


# ---- (c) one context, the route alternating ---------------------------------------------------------------------

def _one_run(e, p, nr, sink):
    e.set_frame(p)
    got = None
    if sink is None:
        e.run()
    else:
        got = Sink(nr, sink, offset=8).run(e)
    out, st = e.fetch()
    return out.tobytes(), e.fetch_tuples().tobytes(), got, st["search_form"], st["matrix_flops"], st["evaluated_mappings"]


@pytest.mark.parametrize("sink", [None, "pinned"], ids=["no_sink", "pinned_sink"])
@pytest.mark.parametrize("order", ["under,over,under", "over,under,over"])
def test_one_context_alternating_routes(order, sink):
    frames = {k: f() for k, f in _small.items()}
    doms, rngs = F.create_uniform_grid(256, 256, 16, 8), F.create_uniform_grid(256, 256, 8, 8)

    def engine():
        e = F.Engine(0, 4, False, 0.0, -1.0, F.ENGINE_AUTO, flags=F.FLAG_PRUNE)
        e.set_frame(frames["under"])
        e.set_domains(doms)
        e.set_ranges(rngs)
        return e

    fresh = {}
    for name, p in frames.items():
        with engine() as e:
            fresh[name] = _one_run(e, p, len(rngs), sink)
    assert fresh["under"][3] == F.FORM_SEA_MFMA and fresh["over"][3] == F.FORM_FOURIER
    with engine() as one:
        for k, name in enumerate(order.split(",")):
            got = _one_run(one, frames[name], len(rngs), sink)
            assert got == fresh[name], f"run {k} ({name}) differs from a fresh context's"
            if sink is not None:
                assert got[2] == got[1], f"run {k} ({name}): the sink's bytes differ from the fetched tuples"
