"""The tiled form's search keeps, per range slot and row half, the window's maximum, the number of chunks attaining
it and the first two of them (search_dft CHUNKED, one record), and resolve_dft<true> evaluates the listed chunks,
or every chunk of the window when more attain it.  The cases are the ties that decide that: tp_tie_frames' planted
frames (two chunks tie; three tie: more than a record lists; two tie and a later chunk beats them; two hits in two
chunks; one exact match; three tie in a bucket that is not the last, with a decoy in the next bucket's tile: the
window's end, not the chunk's or the tile count, ends the walk — test_tp_tie_frames.py checks those properties on
the CPU) and sea_frames' levels, whose least error is attained by many domains over many chunks and whose windows
end before the last tile, with and without the classifier, with and without hits.

Every case: records and tuples field for field against the oracle, on ENGINE_SEA and on AUTO with FRAC_FLAG_PRUNE
(the route the restated window rule predicts; over the budget the fallback must have run), with no sink (the
slot-order walk) and with a pinned sink inside a guarded buffer (the range-order walk); evaluated_mappings and
matrix_flops from the model."""
import numpy as np
import pytest

import auto_prune_frames as A
import fractencode_amd as F
import sea_frames as SF
import tp_tie_frames as T
from golden_util import FIELDS
from test_gpu_parity import as_oracle_fields
from test_gpu_sink_stores import Sink

pytestmark = pytest.mark.gpu

FLOPS = 6 * 32768  # per block × tile pair: six MFMA 32×32×16
SEA, AUTO_PRUNE = (F.ENGINE_SEA, 0), (F.ENGINE_AUTO, F.FLAG_PRUNE)
route_param = pytest.mark.parametrize("route", [SEA, AUTO_PRUNE], ids=["sea", "auto_prune"])
sink_param = pytest.mark.parametrize("sink", [None, "pinned"], ids=["no_sink", "pinned_sink"])

_cache = {}


def _frame(name):
    """(src, tgt, thr or None) of a named frame."""
    if name in T.CASES:
        return T.case(name)
    src, tgt = SF.levels(SF.LEVELS_SEED) if name == "levels" else SF.close_levels(SF.CLOSE_LEVELS_SEED)
    return src, tgt, None


def _items(oracle, src, tgt, cls, sel=None):
    doms, rngs = oracle.uniform_grid(T.S, T.S, 16, 8), oracle.uniform_grid(T.S, T.S, 8, 8)
    if cls:
        doms, rngs = oracle.classify(src, doms), oracle.classify(tgt, rngs)
    return doms, (rngs if sel is None else np.ascontiguousarray(rngs[sel]))


def _reference(oracle, key, src, tgt, doms, rngs, cls, thr, sel=None):
    """(oracle records, rejected, oracle tuples, the model's layout), once per key."""
    if key not in _cache:
        want, rej, _ = oracle.estimate(src, doms, rngs, T=4, thr=thr, use_classifier=cls, tgt=tgt, threads=16)
        index = {(int(d["x"]), int(d["y"])): i for i, d in enumerate(doms)}
        tup = np.zeros(len(rngs), dtype=F.TUPLE)
        tup["domain"] = [index[(int(x), int(y))] if w else F.NO_DOMAIN
                         for x, y, w in zip(want["dx"], want["dy"], want["dw"])]
        tup["transform"], tup["contrast"], tup["brightness"], tup["distance"] = want["t"], want["s"], want["o"], want["dist"]
        cats = dict(rcat=rngs["category"], dcat=doms["category"]) if cls else {}
        idx = None if sel is None else np.arange(1024)[sel]
        lay = T.layout(src, tgt, F.hit_limit(thr, 8) if thr > 0 else -1, ranges=idx, **cats)
        _cache[key] = (want, rej, tup, lay)
    return _cache[key]


def _run(e, nr, sink):
    """One run of a prepared engine: (records, stats, tuples), the sink's bytes checked against fetch_tuples()."""
    if sink is None:
        e.run()
        got = None
    else:
        got = Sink(nr, sink, offset=8).run(e)
    out, st = e.fetch()
    tuples = e.fetch_tuples()
    if got is not None:
        assert got == tuples.tobytes(), "the sink's bytes differ from the fetched tuples"
    return out, st, tuples


def _check(out, st, tuples, ref, route, what):
    want, rej, tup, lay = ref
    got = as_oracle_fields(out)
    for k in FIELDS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: field {k}")
    np.testing.assert_array_equal(tuples["domain"], tup["domain"], err_msg=f"{what}: tuple domain")
    found = tup["domain"] != F.NO_DOMAIN
    for k in ("transform", "contrast", "brightness", "distance"):
        np.testing.assert_array_equal(tuples[k][found], tup[k][found], err_msg=f"{what}: tuple {k}")
    assert st["rejected_mappings"] == rej and st["fallback_ranges"] == 0, what
    pruned = lay["pairs"] <= A.BUDGET * lay["full"]
    print(f"{what}: share {lay['share']:.4f}, form {st['search_form']}, flops {st['matrix_flops']}, evaluated "
          f"{st['evaluated_mappings']} of {lay['eligible']}")
    if route is SEA:  # the windows alone: its seed is not in its counters
        assert (st["engine"], st["search_form"]) == (F.ENGINE_SEA, F.FORM_SEA_MFMA), what
        assert st["matrix_flops"] == lay["pairs"] * FLOPS, what
        assert st["evaluated_mappings"] == lay["evals"], what
    elif pruned:
        assert (st["engine"], st["search_form"]) == (F.ENGINE_MFMA, F.FORM_SEA_MFMA), what
        assert st["matrix_flops"] == (lay["seed_pairs"] + lay["pairs"]) * FLOPS, what
        assert st["evaluated_mappings"] == lay["seed_evals"] + lay["evals"], what
    else:  # over the budget: the seed, then the exhaustive search
        assert (st["engine"], st["search_form"]) == (F.ENGINE_MFMA, F.FORM_FOURIER), what
        assert st["matrix_flops"] == (lay["seed_pairs"] + lay["full"]) * FLOPS, what
        assert st["evaluated_mappings"] == lay["seed_evals"] + lay["eligible"], what


def _case(oracle, name, route, sink, cls=False, thr=None, sel=None, sel_key=None):
    src, tgt, cthr = _frame(name)
    thr = cthr if thr is None else thr
    doms, rngs = _items(oracle, src, tgt, cls, sel)
    ref = _reference(oracle, (name, cls, thr, sel_key), src, tgt, doms, rngs, cls, thr, sel)
    with F.Engine(0, 4, cls, thr, -1.0, route[0], flags=route[1]) as e:
        e.set_planes(src, tgt)
        e.set_domains(doms.astype(F.GRID_ITEM))
        e.set_ranges(rngs.astype(F.GRID_ITEM))
        out, st, tuples = _run(e, len(rngs), sink)
    _check(out, st, tuples, ref, route, f"{name} cls={cls} thr={thr} {sel_key} route={route} sink={sink}")
    return ref, st


# ---- 1: the planted ties -----------------------------------------------------------------------------------------

@sink_param
@route_param
@pytest.mark.parametrize("name", list(T.CASES))
def test_planted_ties(oracle, name, route, sink):
    if T.CASES[name][2] > 0:
        assert F.hit_limit(T.CASES[name][2], 8) == 16384
    (want, _, tup, lay), st = _case(oracle, name, route, sink)
    assert lay["share"] == 1.0  # every window is the whole bucket: AUTO falls back, ENGINE_SEA searches it all
    assert want["dw"][T.RANGE_INDEX] == 16 and (st["hit_ranges"] > 0) == (name in ("two_hits", "exact"))


# ---- 2: many-way ties, hits over many chunks, the classifier's buckets ----------------------------------------------

@sink_param
@route_param
@pytest.mark.parametrize("thr", [0.0, 1.5])
@pytest.mark.parametrize("cls", [False, True], ids=["plain", "classifier"])
@pytest.mark.parametrize("name", ["levels", "close_levels"])
def test_levels(oracle, name, cls, thr, route, sink):
    _case(oracle, name, route, sink, cls=cls, thr=thr)


# ---- 3: no stale record: a bucket of ranges without domains between two runs of "three" ---------------------------

def test_no_stale_record_is_read(oracle):
    """One context takes "three", then the same geometry with the upper half of the ranges in a category no domain
    has (those blocks have no group: their records are the first run's), then "three" again."""
    src, tgt, _ = T.case("three")
    doms, rngs = _items(oracle, src, tgt, False)
    doms["category"], rngs["category"] = 0, 0  # categories by hand: one bucket, as without the classifier
    split = rngs.copy()
    split["category"][:512] = 1
    refs = [_reference(oracle, ("three", True, 0.0, "one_bucket"), src, tgt, doms, rngs, True, 0.0),
            _reference(oracle, ("three", True, 0.0, "no_domains"), src, tgt, doms, split, True, 0.0)]
    assert int((refs[1][0]["dw"][:512] == 0).sum()) == 512 and int((refs[1][0]["dw"][512:] != 0).sum()) == 512
    assert refs[0][0].tobytes() == _reference(oracle, ("three", False, 0.0, None), src, tgt, doms, rngs, False,
                                              0.0)[0].tobytes()
    with F.Engine(0, 4, True, 0.0, -1.0, F.ENGINE_SEA) as e:
        e.set_planes(src, tgt)
        e.set_domains(doms.astype(F.GRID_ITEM))
        for k, (items, ref) in enumerate(((rngs, refs[0]), (split, refs[1]), (rngs, refs[0]))):
            e.set_ranges(items.astype(F.GRID_ITEM))
            for sink in (None, "pinned"):
                out, st, tuples = _run(e, len(items), sink)
                _check(out, st, tuples, ref, SEA, f"run {k} sink={sink}")
                assert st["empty_ranges"] == (512 if k == 1 else 0)


@sink_param
def test_overflow_walk_ends_at_the_window(oracle, sink):
    """tp_tie_frames.inner_bucket: three chunks attain the least error in a bucket that is not the last and whose
    window ends mid-chunk; a domain of the same error, first in domain order, waits in the next bucket's tile."""
    src, tgt, rcat, dcat = T.inner_bucket()
    doms, rngs = _items(oracle, src, tgt, False)
    doms["category"], rngs["category"] = dcat, rcat
    ref = _reference(oracle, ("inner_bucket", True, 0.0, None), src, tgt, doms, rngs, True, 0.0)
    d = T.grid(T.S, T.S, 16, 8)
    assert (ref[0]["dx"][T.RANGE_INDEX], ref[0]["dy"][T.RANGE_INDEX]) != (d[0][T.DECOY], d[1][T.DECOY])
    with F.Engine(0, 4, True, 0.0, -1.0, F.ENGINE_SEA) as e:
        e.set_planes(src, tgt)
        e.set_domains(doms.astype(F.GRID_ITEM))
        e.set_ranges(rngs.astype(F.GRID_ITEM))
        out, st, tuples = _run(e, len(rngs), sink)
    _check(out, st, tuples, ref, SEA, f"inner_bucket sink={sink}")


# ---- 4: a third of the ranges ----------------------------------------------------------------------------------------

@sink_param
@pytest.mark.parametrize("name", ["three", "levels"])
def test_a_third_of_the_ranges(oracle, name, sink):
    assert T.RANGE_INDEX % 3 == 0  # the shard keeps the constant range
    (want, _, _, lay), _ = _case(oracle, name, SEA, sink, thr=0.0, sel=slice(0, None, 3), sel_key="every_third")
    assert len(want) == 342 and sum(g[3] for g in lay["groups"]) == 11  # 8 + 3 blocks, the last partial
