"""The sorted route's resolve works in groups of G consecutive items (resolve_dft_groups, fracenc_dft.hip: ranges when
the tuple sink is host memory, slots otherwise): the waves of a workgroup evaluate the items, one lane per item fits
it, and with a host sink the group's records and tuples leave as whole blocks whose pieces of a range that is not
written there (fp32 regime, past the end of a partial group) are skipped.  G comes from the library
(frac_debug_resolve_group).  Runs with a hit threshold may keep the one-wave-per-item kernels (kTpGrpHits); the cases
with hits pin whichever runs.

Every case runs on ENGINE_SEA and on AUTO | FLAG_PRUNE, on one context with no sink, a device sink and a pinned sink
at offsets 0 and 8 inside a 0xAB-guarded buffer in turn (Sink checks the guards), compares the records field for
field with ENGINE_VALU or the oracle and the sink's bytes with fetch_tuples().

  group edges    lists of 1, G − 1, G, G + 1, 2G + 3 and 1,021 ranges and every third range of a 256² mosaic;
  outcomes       fallback_probe.frame(6, 512) with the classifier: empty, fp32-regime and ordinary ranges interleaved
                 so that one group holds all three.  Two things differ from the plan this file was written to.  The
                 frame has no empty range under the classifier (every category has domains), so the domains of one
                 category are left out of the domain list: its ranges are empty.  And the fp32 regime S16 ≥ 2^24 is
                 distance ≥ 4,096 at n = 8 (distance = S16 / 4,096), not 16,384, which no range of an 8-bit frame
                 reaches (64 · 1020² / 4,096 = 16,256);
  ties, walks    every tp_tie_frames case, levels and close_levels with and without the classifier at thr 0 and 1.5
                 (two and three chunks attaining the maximum, the whole-window walk, hits), and "two_rows": two rows
                 of one tile and one row half attain the target, so two lanes hold a key and the 64-lane minimum
                 runs, not the one-lane shortcut (checked on the CPU by test_two_rows_of_one_tile_attain);
  reuse          device, pinned, device and no sink in turn, and two frames alternating into one sink.
"""
import numpy as np
import pytest

import fractencode_amd as F
import test_gpu_sink_stores as SS
import test_gpu_tp_records as TR
import tp_tie_frames as T
from test_gpu_sink_stores import Sink

gpu = pytest.mark.gpu

ROUTES = {"sea": TR.SEA, "auto_prune": TR.AUTO_PRUNE}
route_param = pytest.mark.parametrize("route", list(ROUTES))
SINKS = ((None, 0), ("device", 0), ("pinned", 0), ("pinned", 8))
TWO_ROWS = (2, ((124, None), (124, None)))  # seed, plants: two constant domains at one level, neighbours in ΣD4 order


def group() -> int:
    return int(F.lib().frac_debug_resolve_group())


def _runs(e, nr):
    """A prepared context through every sink in turn: [(what, records, stats, tuples)], the sink's bytes checked
    against fetch_tuples() and its guard bytes by Sink.run."""
    res = []
    for where, offset in SINKS:
        if where is None:
            e.run()
            got = None
        else:
            got = Sink(nr, where, offset).run(e)
        out, st = e.fetch()
        tuples = e.fetch_tuples()
        if got is not None:
            assert got == tuples.tobytes(), f"sink {where}+{offset}: its bytes differ from the fetched tuples"
        res.append((f"sink {where}+{offset}", out, st, tuples))
    return res


def _same_records(out, want, what):
    for k in F.ENCODE_ITEM.names:
        np.testing.assert_array_equal(out[k], want[k], err_msg=f"{what}: field {k}")
    assert out.tobytes() == want.tobytes(), what


# ---- 1: group edges ------------------------------------------------------------------------------------------------

def _edges():
    g = group()
    return {"one": slice(0, 1), "g_minus_1": slice(0, g - 1), "g": slice(0, g), "g_plus_1": slice(0, g + 1),
            "two_g_plus_3": slice(0, 2 * g + 3), "first1021": slice(0, 1021), "every_third": slice(0, None, 3)}


@gpu
@route_param
@pytest.mark.parametrize("edge", ["one", "g_minus_1", "g", "g_plus_1", "two_g_plus_3", "first1021", "every_third"])
def test_group_edges(edge, route):
    sel = _edges()[edge]
    p = SS._plane("mosaic256")
    doms, rngs = SS._grids(p, sel)
    assert len(rngs) == len(range(*sel.indices(1024)))
    want, wst = SS._reference("mosaic256", ("groups", edge, group()), sel)
    engine, flags = ROUTES[route]
    with F.Engine(0, 4, False, 0.0, -1.0, engine, flags=flags) as e:
        e.set_frame(p)
        e.set_domains(doms)
        e.set_ranges(rngs)
        for what, out, st, _ in _runs(e, len(rngs)):
            _same_records(out, want, f"{edge} {route} {what}")
            assert (st["hit_ranges"], st["fallback_ranges"]) == (wst["hit_ranges"], wst["fallback_ranges"]), what


# ---- 2: every outcome inside one group -----------------------------------------------------------------------------

_outcomes = {}
LEFT_OUT = 5  # the category whose domains are left out: its ranges have no eligible domain


def _outcome_case(oracle):
    """(plane, domains, the interleaved range list, its kinds, the ENGINE_VALU records and stats of that list)."""
    if not _outcomes:
        p = SS._plane("fallback512")
        doms = oracle.classify(p, oracle.uniform_grid(512, 512, 16, 8))
        rngs = oracle.classify(p, oracle.uniform_grid(512, 512, 8, 8))
        doms = np.ascontiguousarray(doms[doms["category"] != LEFT_OUT]).astype(F.GRID_ITEM)
        rngs = rngs.astype(F.GRID_ITEM)
        with F.Engine(0, 4, True, 0.0, -1.0, F.ENGINE_VALU) as e:
            e.set_frame(p)
            e.set_domains(doms)
            e.set_ranges(rngs)
            e.run()
            full, _ = e.fetch()
            tuples = e.fetch_tuples()
            # the three kinds, from this run alone
            empty = tuples["domain"] == F.NO_DOMAIN
            fp32 = ~empty & (full["distance"] * 4096.0 >= float(1 << 24))
            ordinary = ~empty & ~fp32
            ie, ifp, io = (np.flatnonzero(m) for m in (empty, fp32, ordinary))
            n = min(len(ie), len(ifp), len(io))
            assert n >= 1, (len(ie), len(ifp), len(io))
            g = group()
            order = np.stack([ie[:n], ifp[:n], io[:n]], 1).ravel()  # empty, fp32, ordinary, empty, …
            rest = np.stack([ie[n:n + g], io[n:n + g]], 1).ravel()   # then empty and ordinary alternate
            order = np.concatenate([order, rest])[:max(2 * g + 3, 3)]
            kinds = np.where(empty[order], 0, np.where(fp32[order], 1, 2))
            # one group of G consecutive list entries holds all three kinds: the first
            assert set(kinds[:g].tolist()) == {0, 1, 2}, kinds[:g]
            e.set_ranges(np.ascontiguousarray(rngs[order]))
            e.run()
            want, wst = e.fetch()
        assert want.tobytes() == full[order].tobytes()  # a range's record does not depend on the list
        _outcomes["case"] = (p, doms, np.ascontiguousarray(rngs[order]), kinds, want, wst)
    return _outcomes["case"]


@gpu
@route_param
def test_every_outcome_in_one_group(oracle, route):
    p, doms, rngs, kinds, want, wst = _outcome_case(oracle)
    assert wst["fallback_ranges"] == int((kinds == 1).sum()) and wst["empty_ranges"] == int((kinds == 0).sum())
    engine, flags = ROUTES[route]
    with F.Engine(0, 4, True, 0.0, -1.0, engine, flags=flags) as e:
        e.set_frame(p)
        e.set_domains(doms)
        e.set_ranges(rngs)
        for what, out, st, tuples in _runs(e, len(rngs)):
            _same_records(out, want, f"{route} {what}")
            assert (st["fallback_ranges"], st["empty_ranges"]) == (wst["fallback_ranges"], wst["empty_ranges"]), what
            np.testing.assert_array_equal(tuples["domain"] == F.NO_DOMAIN, kinds == 0, err_msg=what)


# ---- 3: ties and walks ---------------------------------------------------------------------------------------------

def _tie_frame(name):
    if name == "two_rows":
        return T.planted(*TWO_ROWS) + (0.0,)
    return TR._frame(name)


def test_two_rows_of_one_tile_attain(oracle):
    """CPU: in "two_rows" exactly two domains attain the constant range's least error, in one tile and one row half
    (two lanes of one evaluation hold a key), and the oracle picks the earlier of them at that error."""
    src, tgt, _ = _tie_frame("two_rows")
    lay = T.layout(src, tgt)
    least, rows, _ = T.attaining(src, tgt, lay)
    assert len(rows) == 2 and rows[0][0] != rows[1][0]
    assert rows[0][1:4] == rows[1][1:4]  # the same tile, chunk and row half
    assert lay["dom_row"][rows[0][0]] != lay["dom_row"][rows[1][0]]
    doms, rngs = oracle.uniform_grid(T.S, T.S, 16, 8), oracle.uniform_grid(T.S, T.S, 8, 8)
    want, _, _ = oracle.estimate(src, doms, rngs, T=4, thr=0.0, use_classifier=False, tgt=tgt, threads=16)
    first = min(rows[0][0], rows[1][0])
    assert want["dist"][T.RANGE_INDEX] * 4096.0 == least == 16384
    assert (want["dx"][T.RANGE_INDEX], want["dy"][T.RANGE_INDEX]) == (doms["x"][first], doms["y"][first])


TIES = [(name, False, None) for name in T.CASES] + [("two_rows", False, None)] + \
       [(name, cls, thr) for name in ("levels", "close_levels") for cls in (False, True) for thr in (0.0, 1.5)]


@gpu
@route_param
@pytest.mark.parametrize("name,cls,thr", TIES, ids=[f"{n}-{'cls' if c else 'plain'}-{t}" for n, c, t in TIES])
def test_ties_and_walks(oracle, name, cls, thr, route):
    src, tgt, cthr = _tie_frame(name)
    thr = cthr if thr is None else thr
    doms, rngs = TR._items(oracle, src, tgt, cls)
    ref = TR._reference(oracle, (name, cls, thr, None), src, tgt, doms, rngs, cls, thr)
    r = ROUTES[route]
    with F.Engine(0, 4, cls, thr, -1.0, r[0], flags=r[1]) as e:
        e.set_planes(src, tgt)
        e.set_domains(doms.astype(F.GRID_ITEM))
        e.set_ranges(rngs.astype(F.GRID_ITEM))
        for what, out, st, tuples in _runs(e, len(rngs)):
            TR._check(out, st, tuples, ref, r, f"{name} cls={cls} thr={thr} route={route} {what}")


# ---- 4: reuse ------------------------------------------------------------------------------------------------------

@gpu
@route_param
def test_sink_kinds_in_turn(route):
    name = "mosaic264"
    doms, rngs = SS._grids(SS._plane(name))
    want = SS._reference(name)[0]
    engine, flags = ROUTES[route]
    with F.Engine(0, 4, False, 0.0, -1.0, engine, flags=flags) as e:
        e.set_frame(SS._plane(name))
        e.set_domains(doms)
        e.set_ranges(rngs)
        seen = []
        for where in ("device", "pinned", "device", None):
            if where is None:
                e.run()
            else:
                got = Sink(len(rngs), where, offset=8).run(e)
            out, _ = e.fetch()
            tuples = e.fetch_tuples().tobytes()
            assert where is None or got == tuples
            _same_records(out, want, f"{route} {where}")
            seen.append(tuples)
    assert seen[0] == seen[1] == seen[2] == seen[3]


@gpu
@route_param
def test_two_frames_alternate_into_one_sink(route):
    names = ["mosaic256", "mosaic256b"]
    doms, rngs = SS._grids(SS._plane(names[0]))
    sink = Sink(len(rngs), "pinned")
    engine, flags = ROUTES[route]
    with F.Engine(0, 4, False, 0.0, -1.0, engine, flags=flags) as e:
        e.set_domains(doms)
        e.set_ranges(rngs)
        seen = []
        for k in range(4):
            e.set_frame(SS._plane(names[k & 1]))
            got = sink.run(e)
            out, _ = e.fetch()
            assert got == e.fetch_tuples().tobytes()
            _same_records(out, SS._reference(names[k & 1])[0], f"{route} frame {k}")
            seen.append(got)
    assert seen[0] == seen[2] and seen[1] == seen[3] and seen[0] != seen[1]
