"""The context-walk catalogue (context_states.py) checked without a GPU: `apply` issues exactly the difference
between two states, and the states are what the walk needs them to be, by the oracle and the window predictor
alone — conditions on the inputs, so no state can be excused on the GPU."""
import itertools

import numpy as np
import pytest

import auto_prune_frames as APF
import context_states as CS


class Recorder:
    """An engine that only records the setter calls made on it."""

    def __init__(self):
        self.calls = []

    def set_frame(self, plane):
        self.calls.append(("set_frame", CS._key(plane)))

    def set_planes(self, source, target):
        self.calls.append(("set_planes", CS._key(source) + CS._key(target)))

    def set_domains(self, items):
        self.calls.append(("set_domains", CS._key(items)))

    def set_ranges(self, items):
        self.calls.append(("set_ranges", CS._key(items)))

    def set_params(self, **kw):
        self.calls.append(("set_params", kw))


def _calls(prev, st):
    r = Recorder()
    CS.apply(r, prev, st)
    return r.calls


@pytest.fixture(scope="module")
def results(oracle):
    """Every state's oracle result, computed once."""
    return {s.name: CS.expected(oracle, s) for s in CS.catalogue()}


def test_names_and_sizes():
    cat = CS.catalogue()
    assert tuple(s.name for s in cat) == CS.NAMES and len(set(CS.NAMES)) == len(CS.NAMES)
    assert set(CS.ENQUEUE_ONLY) <= set(CS.NAMES)
    for s in cat:
        for p in (s.source,) + (() if s.target is None else (s.target,)):
            assert p.dtype == np.uint8 and p.shape[1] <= 264 and p.shape[0] <= 256, s.name
    assert CS.state("frame_264x248").source.shape == (248, 264) and CS.state("frame_70x58").source.shape == (58, 70)


def test_apply_from_nothing_issues_everything():
    for s in CS.catalogue():
        calls = _calls(None, s)
        plane_call = ("set_frame", s.planes_key) if s.target is None else ("set_planes", s.planes_key)
        assert calls == [plane_call, ("set_domains", s.doms_key), ("set_ranges", s.rngs_key),
                         ("set_params", s.params)], s.name


def test_apply_issues_exactly_the_difference():
    st = CS.state
    base = st("base")
    assert _calls(base, base) == []
    # one respect each: a parameter goes through set_params alone, with that parameter alone
    assert _calls(base, st("t8")) == [("set_params", {"transforms": 8})]
    assert _calls(st("t8"), base) == [("set_params", {"transforms": 4})]
    assert _calls(base, st("cls")) == [("set_params", {"use_classifier": True})]
    assert _calls(base, st("thr40")) == [("set_params", {"rms_threshold": 40.0})]
    assert _calls(st("thr40"), st("thr1e9")) == [("set_params", {"rms_threshold": 1e9})]
    assert _calls(base, st("smax05")) == [("set_params", {"s_max": 0.5})]
    assert _calls(st("smax05"), st("t8")) == [("set_params", {"transforms": 8, "s_max": -1.0})]
    # a list alone
    assert _calls(base, st("no_domains")) == [("set_domains", st("no_domains").doms_key)]
    assert _calls(base, st("dom_stride4")) == [("set_domains", st("dom_stride4").doms_key)]
    assert _calls(base, st("perm37")) == [("set_ranges", st("perm37").rngs_key)]
    assert _calls(base, st("sampled_16to4")) == [("set_ranges", st("sampled_16to4").rngs_key)]
    assert [c[0] for c in _calls(base, st("n4"))] == ["set_domains", "set_ranges"]
    assert [c[0] for c in _calls(st("n4"), st("sampled_16to4"))] == ["set_domains"]
    assert [c[0] for c in _calls(base, st("cls_empty"))] == ["set_domains", "set_ranges", "set_params"]
    # a plane and the engine that searches it; planes of another size bring their lists
    assert _calls(base, st("valu")) == [("set_frame", st("valu").planes_key), ("set_params", {"engine": CS.ENGINE_VALU})]
    assert _calls(st("sea"), st("sea_per_range")) == [("set_frame", st("sea_per_range").planes_key),
                                                      ("set_params", {"flags": CS.FLAG_SEA_PER_RANGE})]
    assert _calls(st("prune"), st("prune_fallback")) == [("set_frame", st("prune_fallback").planes_key)]
    assert [c[0] for c in _calls(base, st("frame_70x58"))] == ["set_frame", "set_domains", "set_ranges"]
    assert [c[0] for c in _calls(base, st("distinct_planes"))] == ["set_planes", "set_domains", "set_ranges"]
    assert [c[0] for c in _calls(st("distinct_planes"), base)] == ["set_frame", "set_domains", "set_ranges"]
    # every pair: a call is issued exactly when its part differs, with the new state's value
    for a, b in itertools.permutations(CS.catalogue(), 2):
        got = dict(_calls(a, b))
        assert ("set_frame" in got or "set_planes" in got) == (a.planes_key != b.planes_key), (a.name, b.name)
        assert ("set_planes" in got) == (a.planes_key != b.planes_key and b.target is not None)
        assert got.get("set_domains", b.doms_key) == b.doms_key and ("set_domains" in got) == (a.doms_key != b.doms_key)
        assert got.get("set_ranges", b.rngs_key) == b.rngs_key and ("set_ranges" in got) == (a.rngs_key != b.rngs_key)
        assert got.get("set_params", {}) == {k: v for k, v in b.params.items() if a.params[k] != v}, (a.name, b.name)


def test_states_sharing_a_range_list_have_different_records(results):
    """A stale record must not pass for a fresh one: no two states with the same ranges give the same bytes."""
    for a, b in itertools.combinations(CS.catalogue(), 2):
        if a.geometry_key == b.geometry_key:
            assert results[a.name][0].tobytes() != results[b.name][0].tobytes(), (a.name, b.name)


def test_threshold_state_has_hits_and_misses(results):
    rec, _ = results["thr40"]
    hits = int((rec["dist"] <= 40.0).sum())
    assert 0 < hits < len(rec), hits
    assert (results["thr1e9"][0]["dist"] <= 1e9).all()


def test_empty_bucket_state_has_domainless_ranges(results):
    s = CS.state("cls_empty")
    rec, rej = results["cls_empty"]
    none = ~np.isin(s.rngs["category"], s.doms["category"])
    assert 0 < none.sum() < len(rec)  # (a block without a strict order keeps −1, as preclassify leaves it)
    np.testing.assert_array_equal(rec["dw"] == 0, none)
    assert rej >= int(none.sum()) * len(s.doms)
    assert (results["no_domains"][0]["dw"] == 0).all()


def test_fp32_state_has_fp32_regime_ranges(results):
    """The white ranges' least error over every candidate is at or above 2^24 in S16 = 16 · 256 · distance."""
    rec, _ = results["fp32"]
    fp32 = rec["dist"] * 16.0 * 256.0 >= float(1 << 24)
    assert 0 < fp32.sum() <= 3 and (rec["dw"] == 16).all()


def test_pruned_route_states_meet_the_predictor():
    W, H = CS.PRUNE_SIZE
    a, b = CS.state("prune"), CS.state("prune_fallback")
    assert a.source.shape == b.source.shape == (H, W)
    assert APF.predict(a.source)["share"] <= APF.BUDGET / 2
    assert APF.predict(b.source)["share"] == 1.0
    for s in (a, b):
        assert s.flags == CS.FLAG_PRUNE and s.engine == CS.ENGINE_AUTO and s.transforms == 4 and not s.use_classifier
        assert int(s.rngs["w"][0]) == 8 and int(s.doms["w"][0]) == 16


def test_catalogue_covers_the_paths():
    """What each state is there to move: its geometry and parameters, stated once."""
    st = CS.state
    assert [int(st(k).rngs["w"][0]) for k in ("n4", "n2", "n16", "sampled_16to4", "generic_12to6")] == [4, 2, 16, 4, 6]
    assert [int(st(k).doms["w"][0]) for k in ("n4", "n2", "n16", "sampled_16to4", "generic_12to6")] == [8, 4, 32, 16, 12]
    r = st("rect_8x4")
    assert (int(r.rngs["w"][0]), int(r.rngs["h"][0]), int(r.doms["w"][0]), int(r.doms["h"][0])) == (8, 4, 16, 8)
    d = st("distinct_planes")
    assert d.source.shape == (80, 96) and d.target.shape == (40, 48)
    assert len(st("perm37").rngs) == 37 and len(st("no_domains").doms) == 0
    assert len(st("dom_stride4").doms) == 13 * 13
    # odd frames: partial 32-range blocks and 32-domain tiles
    for k in ("frame_70x58", "frame_264x248", "perm37"):
        assert len(st(k).rngs) % 32 and (len(st(k).doms) % 32 or k == "frame_264x248")
    assert [s.name for s in CS.catalogue() if s.frc1] != []
