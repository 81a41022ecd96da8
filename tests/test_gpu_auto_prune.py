"""FRAC_ENGINE_AUTO's pruned route (n = 8, T = 4, ratio 2): the tiled form's windows under the MFMA engine, the
exhaustive Fourier search in the same run when the windows hold more than kAutoPruneBudget of the block × tile
pairs, and the routing around it (FRAC_FLAG_PRUNE, FRAC_FLAG_EXHAUSTIVE, the minimum size).

Bar: every case's records are byte-identical to ENGINE_VALU's and bit-exact against the oracle, and engine,
search_form, matrix_flops and evaluated_mappings are asserted from auto_prune_frames.predict — the window rule
restated in numpy, so the route of every frame is known before it runs (test_auto_prune_frames.py).

Frames: 256×256 (961 domains: 31 tiles, the last of one row; 1,024 ranges) and 264×248 (960 domains in 30 full
tiles; 1,023 ranges: the last block is partial), the latter also with domains at stride 4 (3,721: a partial
last tile).  Value noise and the diagonal ramp cannot prune at this size (four groups: every window holds a
quarter of the tiles or more; predicted shares 0.59 – 0.71), so they are the cases of a share over the budget
that is not 1; the pruned cases run auto_prune_frames.mosaic.  The classifier has at most 7 buckets and
kTpMaxBuckets is 8, so no configuration exceeds it: that branch of the routing has no case here.
"""
import numpy as np
import pytest

import auto_prune_frames as A
import fractencode_amd as F
from golden_util import FIELDS
from test_gpu_parity import as_oracle_fields, run_engine

pytestmark = pytest.mark.gpu

FLOPS = 6 * 32768  # per block × tile pair: six MFMA 32×32×16 on both routes
PRUNE, EXH = F.FLAG_PRUNE, F.FLAG_EXHAUSTIVE

_frames = {
    "mosaic256": lambda: A.mosaic(256, 256),
    "mosaic_noisy264": lambda: A.mosaic(264, 248, amp=2),
    "noise256": lambda: A.noise(256, 256),
    "noise264": lambda: A.noise(264, 248),
    "value_noise256": lambda: __import__("fractencode_amd.synth", fromlist=["value_noise"]).value_noise(256, 256, 77),
    "ramp256": lambda: A.ramp(256, 256),
}
_cache = {}


def _meta(W, H, dstep=8, T=4, cls=False, thr=0.0):
    return dict(src=16 if dstep == 8 else (W, H, 16, 16, dstep, dstep), tgt=8, T=T, cls=cls, thr=thr, smax=-1.0)


def _reference(oracle, name, dstep=8, cls=False, thr=0.0):
    """(plane, meta, VALU records, VALU stats, oracle records, rejected), once per case."""
    key = (name, dstep, cls, thr)
    if key not in _cache:
        p = _frames[name]()
        H, W = p.shape
        meta = _meta(W, H, dstep, cls=cls, thr=thr)
        vout, vst = run_engine(p, meta, F.ENGINE_VALU)
        doms, rngs = oracle.uniform_grid(W, H, 16, dstep), oracle.uniform_grid(W, H, 8, 8)
        if cls:
            doms, rngs = oracle.classify(p, doms), oracle.classify(p, rngs)
        want, rej, _ = oracle.estimate(p, doms, rngs, T=4, thr=thr, use_classifier=cls, threads=16)
        _cache[key] = (p, meta, vout, vst, want, rej)
    return _cache[key]


def _predict(p, dstep=8, cls=False, thr=0.0, **kw):
    H, W = p.shape
    cats = {}
    if cls:
        cats = dict(rcat=F.preclassify(p, F.create_uniform_grid(W, H, 8, 8))["category"],
                    dcat=F.preclassify(p, F.create_uniform_grid(W, H, 16, dstep))["category"])
    return A.predict(p, dstep, hitH=F.hit_limit(thr, 8) if thr > 0 else -1, **cats, **kw)


def _check_route(st, pred, pruned, what):
    print(f"{what}: predicted share {pred['share']:.4f}, form {st['search_form']}, flops {st['matrix_flops']}, "
          f"evaluated {st['evaluated_mappings']} of {pred['eligible']}")
    assert st["engine"] == F.ENGINE_MFMA, what
    if pruned:
        assert st["search_form"] == F.FORM_SEA_MFMA, what
        assert st["matrix_flops"] == (pred["seed_pairs"] + pred["pairs"]) * FLOPS, what
        assert st["evaluated_mappings"] == pred["seed_evals"] + pred["evals"], what
    else:
        # seed plus exhaustive, nothing from the windows: no entry array was sized from them
        assert st["search_form"] == F.FORM_FOURIER, what
        assert st["matrix_flops"] == (pred["seed_pairs"] + pred["full"]) * FLOPS, what
        assert st["evaluated_mappings"] == pred["seed_evals"] + pred["eligible"], what


def _check_records(out, st, ref, what):
    _, _, vout, vst, want, rej = ref
    assert out.tobytes() == vout.tobytes(), what
    got = as_oracle_fields(out)
    for k in FIELDS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: field {k}")
    assert st["rejected_mappings"] == rej == vst["rejected_mappings"], what
    assert st["hit_ranges"] == vst["hit_ranges"] and st["fallback_ranges"] == vst["fallback_ranges"], what


# ---- 1, 2: the two routes; 3: the prediction that tells them apart ------------------------------------------

@pytest.mark.parametrize("name,dstep", [("mosaic256", 8), ("mosaic_noisy264", 8), ("mosaic_noisy264", 4)])
def test_pruning_frames_take_the_windows(oracle, name, dstep):
    ref = _reference(oracle, name, dstep)
    pred = _predict(ref[0], dstep)
    assert pred["share"] <= A.BUDGET / 4
    out, st = run_engine(ref[0], ref[1], F.ENGINE_AUTO, flags=PRUNE)
    _check_route(st, pred, True, f"{name} stride {dstep}")
    assert st["evaluated_mappings"] < pred["eligible"]
    _check_records(out, st, ref, f"{name} stride {dstep}")


@pytest.mark.parametrize("name,dstep", [("noise256", 8), ("noise264", 8), ("noise264", 4)])
def test_noise_falls_back_to_the_exhaustive_search(oracle, name, dstep):
    ref = _reference(oracle, name, dstep)
    pred = _predict(ref[0], dstep)
    assert pred["share"] == 1.0
    out, st = run_engine(ref[0], ref[1], F.ENGINE_AUTO, flags=PRUNE)
    _check_route(st, pred, False, f"{name} stride {dstep}")
    _check_records(out, st, ref, f"{name} stride {dstep}")


@pytest.mark.parametrize("name", ["value_noise256", "ramp256"])
def test_smooth_frames_of_this_size_fall_back(oracle, name):
    """Value noise and the ramp at 256×256: windows of 0.69 and 0.59 of the pairs, over the budget without being
    everything — the fallback after windows that did prune."""
    ref = _reference(oracle, name)
    pred = _predict(ref[0])
    assert 1.5 * A.BUDGET <= pred["share"] < 1.0
    out, st = run_engine(ref[0], ref[1], F.ENGINE_AUTO, flags=PRUNE)
    _check_route(st, pred, False, name)
    _check_records(out, st, ref, name)


def _valu_bound(p, rx, ry, dx, dy):
    """The seed bound from the VALU engine: each range's least S16 over the seed tile's domains."""
    item = lambda x, y, s: np.array([(a, b, s, s, -1) for a, b in zip(x, y)], dtype=F.GRID_ITEM)
    with F.Engine(0, 4, False, 0.0, -1.0, F.ENGINE_VALU) as e:
        e.set_frame(p)
        e.set_domains(item(dx, dy, 16))
        out, _ = e.search(item(rx, ry, 8))
    s16 = out["distance"] * 4096.0  # distance = (S16 / 16) / 256, exact below 2^24
    assert np.array_equal(s16, np.round(s16))
    return s16.astype(np.int64)


@pytest.mark.parametrize("name", ["mosaic256", "mosaic_noisy264", "noise264"])
def test_prediction_from_the_valu_engine_s_seed_bound(name):
    """The restated window rule with U from the VALU engine's minimum over each seed tile gives the share the
    numpy bound gives (so the CPU check of the frames stands for what the device computes)."""
    p = _frames[name]()
    a, b = A.predict(p), A.predict(p, bound=_valu_bound)
    assert (a["pairs"], a["full"], a["evals"], a["seed_evals"]) == (b["pairs"], b["full"], b["evals"], b["seed_evals"])
    assert b["share"] == 1.0 if name.startswith("noise") else b["share"] <= A.BUDGET / 4


# ---- 4: hits and the classifier -------------------------------------------------------------------------------

@pytest.mark.parametrize("cls,thr", [(False, 40.0), (True, 0.0), (True, 40.0)])
@pytest.mark.parametrize("name", ["mosaic256", "mosaic_noisy264", "noise264"])
def test_threshold_and_classifier(oracle, name, cls, thr):
    """rms threshold 40 (H = 163,840 widens every window to ±3,239) and the classifier (its buckets window
    separately).  The route follows from the prediction, which stays clear of the budget on either side: flat
    mosaic cells are all category −1 (one bucket, pruned), noisy ones scatter over seven buckets of a few tiles
    each (windows of nearly everything: the fallback)."""
    ref = _reference(oracle, name, cls=cls, thr=thr)
    pred = _predict(ref[0], cls=cls, thr=thr)
    assert pred["share"] <= A.BUDGET / 2 or pred["share"] >= 1.5 * A.BUDGET, pred["share"]
    out, st = run_engine(ref[0], ref[1], F.ENGINE_AUTO, flags=PRUNE)
    what = f"{name} cls={cls} thr={thr}"
    _check_route(st, pred, pred["share"] <= A.BUDGET, what)
    _check_records(out, st, ref, what)
    if thr > 0 and name.startswith("mosaic"):
        assert st["hit_ranges"] > 0


# ---- 6: one context, the route flipping between frames ---------------------------------------------------------

def _run_frame(e, p, nr):
    import torch

    buf = torch.full((nr * F.TUPLE.itemsize,), 0xAB, dtype=torch.uint8).pin_memory()
    e.set_frame(p)
    e.set_tuple_sink(buf.data_ptr())
    e.run()
    e.set_tuple_sink(None)
    out, st = e.fetch()
    torch.cuda.synchronize()
    return out.tobytes(), buf.numpy().tobytes(), st


@pytest.mark.parametrize("W,H", [(256, 256), (264, 248)])
def test_route_flips_across_frames_of_one_context(W, H):
    """Pruned → fallback → pruned on one context with the tuple sink (pinned) and a shard of 800 ranges (groups
    of 8, 8, 8 and 1 blocks): each run's records and sink equal a fresh context's and the VALU engine's."""
    frames = [A.mosaic(W, H), A.noise(W, H), A.mosaic(W, H, amp=3, noise_seed=99)]
    idx = A.mosaic_shard(W, H)
    rngs, doms = F.create_uniform_grid(W, H, 8, 8)[idx], F.create_uniform_grid(W, H, 16, 8)
    preds = [A.predict(p, ranges=idx) for p in frames]
    assert [pr["share"] <= A.BUDGET / 4 for pr in preds] == [True, False, True] and preds[1]["share"] == 1.0

    def engine(eng, flags=0):
        e = F.Engine(0, 4, False, 0.0, -1.0, eng, flags=flags)
        e.set_frame(frames[0])
        e.set_domains(doms)
        e.set_ranges(rngs)
        return e

    with engine(F.ENGINE_AUTO, PRUNE) as one:
        got = [_run_frame(one, p, len(rngs)) for p in frames]
    for k, (p, pr) in enumerate(zip(frames, preds)):
        with engine(F.ENGINE_AUTO, PRUNE) as fresh, engine(F.ENGINE_VALU) as valu:
            want, vwant = _run_frame(fresh, p, len(rngs)), _run_frame(valu, p, len(rngs))
        _check_route(got[k][2], pr, k != 1, f"frame {k}")
        assert got[k][0] == want[0] == vwant[0], f"frame {k}: records"
        assert got[k][1] == want[1] == vwant[1], f"frame {k}: tuple sink"
        assert got[k][2]["search_form"] == want[2]["search_form"]


# ---- 7, 8: the flags and the minimum size ----------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, EXH, EXH | PRUNE], ids=["none", "exhaustive", "exhaustive+prune"])
@pytest.mark.parametrize("name", ["mosaic256", "noise264"])
def test_small_frames_and_exhaustive_stay_on_the_fourier_search(oracle, name, flags):
    """Without FRAC_FLAG_PRUNE these sizes are below kAutoPruneMinPairs; FRAC_FLAG_EXHAUSTIVE wins over
    FRAC_FLAG_PRUNE.  The run is today's: no seed in its flops or its evaluated pairs."""
    ref = _reference(oracle, name)
    pred = _predict(ref[0])
    out, st = run_engine(ref[0], ref[1], F.ENGINE_AUTO, flags=flags)
    assert (st["engine"], st["search_form"]) == (F.ENGINE_MFMA, F.FORM_FOURIER)
    assert st["matrix_flops"] == pred["full"] * FLOPS and st["evaluated_mappings"] == pred["eligible"]
    _check_records(out, st, ref, f"{name} flags={flags}")


def test_explicit_engines_ignore_the_flags(oracle):
    ref = _reference(oracle, "mosaic256")
    for eng, form in ((F.ENGINE_MFMA, F.FORM_FOURIER), (F.ENGINE_SEA, F.FORM_SEA_MFMA), (F.ENGINE_VALU, F.FORM_DOT2)):
        out, st = run_engine(ref[0], ref[1], eng, flags=PRUNE)
        assert (st["engine"], st["search_form"]) == (eng, form)
        assert out.tobytes() == ref[2].tobytes()


# ---- 9: everything else under AUTO is where it was -------------------------------------------------------------

@pytest.mark.parametrize("src,tgt,T", [(16, 8, 8), (16, 4, 4), (8, 4, 4), (32, 16, 4)])
def test_other_geometries_keep_their_route(src, tgt, T):
    """T = 8, 16→4 and the other range sizes under AUTO with FRAC_FLAG_PRUNE: the form and the bytes of
    ENGINE_MFMA without it."""
    p = A.mosaic(256, 256, amp=2)
    meta = dict(src=src, tgt=tgt, T=T, cls=False, thr=0.0, smax=-1.0)
    want, wst = run_engine(p, meta, F.ENGINE_MFMA)
    out, st = run_engine(p, meta, F.ENGINE_AUTO, flags=PRUNE)
    assert (st["engine"], st["search_form"]) == (wst["engine"], wst["search_form"])
    assert st["search_form"] != F.FORM_SEA_MFMA
    assert (st["matrix_flops"], st["evaluated_mappings"]) == (wst["matrix_flops"], wst["evaluated_mappings"])
    assert out.tobytes() == want.tobytes()


def test_quadtree_keeps_its_route():
    p = A.mosaic(256, 256, amp=2)
    res = []
    for eng, flags in ((F.ENGINE_MFMA, 0), (F.ENGINE_AUTO, PRUNE)):
        with F.Engine(0, 4, False, 0.0, -1.0, eng, flags=flags) as e:
            e.set_frame(p)
            res.append(e.encode_quadtree(16, 4, 10.0))
    (a, sa), (b, sb) = res
    assert a.tobytes() == b.tobytes()
    assert (sa["search_form"], sa["matrix_flops"]) == (sb["search_form"], sb["matrix_flops"])
    assert sb["search_form"] != F.FORM_SEA_MFMA
