"""The tiled form's fused launches (fracenc_tp.hip: tp_keys, tp_build, tp_prep, tp_seed_windows, tp_plan) where
the fusion itself can go wrong; the route's records, windows and routing are pinned by test_gpu_auto_prune.py,
test_gpu_sea.py, test_gpu_tuple_sink.py, test_gpu_frame_stream.py and test_gpu_fullsize.py.

1, 2  tp_plan walks its input in passes of 256 with a carry.  2048×2056 has 65,792 ranges in 2,056 blocks and
      257 groups of 8 (one group past a pass of groups, nine passes of blocks) and 65,280 domains in 2,040
      tiles; the shard has groups of unequal block counts and a range count that is no multiple of 256.  The
      oracle is too slow at this size: the records are compared with FRAC_FLAG_EXHAUSTIVE's, a route these
      launches are not part of and which the suites above pin against the oracle.  The counters come from
      auto_prune_frames.predict.
3     One context on a caller's stream, pruned and fallback frames alternating, the tuple sink on every other
      run, no host synchronisation but the library's own: a buffer left over from the previous run, or a
      missing reset, shows as a record that differs from the VALU engine's.
4     The best_key reset lives in tp_keys: ranges without a domain in their bucket, after a run that found
      winners for the same range indices, keep the default record.
"""
import ctypes as C

import numpy as np
import pytest

import auto_prune_frames as A
import fractencode_amd as F
from test_gpu_parity import run_engine

pytestmark = pytest.mark.gpu

FLOPS = 6 * 32768  # per block × tile pair: six MFMA 32×32×16
PRUNE, EXH = F.FLAG_PRUNE, F.FLAG_EXHAUSTIVE
W, H = 2048, 2056
META = dict(src=16, tgt=8, T=4, cls=False, thr=0.0, smax=-1.0)

_frames = {
    "mosaic": lambda: A.mosaic(W, H),
    "mosaic_noisy": lambda: A.mosaic(W, H, amp=2),
    "value_noise": lambda: __import__("fractencode_amd.synth", fromlist=["value_noise"]).value_noise(W, H, 77),
}
_cache = {}


def _case(name, shard):
    """(plane, range indices or None, prediction, FLAG_EXHAUSTIVE records and stats), once per case."""
    key = (name, shard)
    if key not in _cache:
        p = _frames[name]()
        idx = A.mosaic_shard(W, H) if shard else None
        pred = A.predict(p, ranges=idx)
        out, st = run_engine(p, META, F.ENGINE_AUTO, ranges_idx=idx, flags=EXH)
        assert st["search_form"] == F.FORM_FOURIER
        _cache[key] = (p, idx, pred, out, st)
    return _cache[key]


def _check_pruned(st, pred, engine, what):
    """_check_route of test_gpu_auto_prune.py for a pruned run; ENGINE_SEA runs the same launches unbudgeted and
    counts the windows alone (its seed is not in its counters)."""
    print(f"{what}: predicted share {pred['share']:.4f}, form {st['search_form']}, flops {st['matrix_flops']}, "
          f"evaluated {st['evaluated_mappings']} of {pred['eligible']}")
    assert st["search_form"] == F.FORM_SEA_MFMA, what
    if engine == F.ENGINE_AUTO:
        assert st["engine"] == F.ENGINE_MFMA, what
        assert st["matrix_flops"] == (pred["seed_pairs"] + pred["pairs"]) * FLOPS, what
        assert st["evaluated_mappings"] == pred["seed_evals"] + pred["evals"], what
    else:
        assert st["engine"] == F.ENGINE_SEA, what
        assert st["matrix_flops"] == pred["pairs"] * FLOPS, what
        assert st["evaluated_mappings"] == pred["evals"], what


def _run_case(name, shard, engine):
    p, idx, pred, want, wst = _case(name, shard)
    assert pred["share"] <= A.BUDGET / 4
    out, st = run_engine(p, META, engine, ranges_idx=idx, flags=PRUNE if engine == F.ENGINE_AUTO else 0)
    what = f"{name} shard={shard} engine={engine}"
    _check_pruned(st, pred, engine, what)
    assert out.tobytes() == want.tobytes(), what
    for k in ("rejected_mappings", "hit_ranges", "fallback_ranges"):
        assert st[k] == wst[k], (what, k)
    return pred


engine_param = pytest.mark.parametrize("engine", [F.ENGINE_AUTO, F.ENGINE_SEA], ids=["auto_prune", "sea"])


# ---- 1: more than one pass in tp_plan ---------------------------------------------------------------------------

@engine_param
@pytest.mark.parametrize("name", list(_frames))
def test_plan_carries_across_passes(name, engine):
    nr, nd = (W // 8) * (H // 8), (W // 8 - 1) * (H // 8 - 1)
    assert (nr, (nr + 31) // 32, nd, (nd + 31) // 32) == (65792, 2056, 65280, 2040)
    pred = _run_case(name, False, engine)
    assert len(pred["groups"]) == 257  # one past a pass
    if name.startswith("mosaic"):
        assert (pred["pairs"], pred["full"], pred["seed_pairs"]) == (52720, 4194240, 2056)
        assert (pred["evals"], pred["seed_evals"]) == (53985280, 2105344)


# ---- 2: a shard ------------------------------------------------------------------------------------------------

@engine_param
def test_shard_with_unequal_groups(engine):
    pred = _run_case("mosaic", True, engine)
    sizes = [len(r) for r, _ in pred["groups"]]
    assert sum(sizes) % 256 != 0 and len({(s + 31) // 32 for s in sizes}) > 1


# ---- 3: one context, frames alternating ------------------------------------------------------------------------

def _valu(p, doms, rngs):
    with F.Engine(0, 4, False, 0.0, -1.0, F.ENGINE_VALU) as e:
        e.set_frame(p)
        e.set_domains(doms)
        out, _ = e.search(rngs)
        return out.tobytes(), e.fetch_tuples().tobytes()


@pytest.mark.parametrize("streamed", [False, True], ids=["set_frame", "set_frame_async"])
def test_alternating_frames_on_one_context(streamed):
    import torch

    frames = {"m": A.mosaic(256, 256), "n": A.noise(256, 256)}
    doms, rngs = F.create_uniform_grid(256, 256, 16, 8), F.create_uniform_grid(256, 256, 8, 8)
    preds = {k: A.predict(p) for k, p in frames.items()}
    assert preds["m"]["share"] <= A.BUDGET / 4 and preds["n"]["share"] == 1.0
    want = {k: _valu(p, doms, rngs) for k, p in frames.items()}
    hosts = {k: torch.from_numpy(p.copy()).pin_memory() for k, p in frames.items()}
    stream = torch.cuda.Stream("cuda:0")
    with F.Engine(0, 4, False, 0.0, -1.0, F.ENGINE_AUTO, timing=True, flags=PRUNE) as e:
        e.set_stream(stream.cuda_stream)
        e.set_frame(frames["m"])
        e.set_domains(doms)
        e.set_ranges(rngs)
        for run, k in enumerate("mnmmnm"):
            what = f"run {run} ({k})"
            if streamed:
                e.set_frame_async(hosts[k])
            else:
                e.set_frame(frames[k])
            st = F.FracStats()
            if run % 2:  # the tuples through the sink, the counters alone from the fetch
                sink = torch.full((len(rngs) * F.TUPLE.itemsize,), 0xAB, dtype=torch.uint8).pin_memory()
                e.set_tuple_sink(sink.data_ptr())
                e.run()
                e.set_tuple_sink(None)
                e._check(F.lib().frac_fetch(e._ctx, None, C.byref(st)))
                assert sink.numpy().tobytes() == want[k][1], what
                st = st.as_dict()
            else:
                e.run()
                out, st = e.fetch()
                assert out.tobytes() == want[k][0], what
            pr = preds[k]
            assert st["engine"] == F.ENGINE_MFMA, what
            if k == "m":
                _check_pruned(st, pr, F.ENGINE_AUTO, what)
            else:
                assert st["search_form"] == F.FORM_FOURIER, what
                assert st["matrix_flops"] == (pr["seed_pairs"] + pr["full"]) * FLOPS, what
                assert st["evaluated_mappings"] == pr["seed_evals"] + pr["eligible"], what
        assert len(e.timing_history()) == 6
    torch.cuda.synchronize()


# ---- 4: resets with nothing to search ---------------------------------------------------------------------------

def _classified(p):
    doms = F.preclassify(p, F.create_uniform_grid(256, 256, 16, 8))
    rngs = F.preclassify(p, F.create_uniform_grid(256, 256, 8, 8))
    return doms, rngs


def _fresh(engine, flags, p, doms, rngs):
    with F.Engine(0, 4, True, 0.0, -1.0, engine, flags=flags) as e:
        e.set_frame(p)
        e.set_domains(doms)
        return e.search(rngs)


@pytest.mark.parametrize("engine,flags,every", [(F.ENGINE_AUTO, PRUNE, False), (F.ENGINE_SEA, 0, False),
                                                (F.ENGINE_SEA, 0, True)],
                         ids=["auto_prune-some", "sea-some", "sea-every"])
def test_ranges_without_domains_after_a_run_with_winners(engine, flags, every):
    """The classifier on; after a run in which every range found a winner, the domains of the first range's
    category go (some: the other buckets still search; every: the ranges are that category's alone, so no
    group is left and the run ends after its preparation).  Those ranges' records are the default ones: those
    of a fresh context and of the VALU engine."""
    from fractencode_amd.synth import value_noise

    p = value_noise(256, 256, 77)
    doms, rngs = _classified(p)
    cat = rngs["category"][0]
    if every:
        rngs = rngs[rngs["category"] == cat]
    assert (doms["category"] == cat).any()
    fewer = doms[doms["category"] != cat]
    gone = rngs["category"] == cat
    assert len(fewer) and gone.any() and gone.all() == every
    want, wst = _fresh(F.ENGINE_VALU, 0, p, fewer, rngs)
    assert wst["empty_ranges"] == int(gone.sum())
    with F.Engine(0, 4, True, 0.0, -1.0, engine, flags=flags) as e:
        e.set_frame(p)
        e.set_domains(doms)
        first, st1 = e.search(rngs)
        assert (first["sw"][gone] != 0).all()
        e.set_domains(fewer)
        e.run()
        out, st = e.fetch()
    fresh, fst = _fresh(engine, flags, p, fewer, rngs)
    assert out.tobytes() == fresh.tobytes() == want.tobytes()
    assert (out["sw"][gone] == 0).all()
    for k in ("empty_ranges", "rejected_mappings", "hit_ranges", "fallback_ranges"):
        assert st[k] == fst[k] == wst[k], k
    if not every:
        assert st["search_form"] == fst["search_form"]
