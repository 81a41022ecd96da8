"""The tiled form's windowed search after DESIGN §7.10: the guarded fast epilogue (kTpFastSearch), the groups taken
longest window first (kTpLongestFirst) and no pool on the route (kTpSkipPool).  None of the three may change a record,
a window or a statistic, so every case compares records and tuples field for field with the oracle, and the
counters with tp_tie_frames.layout, on ENGINE_SEA and on AUTO | FRAC_FLAG_PRUNE.

Guard.  The fast epilogue runs for a (block, tile) pair iff R6·(2·D6) + Σb² ≤ 2^24 − 1, with R6 the greatest
Σ_o(|s_a + u_a| + |s_a − u_a|) over the block's ranges (a = r − 128, s and u the sums of an orbit's opposite
cells) and 2·D6, Σb² the greatest over the tile's domains (b = D4 − 512).  guard_pairs() evaluates that rule on the
host, from the frame and the layout alone, and the frames are checked with it without a GPU:
  mixed   512×384 value noise stretched to 0..255.  For a flat range and a flat domain both d levels from 128 the
          guard's left side is 3072·d², over the limit from d = 74: the windows of the darkest and the brightest
          groups straddle that level, so within one window some pairs pass and some do not.  Twelve groups, a share
          of 0.24: under AUTO's budget, so FRAC_FLAG_PRUNE stays on the windowed search.
  smooth  256², 128 ± 3: every pair passes.
  zeros   256², 0 with a few 1s: Σb² is 2^24 or just under, 2·D6 = 4096, every block's R6 is about 8,192: no pair
          passes.  (Both hold the whole bucket in every window: over the budget, so AUTO falls back on them and
          ENGINE_SEA is the route that runs the windowed search.)
  The 961 domains of a 256² frame make 31 tiles, the last with one valid row and 31 of padding (a tile of padding
  alone cannot exist: tiles are ⌈domains / 32⌉ per bucket); in each frame a window ends at the last tile with a
  partial last chunk, so the chunk's one load of four thresholds reads the array's padding.
Order.  The permutation itself is not visible through the API; what a wrong one breaks is: a group searched twice
and another not at all.  One group (200 ranges), four groups, 272 groups (more than tp_plan's 256 threads, two per
thread and the last threads idle; compared with the exhaustive route byte for byte, the oracle being too slow at
that size), all windows equal (a constant frame), the classifier's buckets, and frame A then frame B on one context
against a fresh context, so a skipped group cannot hide behind A's records.  (A window is never empty while its
bucket has a tile: the seed tile's best row always lies inside it.)
Pool.  A source near 0 and a target half near 0, half near 255: every range of the bright half has its least error
near 64·1020² > 2^24, so fallback_ranges > 0 on the windowed search (ENGINE_SEA: with no seed bound the windows hold
the whole bucket, which AUTO would count as over its budget), whose fp32 fallback now samples the plane.  The route's
fit is always fused (launch_tp), so there is no unfused variant to run.  The same context then runs FLAG_EXHAUSTIVE,
and the reverse.  test_gpu_tp_route covers the fp32 regime under AUTO | FRAC_FLAG_PRUNE within the budget (its
classifier case) and the over-budget fall into the exhaustive search."""
import numpy as np
import pytest

import auto_prune_frames as A
import fractencode_amd as F
import tp_tie_frames as T
from fractencode_amd import synth
from test_gpu_tp_records import FLOPS, SEA, _run, route_param, sink_param
from test_gpu_tp_records import _check as check_thr
from test_gpu_tp_records import _reference as reference_thr
from golden_util import FIELDS
from test_gpu_parity import as_oracle_fields
from test_gpu_tp_route import _check, _reference

gpu = pytest.mark.gpu
S = 256
FAST6_LIMIT = (1 << 24) - 1
_cache = {}


# ---- frames -----------------------------------------------------------------------------------------------------

MW, MH = 512, 384


def mixed():
    v = synth.value_noise(MW, MH, 5).astype(np.int64)
    return ((v - v.min()) * 255 // (v.max() - v.min())).astype(np.uint8)


def smooth():
    return (128 + np.random.default_rng(8).integers(-3, 4, (S, S))).astype(np.uint8)


def zeros():
    p = np.zeros((S, S), np.uint8)
    rng = np.random.default_rng(9)
    p[rng.integers(0, S, 60), rng.integers(0, S, 60)] = 1
    return p


def constant():
    return np.full((S, S), 77, np.uint8)


def halves():
    """(source, target): the source near 0 everywhere, the target's left half near 0 and its right half near 255, so
    every range of the right half has its least error near 64·1020² > 2^24: the fp32 regime."""
    rng = np.random.default_rng(10)
    src = rng.integers(0, 3, (S, S)).astype(np.uint8)
    tgt = rng.integers(0, 3, (S, S)).astype(np.uint8)
    tgt[:, S // 2:] = 255 - tgt[:, S // 2:]
    return src, tgt


FRAMES = {"mixed": mixed, "smooth": smooth, "zeros": zeros, "constant": constant}


# ---- the guard rule on the host ---------------------------------------------------------------------------------

def _orbit_terms(v):
    """(|orbit sums|, |alternating orbit sums|) of an 8×8 integer block, per cell (each orbit four times)."""
    r1, r2, r3 = np.rot90(v, 1), np.rot90(v, 2), np.rot90(v, 3)
    return np.abs(v + r1 + r2 + r3), np.abs(v - r1 + r2 - r3)


def guard_pairs(p, lay):
    """Per group: (pairs of its window that pass the guard, pairs that do not, whether its window ends at the last
    tile with a partial last chunk)."""
    H, W = p.shape
    rx, ry = T.grid(W, H, 8, 8)
    dx, dy = T.grid(W, H, 16, 8)
    ntiles = int(lay["dom_tile"].max()) + 1
    gx, gy = np.zeros(ntiles, np.int64), np.zeros(ntiles, np.int64)
    for k, (x, y) in enumerate(zip(dx, dy)):
        b = T._d4(p, x, y) - 512
        s, a = _orbit_terms(b)
        t = lay["dom_tile"][k]
        gx[t] = max(gx[t], 2 * max(int(s.max()), int(a.max())))
        gy[t] = max(gy[t], int((b * b).sum()))
    trmax = np.where(gy > FAST6_LIMIT, -1, np.where(gx == 0, np.iinfo(np.int32).max,
                                                   (FAST6_LIMIT - gy) // np.maximum(gx, 1)))
    out = []
    for _, t0, t1, nblk, rs, _ in lay["groups"]:
        ok = bad = 0
        for k in range(nblk):
            r6 = 0
            for r in rs[32 * k:32 * k + 32]:
                s, a = _orbit_terms(p[ry[r]:ry[r] + 8, rx[r]:rx[r] + 8].astype(np.int64) - 128)
                r6 = max(r6, (int(s.sum()) + int(a.sum())) // 4)
            passing = int((r6 <= trmax[t0:t1]).sum())
            ok += passing
            bad += (t1 - t0) - passing
        out.append((ok, bad, t1 == ntiles and (t1 - t0) % 4 != 0))
    return out


@pytest.mark.parametrize("name", ["mixed", "smooth", "zeros"])
def test_guard_frames_are_what_they_claim(name):
    p = FRAMES[name]()
    lay = T.layout(p, p)
    g = guard_pairs(p, lay)
    print(name, "share", round(lay["share"], 4), "groups (pass, fail, partial chunk at the padding):", g)
    if name == "mixed":
        assert lay["pairs"] <= A.BUDGET * lay["full"], "the frame must stay on the windowed route under AUTO"
        assert any(ok > 0 and bad > 0 for ok, bad, _ in g), "both kinds of pair in one window"
    elif name == "smooth":
        assert all(bad == 0 and ok > 0 for ok, bad, _ in g)
    else:
        assert all(ok == 0 and bad > 0 for ok, bad, _ in g)
    assert any(end for _, _, end in g), "a window ending at the last tile with a partial chunk"


# ---- guard ------------------------------------------------------------------------------------------------------

def _grids(oracle, p):
    H, W = p.shape
    return oracle.uniform_grid(W, H, 16, 8), oracle.uniform_grid(W, H, 8, 8)


@gpu
@route_param
@sink_param
@pytest.mark.parametrize("name", ["mixed", "smooth", "zeros", "constant"])
def test_guard_both_ways(oracle, name, route, sink):
    p = FRAMES[name]()
    doms, rngs = _grids(oracle, p)
    ref = _reference(oracle, ("fast", name), p, doms, rngs, False)
    with F.Engine(0, 4, False, 0.0, -1.0, route[0], flags=route[1]) as e:
        e.set_frame(p)
        e.set_domains(doms.astype(F.GRID_ITEM))
        e.set_ranges(rngs.astype(F.GRID_ITEM))
        out, st, tuples = _run(e, len(rngs), sink)
    _check(out, st, tuples, ref, route, f"{name} route={route} sink={sink}")
    if route is SEA or name == "mixed":
        assert st["search_form"] == F.FORM_SEA_MFMA


@gpu
@route_param
@sink_param
def test_guard_with_a_threshold(oracle, route, sink):
    """The HITS twin over the mixed frame, at a threshold some ranges meet and others do not."""
    p, thr = mixed(), 2.0
    doms, rngs = _grids(oracle, p)
    ref = reference_thr(oracle, ("fast-thr", thr), p, p, doms, rngs, False, thr)
    with F.Engine(0, 4, False, thr, -1.0, route[0], flags=route[1]) as e:
        e.set_frame(p)
        e.set_domains(doms.astype(F.GRID_ITEM))
        e.set_ranges(rngs.astype(F.GRID_ITEM))
        out, st, tuples = _run(e, len(rngs), sink)
    check_thr(out, st, tuples, ref, route, f"mixed thr={thr} route={route} sink={sink}")
    print("hit ranges", st["hit_ranges"], "of", len(rngs))
    assert 0 < st["hit_ranges"] < len(rngs)


# ---- order ------------------------------------------------------------------------------------------------------

@gpu
@route_param
def test_one_group(oracle, route):
    p = mixed()
    doms, rngs = _grids(oracle, p)
    # 200 ranges of neighbouring sums (seven blocks, one group): a narrow window, so AUTO stays on the windowed search
    sums = T._box(p, *T.grid(MW, MH, 8, 8), 8)
    sel = np.sort(np.argsort(sums, kind="stable")[1400:1600])
    sub = np.ascontiguousarray(rngs[sel])
    key = ("fast-one-group",)
    if key not in _cache:
        want, rej, _ = oracle.estimate(p, doms, sub, T=4, thr=0.0, use_classifier=False, threads=16)
        _cache[key] = (want, rej, T.layout(p, p, -1, ranges=sel))
    want, rej, lay = _cache[key]
    assert len(lay["groups"]) == 1 and lay["pairs"] <= A.BUDGET * lay["full"]
    with F.Engine(0, 4, False, 0.0, -1.0, route[0], flags=route[1]) as e:
        e.set_frame(p)
        e.set_domains(doms.astype(F.GRID_ITEM))
        e.set_ranges(sub.astype(F.GRID_ITEM))
        out, st, _ = _run(e, len(sub), None)
    got = as_oracle_fields(out)
    for k in FIELDS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"one group: field {k}")
    assert st["search_form"] == F.FORM_SEA_MFMA
    seed = route is not SEA
    assert st["evaluated_mappings"] == seed * lay["seed_evals"] + lay["evals"]


@gpu
@route_param
def test_classifier_buckets(oracle, route):
    p = mixed()
    doms, rngs = _grids(oracle, p)
    doms, rngs = oracle.classify(p, doms), oracle.classify(p, rngs)
    ref = _reference(oracle, ("fast", "mixed-cls"), p, doms, rngs, True)
    assert len(ref[3]["groups"]) > 4  # several buckets, their last groups short
    with F.Engine(0, 4, True, 0.0, -1.0, route[0], flags=route[1]) as e:
        e.set_frame(p)
        e.set_domains(doms.astype(F.GRID_ITEM))
        e.set_ranges(rngs.astype(F.GRID_ITEM))
        out, st, tuples = _run(e, len(rngs), None)
    _check(out, st, tuples, ref, route, f"mixed classifier route={route}", fallback=st["fallback_ranges"] > 0)


def _bytes(e, p):
    e.set_frame(p)
    e.run()
    out, st = e.fetch()
    return out.tobytes(), e.fetch_tuples().tobytes(), st["search_form"], st["matrix_flops"], st["evaluated_mappings"]


@gpu
def test_frame_a_then_frame_b_on_one_context():
    doms, rngs = F.create_uniform_grid(MW, MH, 16, 8), F.create_uniform_grid(MW, MH, 8, 8)

    def engine():
        e = F.Engine(0, 4, False, 0.0, -1.0, F.ENGINE_AUTO, flags=F.FLAG_PRUNE)
        e.set_frame(np.full((MH, MW), 77, np.uint8))
        e.set_domains(doms)
        e.set_ranges(rngs)
        return e

    with engine() as e:
        fresh = _bytes(e, mixed())
    with engine() as e:
        first = _bytes(e, A.mosaic(MW, MH))
        second = _bytes(e, mixed())
    assert first[2] == second[2] == F.FORM_SEA_MFMA
    assert second == fresh, "frame B after frame A differs from frame B on a fresh context"


@gpu
def test_more_groups_than_plan_threads():
    W, H = 2176, 2048
    p = synth.value_noise(W, H, 5)
    doms, rngs = F.create_uniform_grid(W, H, 16, 8), F.create_uniform_grid(W, H, 8, 8)
    assert (len(rngs) + 255) // 256 == 272  # groups of 8 blocks of 32: two per tp_plan thread, the last threads none
    res = {}
    for name, flags in (("pruned", F.FLAG_PRUNE), ("exhaustive", F.FLAG_EXHAUSTIVE)):
        with F.Engine(0, 4, False, 0.0, -1.0, F.ENGINE_AUTO, flags=flags) as e:
            e.set_frame(p)
            e.set_domains(doms)
            e.set_ranges(rngs)
            e.run()
            out, st = e.fetch()
            res[name] = (out.tobytes(), e.fetch_tuples().tobytes(), st["search_form"], st["fallback_ranges"])
    assert res["pruned"][2] == F.FORM_SEA_MFMA and res["exhaustive"][2] == F.FORM_FOURIER
    assert res["pruned"][:2] == res["exhaustive"][:2]
    assert res["pruned"][3] == res["exhaustive"][3]


# ---- pool -------------------------------------------------------------------------------------------------------

@gpu
@sink_param
def test_fp32_regime_without_a_pool(oracle, sink):
    src, tgt = halves()
    doms, rngs = _grids(oracle, src)
    want, rej, tup, lay = reference_thr(oracle, ("fast-halves",), src, tgt, doms, rngs, False, 0.0)
    with F.Engine(0, 4, False, 0.0, -1.0, F.ENGINE_SEA) as e:
        e.set_planes(src, tgt)
        e.set_domains(doms.astype(F.GRID_ITEM))
        e.set_ranges(rngs.astype(F.GRID_ITEM))
        out, st, tuples = _run(e, len(rngs), sink)
    got = as_oracle_fields(out)
    for k in FIELDS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"halves sink={sink}: field {k}")
    np.testing.assert_array_equal(tuples["domain"], tup["domain"])
    for k in ("transform", "contrast", "brightness", "distance"):
        np.testing.assert_array_equal(tuples[k], tup[k], err_msg=f"halves sink={sink}: tuple {k}")
    print("fallback ranges", st["fallback_ranges"], "of", len(rngs), "share", lay["share"])
    assert st["fallback_ranges"] >= len(rngs) // 4  # the bright half, at the least
    assert (st["engine"], st["search_form"]) == (F.ENGINE_SEA, F.FORM_SEA_MFMA)
    assert st["matrix_flops"] == lay["pairs"] * FLOPS and st["evaluated_mappings"] == lay["evals"]


@gpu
@pytest.mark.parametrize("order", ["pruned,exhaustive,pruned", "exhaustive,pruned,exhaustive"])
def test_fp32_regime_alternating_with_the_exhaustive_route(order):
    """One context, the route changed between runs (ENGINE_SEA: the windowed search; AUTO | FLAG_EXHAUSTIVE: the
    Fourier search), the planes changed with it: every run equals a fresh context's on that route.  The exhaustive run
    rebuilds the pool the pruned one no longer writes; the pruned one must not read the pool the exhaustive one left
    (the second pair of planes is the first turned by 180°, so its rows differ)."""
    doms, rngs = F.create_uniform_grid(S, S, 16, 8), F.create_uniform_grid(S, S, 8, 8)
    how = {"pruned": (F.ENGINE_SEA, 0), "exhaustive": (F.ENGINE_AUTO, F.FLAG_EXHAUSTIVE)}
    a = halves()
    b = tuple(np.ascontiguousarray(x[::-1, ::-1]) for x in a)
    planes = [a, b, a]

    def engine(name):
        e = F.Engine(0, 4, False, 0.0, -1.0, how[name][0], flags=how[name][1])
        e.set_frame(constant())
        e.set_domains(doms)
        e.set_ranges(rngs)
        return e

    def run(e, pl):
        e.set_planes(*pl)
        e.run()
        out, st = e.fetch()
        return out.tobytes(), e.fetch_tuples().tobytes(), st["search_form"], st["fallback_ranges"]

    names = order.split(",")
    with engine(names[0]) as one:
        for k, name in enumerate(names):
            with engine(name) as e:
                fresh = run(e, planes[k])
            one.set_params(engine=how[name][0], flags=how[name][1])
            got = run(one, planes[k])
            assert got[2] == (F.FORM_SEA_MFMA if name == "pruned" else F.FORM_FOURIER)
            assert got[3] > 0
            assert got == fresh, f"run {k} ({name}) differs from a fresh context's"
