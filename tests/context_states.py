"""A catalogue of search configurations for walking one context from state to state (test_gpu_context_walk.py)
and the two helpers the walk needs.  Importable without a GPU: the states are built from seeded generators and
the oracle's grids; test_context_states.py checks their conditions by the oracle alone.

A state is a complete configuration: planes (one, or distinct source and target), domain list, range list and
parameters.  Most states differ from `base` in one respect, so a transition between two of them issues one setter
call and everything else the context prepared for the previous state has to be still right, or rebuilt.  States
that would give the base's records on the base's plane (another engine or form: the engines are exact) get a
plane of their own, so a stale record can never pass for a fresh one.

  apply(engine, prev, state)   issues only the setter calls for what differs between prev and state
  expected(oracle, state)      the oracle's records and reject count
"""
from __future__ import annotations

import functools
import hashlib
from dataclasses import dataclass, field

import numpy as np

import auto_prune_frames as APF

# fractencode_amd's constants, restated so the catalogue imports without the package's library
ENGINE_AUTO, ENGINE_VALU, ENGINE_MFMA, ENGINE_SEA = 0, 1, 2, 3
FLAG_DIRECT_FORM, FLAG_SEA_PER_RANGE, FLAG_PRUNE = 2, 4, 32
ITEM = np.dtype([("x", "<u4"), ("y", "<u4"), ("w", "<u4"), ("h", "<u4"), ("category", "<i4")])
PARAMS = ("transforms", "use_classifier", "rms_threshold", "s_max", "engine", "flags")


def _key(a) -> str:
    a = np.ascontiguousarray(a)
    return hashlib.sha256(repr((a.shape, a.dtype.str)).encode() + a.tobytes()).hexdigest()


@dataclass(frozen=True)
class State:
    name: str
    source: np.ndarray
    doms: np.ndarray
    rngs: np.ndarray
    target: np.ndarray | None = None  # None: one plane (set_frame)
    transforms: int = 4
    use_classifier: bool = False
    rms_threshold: float = 0.0
    s_max: float = -1.0
    engine: int = ENGINE_AUTO
    flags: int = 0
    planes_key: str = field(init=False, compare=False)
    doms_key: str = field(init=False, compare=False)
    rngs_key: str = field(init=False, compare=False)

    def __post_init__(self):
        for a in (self.source, self.doms, self.rngs) + (() if self.target is None else (self.target,)):
            a.setflags(write=False)  # shared among the tests that need them, and left unchanged
        put = lambda k, v: object.__setattr__(self, k, v)
        put("planes_key", _key(self.source) + ("" if self.target is None else _key(self.target)))
        put("doms_key", _key(self.doms))
        put("rngs_key", _key(self.rngs))

    @property
    def params(self) -> dict:
        return {k: getattr(self, k) for k in PARAMS}

    @property
    def geometry_key(self) -> str:
        """The range list without the categories: states that share it could pass each other's records."""
        return _key(np.stack([self.rngs[k] for k in ("x", "y", "w", "h")]))

    @property
    def frame_wh(self):
        p = self.source if self.target is None else self.target
        return p.shape[1], p.shape[0]

    @property
    def frc1(self) -> bool:
        """Whether pack_frc1 takes the state: one plane, square ranges on the row-major grid, domains on the
        (2n, n) lattice (include/fracenc.h), and at least one range."""
        if self.target is not None or not len(self.rngs) or not len(self.doms):
            return False
        n = int(self.rngs["w"][0])
        H, W = self.source.shape
        if int(self.rngs["h"][0]) != n or W < 2 * n or H < 2 * n:
            return False
        same = lambda a, b: len(a) == len(b) and all((a[k] == b[k]).all() for k in ("x", "y", "w", "h"))
        return same(self.rngs, grid(W, H, n, n)) and same(self.doms, grid(W, H, 2 * n, n))


def grid(W, H, size, offset) -> np.ndarray:
    """createUniformGrid (image/partition2.hpp:109-135) restated: row-major, x fastest, categories −1; size and
    offset an int or (x, y).  Empty when the item does not fit (as frac_uniform_grid)."""
    sw, sh = (size, size) if np.isscalar(size) else size
    ox, oy = (offset, offset) if np.isscalar(offset) else offset
    if W < sw or H < sh:
        return np.zeros(0, ITEM)
    ys, xs = np.meshgrid(np.arange(0, H - sh + 1, oy), np.arange(0, W - sw + 1, ox), indexing="ij")
    out = np.zeros(xs.size, ITEM)
    out["x"], out["y"], out["w"], out["h"], out["category"] = xs.reshape(-1), ys.reshape(-1), sw, sh, -1
    return out


def _plane(seed: int, W: int, H: int, kind: str) -> np.ndarray:
    from test_gpu_parity import _random_plane  # the parity tests' kinds: uniform, flat, noise (value noise)

    return np.ascontiguousarray(_random_plane(np.random.default_rng(seed), W, H, kind))


def fp32_frame(k: int, S: int) -> np.ndarray:
    """tools/fallback_probe.py's frame restated at a small size: value noise scaled into [0, 60] with k white 8×8
    ranges, each alone in a black 24×24 cell, so every candidate's error for them is in the fp32 regime
    (48 · (4 · 255 − 4 · 60)² > 2^24)."""
    from fractencode_amd.synth import value_noise

    p = (value_noise(S, S, 1234).astype(np.float64) * (60.0 / 255.0)).astype(np.uint8)
    cells = np.random.default_rng(17).choice((S // 24) ** 2, size=k, replace=False)
    for c in cells:
        y0, x0 = (c // (S // 24)) * 24, (c % (S // 24)) * 24
        y0, x0 = y0 - y0 % 8, x0 - x0 % 8
        p[y0:y0 + 24, x0:x0 + 24] = 0
        p[y0 + 8:y0 + 16, x0 + 8:x0 + 16] = 255
    return p


def _classified(plane, items):
    from oracle import oracle as O

    return O.classify(plane, items)


# the catalogue's names, in order (the GPU tests parametrise over them without building a state)
NAMES = ("base", "t8", "cls", "cls_empty", "thr40", "thr1e9", "smax05", "valu", "sea", "sea_per_range",
         "mfma_direct", "prune", "prune_fallback", "n4", "n2", "n16", "sampled_16to4", "generic_12to6", "rect_8x4",
         "distinct_planes", "frame_70x58", "frame_264x248", "fp32", "no_domains", "perm37", "dom_stride4",
         "multi_flat", "multi_n16", "multi_n4", "multi_sea")
# states whose run may leave work behind it that the next state's setters meet in flight: a deferred fp32
# fallback, the pruned route's plan, the largest buffers
ENQUEUE_ONLY = ("fp32", "prune", "prune_fallback", "frame_264x248")
# the pruned-route frames' size: the mosaic needs its four levels' groups of 256 ranges each (predicted shares at
# 128² and 192²: 1.0 and 0.61, over BUDGET / 2)
PRUNE_SIZE = (256, 256)


@functools.lru_cache(maxsize=None)
def catalogue() -> tuple:
    from fractencode_amd.synth import value_noise

    # the base plane: a corner of a 128² value-noise frame, smooth enough that about half its ranges meet a
    # threshold of 40 (64² value noise itself meets it nowhere)
    b = np.ascontiguousarray(value_noise(128, 128, 4100)[:64, :64])
    d16, r8 = grid(64, 64, 16, 8), grid(64, 64, 8, 8)
    S = []

    def add(name, source=b, doms=d16, rngs=r8, **kw):
        S.append(State(name, source, doms, rngs, **kw))

    add("base")
    add("t8", transforms=8)
    add("cls", use_classifier=True)
    # a category no domain has: the domains of the ranges' most frequent category leave the (preclassified) list
    cd, cr = _classified(b, d16), _classified(b, r8)
    cats, counts = np.unique(cr["category"][cr["category"] >= 0], return_counts=True)
    add("cls_empty", doms=cd[cd["category"] != cats[np.argmax(counts)]], rngs=cr, use_classifier=True)
    add("thr40", rms_threshold=40.0)
    add("thr1e9", rms_threshold=1e9)
    add("smax05", s_max=0.5)
    add("valu", source=_plane(4101, 64, 64, "uniform"), engine=ENGINE_VALU)
    add("sea", source=_plane(4102, 64, 64, "uniform"), engine=ENGINE_SEA)
    add("sea_per_range", source=_plane(4103, 64, 64, "noise"), engine=ENGINE_SEA, flags=FLAG_SEA_PER_RANGE)
    add("mfma_direct", source=_plane(4104, 64, 64, "uniform"), engine=ENGINE_MFMA, flags=FLAG_DIRECT_FORM)
    W, H = PRUNE_SIZE
    add("prune", source=APF.mosaic(W, H), doms=grid(W, H, 16, 8), rngs=grid(W, H, 8, 8), flags=FLAG_PRUNE)
    add("prune_fallback", source=APF.noise(W, H), doms=grid(W, H, 16, 8), rngs=grid(W, H, 8, 8), flags=FLAG_PRUNE)
    add("n4", doms=grid(64, 64, 8, 4), rngs=grid(64, 64, 4, 4))
    add("n2", doms=grid(64, 64, 4, 2), rngs=grid(64, 64, 2, 2))
    add("n16", doms=grid(64, 64, 32, 16), rngs=grid(64, 64, 16, 16))
    add("sampled_16to4", rngs=grid(64, 64, 4, 4))
    add("generic_12to6", doms=grid(64, 64, 12, 6), rngs=grid(64, 64, 6, 6))
    # rectangles: the domain grid cut so that every transform's samples stay inside the plane
    add("rect_8x4", doms=grid(64, 56, (16, 8), (8, 4)), rngs=grid(64, 64, (8, 4), (8, 4)))
    add("distinct_planes", source=_plane(4105, 96, 80, "noise"), target=_plane(4106, 48, 40, "uniform"),
        doms=grid(96, 80, 8, 4), rngs=grid(48, 40, 4, 4))
    add("frame_70x58", source=_plane(4107, 70, 58, "noise"), doms=grid(70, 58, 16, 8), rngs=grid(70, 58, 8, 8))
    add("frame_264x248", source=_plane(4108, 264, 248, "noise"), doms=grid(264, 248, 16, 8),
        rngs=grid(264, 248, 8, 8))
    add("fp32", source=fp32_frame(3, 96), doms=grid(96, 96, 16, 8), rngs=grid(96, 96, 8, 8))
    add("no_domains", doms=np.zeros(0, ITEM))
    add("perm37", rngs=r8[np.random.default_rng(4109).permutation(len(r8))[:37]])
    add("dom_stride4", doms=grid(64, 64, 16, 4))
    # several respects at once
    add("multi_flat", source=_plane(4110, 64, 64, "flat"), transforms=8, use_classifier=True, rms_threshold=2.5,
        s_max=0.7)
    add("multi_n16", source=_plane(4111, 128, 96, "uniform"), doms=grid(128, 96, 32, 16),
        rngs=grid(128, 96, 16, 16), transforms=8, use_classifier=True, rms_threshold=30.0)
    add("multi_n4", source=_plane(4112, 48, 32, "uniform"), doms=grid(48, 32, 8, 4), rngs=grid(48, 32, 4, 4),
        transforms=8, use_classifier=True, s_max=2.0, engine=ENGINE_VALU)
    add("multi_sea", source=_plane(4113, 98, 74, "uniform"), doms=grid(98, 74, 16, 8), rngs=grid(98, 74, 8, 8),
        use_classifier=True, engine=ENGINE_SEA)
    assert tuple(s.name for s in S) == NAMES
    return tuple(S)


def state(name: str) -> State:
    return catalogue()[NAMES.index(name)]


def apply(engine, prev: State | None, st: State) -> None:
    """The setter calls that take `engine` from prev to st, and no others: planes first (the lists are checked
    against them), then domains, ranges and the parameters that changed.  prev=None issues everything."""
    if prev is None or prev.planes_key != st.planes_key:
        if st.target is None:
            engine.set_frame(st.source)
        else:
            engine.set_planes(st.source, st.target)
    if prev is None or prev.doms_key != st.doms_key:
        engine.set_domains(st.doms)
    if prev is None or prev.rngs_key != st.rngs_key:
        engine.set_ranges(st.rngs)
    changed = {k: v for k, v in st.params.items() if prev is None or prev.params[k] != v}
    if changed:
        engine.set_params(**changed)


def expected(oracle, st: State):
    """(records, rejected mappings) of the state by the oracle (RESULT_DTYPE records in range order)."""
    rec, rej, done = oracle.estimate(st.source, st.doms, st.rngs, T=st.transforms, thr=st.rms_threshold,
                                     smax=st.s_max, use_classifier=st.use_classifier, tgt=st.target)
    assert done == len(st.rngs)
    return rec, rej
