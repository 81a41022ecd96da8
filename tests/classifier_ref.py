"""A plain reference of BrightnessBlocksClassifier2 and the case set of the key-kernel tests.

The reference is written from the reference sources alone (encode/Classifier2.cpp:8-62, image/partition2.hpp:13-31,
image/ImageStatistics.hpp:12-17), independently of the library and of the oracle: the four quadrants of an item are
size // 2 each (an odd last row or column belongs to none), their sums are int64 numpy sums, reduced mod 2^16 when
the quadrant is at most 16 wide (ImageStatistics2::sum adds those in uint16_t), and the category is the first of the
24 strict-order rules that holds, else −1.

The cases are shared by tests/test_classifier_ref.py, which pins the reference (and asserts what the case set has
to contain), and tests/test_gpu_bucket_keys.py, which runs every key kernel of fracenc_bucket.hip on them.  A case
is one call of the hook: a source and a target plane, a domain grid, a range grid and the path.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

ITEM = np.dtype([("x", "<u4"), ("y", "<u4"), ("w", "<u4"), ("h", "<u4"), ("category", "<i4")])

# encode/Classifier2.cpp:22-50, line by line: each rule is three strict comparisons (i, j): a_i > a_j, four
# rules per category.  The second rule of category 5 (a4 > a1, a1 > a3, a3 > a4) contradicts itself and never
# fires; it is kept as written.
RULES = (
    ((1, 2), (2, 3), (3, 4)), ((3, 1), (1, 4), (4, 2)), ((4, 3), (3, 2), (2, 1)), ((2, 4), (4, 1), (1, 3)),
    ((1, 3), (3, 2), (2, 4)), ((2, 1), (1, 4), (4, 3)), ((4, 2), (2, 3), (3, 1)), ((3, 4), (4, 1), (1, 2)),
    ((1, 4), (4, 3), (3, 2)), ((4, 1), (1, 2), (2, 3)), ((3, 2), (2, 4), (4, 1)), ((2, 3), (3, 1), (1, 4)),
    ((1, 2), (2, 4), (4, 3)), ((3, 1), (1, 2), (2, 4)), ((4, 3), (3, 1), (1, 2)), ((2, 4), (4, 3), (3, 1)),
    ((2, 1), (1, 3), (3, 4)), ((1, 3), (3, 4), (4, 2)), ((3, 4), (4, 2), (2, 1)), ((4, 2), (2, 1), (1, 3)),
    ((1, 4), (4, 2), (2, 3)), ((4, 1), (1, 3), (3, 4)), ((2, 3), (3, 4), (4, 1)), ((3, 2), (2, 1), (1, 4)),
)


def quadrant_sums(plane: np.ndarray, items: np.ndarray) -> np.ndarray:
    """[n, 4] int64: the exact sums of topLeft, topRight, bottomLeft, bottomRight of every item."""
    out = np.zeros((len(items), 4), np.int64)
    for i, it in enumerate(items):
        x, y, hw, hh = int(it["x"]), int(it["y"]), int(it["w"]) // 2, int(it["h"]) // 2
        assert x + int(it["w"]) <= plane.shape[1] and y + int(it["h"]) <= plane.shape[0], "item outside the plane"
        for q, (qx, qy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
            out[i, q] = plane[y + qy * hh: y + (qy + 1) * hh, x + qx * hw: x + (qx + 1) * hw].sum(dtype=np.int64)
    return out


def category_of_sums(sums: np.ndarray) -> np.ndarray:
    """The first rule that holds, four rules per category; −1 when none does."""
    a = {k + 1: sums[:, k] for k in range(4)}
    cat = np.full(len(sums), -1, np.int32)
    for r in reversed(range(len(RULES))):  # earlier rules overwrite later ones: the first that holds wins
        hold = np.ones(len(sums), bool)
        for i, j in RULES[r]:
            hold &= a[i] > a[j]
        cat[hold] = r // 4
    return cat


def categories(plane: np.ndarray, items: np.ndarray, wrap: bool = True) -> np.ndarray:
    """The categories of `items` on `plane`.  wrap=False: without the uint16_t arithmetic (what the classifier
    would give if ImageStatistics2::sum never wrapped) — only for measuring what the wrap changes."""
    sums = quadrant_sums(plane, items)
    if wrap:
        narrow = (items["w"] // 2) <= 16
        sums[narrow] %= 1 << 16
    return category_of_sums(sums)


def keys(plane: np.ndarray, items: np.ndarray) -> np.ndarray:
    """Bucket keys: category + 1, a stored category other than −1 passed through."""
    cat = categories(plane, items)
    stored = items["category"] != -1
    cat[stored] = items["category"][stored]
    return (cat + 1).astype(np.uint32)


def grid(W: int, H: int, size, offset, origin=(0, 0), count: int | None = None) -> np.ndarray:
    """Items of size (w, h) at origin + k·offset, row-major, while they fit a W × H plane; the first `count`."""
    w, h = (size, size) if np.isscalar(size) else size
    ox, oy = (offset, offset) if np.isscalar(offset) else offset
    xs = np.arange(origin[0], W - w + 1, ox)
    ys = np.arange(origin[1], H - h + 1, oy)
    out = np.zeros(len(xs) * len(ys), ITEM)
    if len(out):
        out["x"] = np.tile(xs, len(ys))
        out["y"] = np.repeat(ys, len(xs))
    out["w"], out["h"], out["category"] = w, h, -1
    if count is not None:
        assert len(out) >= count, "the grid is smaller than the count asked for"
        out = out[:count].copy()
    return out


# ---- planes (small, seeded) -----------------------------------------------------------------------------------

WRAP_PLANE = "noise5_160x192"  # np.random.default_rng(5).integers(0, 256, (192, 160)): the fixture's plane


@functools.lru_cache(maxsize=None)
def plane(name: str) -> np.ndarray:
    """kind + seed, then W x H: noise (0..255), bright (200..255), value (value noise), flat, two (constant 2×2
    blocks of two values), ocl ((11w + 43h + 124) mod 256, tests/OpenCLTest.cpp:67-75)."""
    kind, size = name.split("_")
    W, H = (int(v) for v in size.split("x"))
    seed = int("".join(c for c in kind if c.isdigit()) or 0)
    kind = kind.rstrip("0123456789")
    rng = np.random.default_rng(seed)
    if kind == "noise":
        p = rng.integers(0, 256, (H, W), dtype=np.uint8)
    elif kind == "bright":
        p = rng.integers(200, 256, (H, W), dtype=np.uint8)
    elif kind == "value":
        from fractencode_amd.synth import value_noise
        p = value_noise(W, H, seed)
    elif kind == "flat":
        p = np.full((H, W), 77, np.uint8)
    elif kind == "two":
        blocks = np.where(rng.integers(0, 2, ((H + 1) // 2, (W + 1) // 2)) == 0, 90, 131).astype(np.uint8)
        p = np.repeat(np.repeat(blocks, 2, 0), 2, 1)[:H, :W]
    elif kind == "ocl":
        hh, ww = np.mgrid[0:H, 0:W]
        p = ((ww * 11 + hh * 43 + 124) % 256).astype(np.uint8)
    else:
        raise KeyError(name)
    p = np.ascontiguousarray(p)
    p.setflags(write=False)
    return p


def plane_size(name: str):
    W, H = (int(v) for v in name.split("_")[1].split("x"))
    return W, H


# ---- cases ----------------------------------------------------------------------------------------------------

ROWS, PAIR, SUMS, AUTO = 1, 2, 3, 0  # the hook's paths (fractencode_amd.KEYS_*)


@dataclass(frozen=True)
class Case:
    name: str
    path: int
    src: str                      # plane name: the domains' plane
    doms: tuple                   # grid() arguments after W, H: (size, offset[, origin[, count]])
    rngs: tuple
    tgt: str | None = None        # the ranges' plane when it is another one
    tags: frozenset = field(default_factory=frozenset)

    def planes(self):
        s = plane(self.src)
        return s, (s if self.tgt is None else plane(self.tgt))

    def grids(self):
        return grid(*plane_size(self.src), *self.doms), grid(*plane_size(self.tgt or self.src), *self.rngs)


def _case(name, path, src, doms, rngs, tgt=None, tags=()):
    return Case(name, path, src, tuple(doms), tuple(rngs), tgt, frozenset(tags))


ROW_HEIGHTS = (2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64)
_ROW_PLANES = ("noise11_100x70", "bright12_100x70", "value13_100x70", "two14_100x70", "ocl_100x70", "noise15_100x70")


def lanes_of(h: int) -> int:
    """keys_rows_item's lanes per item: the height rounded up to a power of two (at least 2)."""
    L = 2
    while L < h:
        L *= 2
    return L


def _rows_cases():
    out = []
    for k, h in enumerate(ROW_HEIGHTS):
        L = lanes_of(h)
        per_wg = 256 // L
        pl = _ROW_PLANES[k % len(_ROW_PLANES)]
        oy = max(1, min(h // 2, 70 - h))
        # a: half width 4 (dword loads): every row pointer 4-aligned (domains: x a multiple of 4) and mixed
        #    (ranges: x = 1 + 3k); the domain count leaves the last workgroup partial
        out.append(_case(f"rows_h{h}_a", ROWS, pl, ((8, h), (4, oy), (0, 0), 2 * per_wg + 1 if h <= 32 else None),
                         ((8, h), (3, oy), (1, 0))))
        # b: half width 3 (bytes) and half width 12 at x = 2 + 5k (dwords where aligned); one range
        out.append(_case(f"rows_h{h}_b", ROWS, pl, ((6, h), (4, oy)), ((24, h), (5, oy), (2, 0), 1)))
    # the uint16_t wrap on the fixture's plane, and its u32 control (quadrants 17 wide)
    out.append(_case("rows_wrap_32x64", ROWS, WRAP_PLANE, ((32, 64), (16, 32)), ((34, 64), (16, 32)),
                     tags=("wrap_d", "control_r")))
    # one wave per item above 64 rows; 1, 3, 4, 5 items around the four items of a workgroup
    out.append(_case("wave_wrap_32x128", ROWS, WRAP_PLANE, ((32, 128), (8, 16)), ((16, 128), (8, 16)),
                     tags=("wrap_d", "wrap_r")))
    out.append(_case("wave_128x128_n1", ROWS, WRAP_PLANE, ((128, 128), (8, 16), (0, 0), 1),
                     ((16, 130), (8, 16), (3, 1), 3)))
    out.append(_case("wave_20x65_n4", ROWS, "value16_160x192", ((20, 65), (7, 9), (1, 0), 4),
                     ((32, 96), (8, 16), (0, 0), 5)))
    out.append(_case("wave_two_96", ROWS, "two17_160x192", ((24, 96), (6, 32)), ((40, 66), (10, 42))))
    return out


def _pair_cases():
    out = []
    # bucket_keys_rows2<2L, L>: L = 4, 8, 16; the domain count a whole number of workgroups (256 / 2L items each)
    # and not
    for L, pl in ((4, "noise21_100x70"), (8, "value22_100x70"), (16, "two23_130x70")):
        per_wg = 256 // (2 * L)
        out.append(_case(f"pair_{2 * L}to{L}_whole", PAIR, pl, (2 * L, L, (0, 0), per_wg), (L, L)))
        out.append(_case(f"pair_{2 * L}to{L}", PAIR, pl, (2 * L, L, (1, 0)), (L, L + 1, (1, 1))))
    out.append(_case("pair_64x16_32x8", PAIR, "noise24_130x70", ((64, 16), (8, 4)), ((32, 8), (32, 8))))
    out.append(_case("pair_64x32_32x16", PAIR, "bright25_130x70", ((64, 32), (32, 16)), ((32, 16), (16, 8))))
    out.append(_case("pair_64x32_32x16_whole", PAIR, "ocl_130x70", ((64, 32), (4, 4), (0, 0), 16),
                     ((32, 16), (7, 5))))
    # no paired launch: two launches of the row kernels
    out.append(_case("pair_4to2", PAIR, "noise26_37x29", (4, 2), (2, 2)))
    out.append(_case("pair_64to32", PAIR, "value27_130x70", (64, 2), (32, 3)))
    out.append(_case("pair_wrap_32x64_16x32", PAIR, WRAP_PLANE, ((32, 64), (16, 32)), ((16, 32), (16, 32)),
                     tags=("wrap_d",)))
    return out


SUMS_PLANES = ("noise31_37x29", "value32_33x65", "two33_100x36", "noise34_130x70")


def _sums_cases():
    out = []
    for pl in SUMS_PLANES:
        W, H = plane_size(pl)
        for q in (2, 4, 8, 16):
            if 2 * q > min(W, H):
                continue
            # domains: every q-aligned 2q square; ranges: 2q squares at stride q + 1, aligned and not
            out.append(_case(f"sums_{W}x{H}_q{q}", SUMS, pl, (2 * q, q), (2 * q, q + 1)))
        # off the lattice everywhere, and sizes without a pyramid level
        out.append(_case(f"sums_{W}x{H}_off", SUMS, pl, (8, 4, (1, 2)), (16, 8, (4, 3))))
        out.append(_case(f"sums_{W}x{H}_nolevel", SUMS, pl, (6, 3), (12, 5)))
        out.append(_case(f"sums_{W}x{H}_rect", SUMS, pl, (24, 7), ((8, 4), (4, 2))))
    out.append(_case("sums_odd_items", SUMS, "ocl_100x36", ((7, 5), (3, 2)), ((4, 8), (4, 4))))
    out.append(_case("sums_flat", SUMS, "flat_37x29", (8, 4), (4, 4)))
    # two planes: the domains' pyramid and the ranges' differ (in size too)
    out.append(_case("sums_two_planes_8to4", SUMS, "value35_130x70", (8, 4), (4, 4), tgt="noise36_100x36"))
    out.append(_case("sums_two_planes_32to16", SUMS, "noise37_100x36", (32, 16), (16, 16), tgt="bright38_130x70"))
    return out


def _auto_cases():
    return [
        _case("auto_16to8", AUTO, "noise41_100x36", (16, 8), (8, 8), tags=("as_sums",)),
        _case("auto_32to16_two_planes", AUTO, "value42_130x70", (32, 16), (16, 16), tgt="two43_100x36",
              tags=("as_sums",)),
        _case("auto_64x16_32x8", AUTO, "noise44_130x70", ((64, 16), (8, 4)), ((32, 8), (32, 8)), tags=("as_pair",)),
        _case("auto_wrap_32x64_16x32", AUTO, WRAP_PLANE, ((32, 64), (16, 32)), ((16, 32), (16, 32)),
              tags=("as_pair", "wrap_d")),
        _case("auto_128to64", AUTO, "value45_160x192", (128, 32), (64, 64), tags=("as_pair",)),
    ]


CASES = _rows_cases() + _pair_cases() + _sums_cases() + _auto_cases()
assert len({c.name for c in CASES}) == len(CASES)

# the reference-made fixture's grids (tests/golden/opencl_classify_rect.npz) on WRAP_PLANE: (w, h), (ox, oy)
RECT_GRIDS = (((32, 64), (16, 32)), ((32, 128), (8, 16)), ((16, 128), (8, 16)), ((34, 64), (16, 32)),
              ((30, 70), (7, 9)))
WRAP_GRIDS, CONTROL_GRID = RECT_GRIDS[:3], RECT_GRIDS[3]

# Engine.classify (classify_items): rectangular, wrapping, odd-sized and tied items
CLASSIFY_CASES = tuple((WRAP_PLANE, g) for g in RECT_GRIDS) + (
    ("ocl_100x36", ((7, 5), (3, 2))), ("two33_100x36", (4, 2)), ("two33_100x36", (8, 2)), ("flat_37x29", (6, 5)),
    ("value32_33x65", ((9, 33), (2, 3))), ("bright12_100x70", ((3, 2), (1, 1))),
)


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """(domain keys, range keys) of a case by the reference; computed once."""
    c = next(c for c in CASES if c.name == name)
    (s, t), (d, r) = c.planes(), c.grids()
    kd, kr = keys(s, d), keys(t, r)
    kd.setflags(write=False)
    kr.setflags(write=False)
    return kd, kr
