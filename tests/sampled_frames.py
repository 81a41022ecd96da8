"""Host-side cases and frames for the sampled form's tests (fracenc_gen.hip: every geometry other than
"domain = 2 × range, n ∈ {2, 4, 8, 16}").  test_sampled_frames.py checks their properties against the oracle
on the CPU, test_gpu_sampled_form.py runs the engines on them.  Plain numpy, fixed seeds; grids are built
here item by item (the layout of createUniformGrid, and of test_unaligned_origins for the offset ones), so
the same arrays serve the engine and the oracle.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

ITEM = np.dtype([("x", "<u4"), ("y", "<u4"), ("w", "<u4"), ("h", "<u4"), ("category", "<i4")])
FIELDS = ("x", "y", "dx", "dy", "dw", "dh", "t", "dist", "s", "o")
EXACT_LIMIT = 1 << 24  # S16 below this is exact in fp32 (kExactLimit): at or above it gen_fallback decides


def grid(W, H, size, step, x0=0, y0=0):
    """Items of `size` (w, h) every `step` (x, y) from (x0, y0) while they fit W×H, row by row."""
    (w, h), (sx, sy) = _pair(size), _pair(step)
    out = [(x, y, w, h, -1) for y in range(y0, H - h + 1, sy) for x in range(x0, W - w + 1, sx)]
    return np.array(out, dtype=ITEM)


def _pair(v):
    return (int(v), int(v)) if np.isscalar(v) else (int(v[0]), int(v[1]))


def cut(W, H, sw, sh):
    """The cut of tools/make_golden.py's cut(): the area of the domain grid within which every rotation of an
    sw×sh domain samples inside the W×H plane (a rotation reaches max(sw, sh) from the origin on both axes).
    (Its second step, down to a multiple of the item size and offset, serves createUniformGrid's assertion
    in the reference; grid() lays items out while they fit.)"""
    M = max(sw, sh)
    return W - (M - sw), H - (M - sh)


def regime(rec, area):
    """(found, fp32) masks of oracle records: found = a domain was eligible, fp32 = the winner's error
    S16 = 16·F is at least 2^24.  F is the reference's fp32 sum: distance = (double)F / area, so rounding
    distance·area to fp32 gives F back (the FP64 quotient is off by 2^-53 relative, F has 24 bits)."""
    found = rec["dw"] != 0
    F = (rec["dist"] * float(area)).astype(np.float32).astype(np.float64)
    return found, found & (F * 16.0 >= EXACT_LIMIT)


# --- A. chunked and large generic ranges -----------------------------------------------------------------

def two_regime(W, H, seed, div):
    """Value noise whose left half is squeezed to v // div + 100 (low contrast: winners with S16 < 2^24, the
    exact regime) and whose right half keeps the full contrast (winners in the fp32 regime)."""
    from fractencode_amd.synth import value_noise
    v = value_noise(W, H, seed)
    p = v // div + 100
    p[:, W // 2:] = v[:, W // 2:]
    return np.ascontiguousarray(p.astype(np.uint8))


# range (w, h), plane (W, H), div, domain stride (None: the range size), oracle's (exact, fp32) found
# ranges at T = 4 without the classifier, pool rows at T = 4
Chunked = namedtuple("Chunked", "name rng plane div dstride mix rows")
CHUNK_SEED = 5
CHUNKED = [
    Chunked("65x65", (65, 65), (390, 325), 8, None, (15, 15), 80),       # two chunks, odd tail; 80 rows
    Chunked("96x48", (96, 48), (576, 384), 8, None, (25, 23), 100),      # chunk border in mid-row
    Chunked("128x128", (128, 128), (768, 512), 8, None, (12, 12), 60),   # four chunks; gen_fallback's last LDS size
    Chunked("130x127", (130, 127), (780, 508), 8, None, (12, 12), 40),   # first size read from the plane
    Chunked("256x256", (256, 256), (1024, 1024), 16, (128, 128), (8, 8), 100),  # kGenMaxN: 16 chunks
    Chunked("33x31", (33, 31), (264, 186), 8, None, (43, 5), 112),       # odd pixel count, one chunk
]
CHUNK_MODES = [(4, False), (8, True)]  # (T, classifier)
THR_CASE = "65x65"


def chunked_case(c: Chunked):
    """(plane, domains, ranges) of a chunked case: domains 2 × the range, the grid's area cut as the
    rectangular goldens' is."""
    (rw, rh), (W, H) = c.rng, c.plane
    p = two_regime(W, H, CHUNK_SEED, c.div)
    sw, sh = 2 * rw, 2 * rh
    ox, oy = c.dstride or (rw, rh)
    dW, dH = cut(W, H, sw, sh)
    return p, grid(dW, dH, (sw, sh), (ox, oy)), grid(W, H, (rw, rh), (rw, rh))


def chunked_threshold(rec, area):
    """A hit threshold inside the exact regime of the oracle's thr = 0 records `rec`: midway between the
    fifth and the sixth of their distinct exact-regime distances."""
    found, fp32 = regime(rec, area)
    d = np.unique(rec["dist"][found & ~fp32])
    return float((d[4] + d[5]) / 2)


TAIL_LEVELS = tuple(20 + 10 * d for d in range(9))  # the corner level of domain d
TAIL_DELTAS = (-3, 2, 4, -1)


def tail_case(seed=21):
    """(source, target, domains, ranges, expected domain per range): 65×65 ranges whose LAST pixel alone decides
    the winner — pixel 4224, the single pixel of gen_search's final pair in its second chunk.

    Source (390²): nine disjoint 130×130 domains (stride 130), each a 65×65 uniform-noise block `base`
    magnified by 2 (so every 2×2 sample sum is 4·base), except domain d's bottom-right 2×2 block, which
    holds TAIL_LEVELS[d].  Target: 36 ranges, each `base` itself with its last pixel set to a level plus a
    small δ.  Under Id a range differs from domain d in that one sample only: S16 = 16·(v − level_d)², least
    for the level v was made from, in the exact regime and without ties (|δ| < 5); every other transform
    compares noise with noise.  An engine that drops, repeats or misplaces the last pixel picks another
    domain."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (65, 65), dtype=np.uint8)
    src = np.zeros((390, 390), np.uint8)
    doms = grid(390, 390, 130, 130)
    for d, it in enumerate(doms):
        x, y = int(it["x"]), int(it["y"])
        src[y:y + 130, x:x + 130] = base.repeat(2, 0).repeat(2, 1)
        src[y + 128:y + 130, x + 128:x + 130] = TAIL_LEVELS[d]
    tgt = np.zeros((390, 390), np.uint8)
    rngs = grid(390, 390, 65, 65)
    expect = np.zeros(len(rngs), np.int64)
    for r, it in enumerate(rngs):
        x, y = int(it["x"]), int(it["y"])
        tgt[y:y + 65, x:x + 65] = base
        expect[r] = (5 * r + 2) % 9
        tgt[y + 64, x + 64] = TAIL_LEVELS[expect[r]] + TAIL_DELTAS[r % 4]
    return src, tgt, doms, rngs, expect


# --- B. templated sizes in the sampled form --------------------------------------------------------------

# (n, S, plane side); domains S at stride max(1, S // 2), ranges n at stride n.  The metric points x·⌊S/n⌋ and
# the fit points (x·S)/n differ at (8, 9), (8, 20), (16, 17) and (16, 40); at n = 2 they coincide (x ∈ {0, 1})
TEMPLATED = [(2, 3, 24), (2, 5, 30), (2, 6, 24), (2, 8, 32), (8, 9, 72), (8, 20, 80),
             (16, 17, 96), (16, 40, 160), (16, 48, 192)]
# mode: (T, classifier, threshold, plane kind); thr "flat" is FLAT_THR[(n, S)]
MODES = {
    "t8_uniform": (8, False, 0.0, "uniform"),
    "t4_cls_noise": (4, True, 0.0, "noise"),
    "t4_thr_flat": (4, False, "flat", "flat"),
    "t4_thr0_flat": (4, False, 0.0, "flat"),      # H = 0: only exact copies hit
    "t8_all_fallback": (8, False, 1e9, "uniform"),  # every candidate hits: gen_fallback alone
}
# thresholds on the flat plane with hits and misses among the oracle's records (test_sampled_frames.py)
FLAT_THR = {(2, 3): 5.0, (2, 5): 5.0, (2, 6): 10.0, (2, 8): 60.0, (8, 9): 200.0, (8, 20): 300.0,
            (16, 17): 480.0, (16, 40): 500.0, (16, 48): 330.0}
# On the flat plane every 2×2 range is constant and a 3×3 domain, or the 4×4 pixels a 5×5 domain is sampled
# from, fits into one 4×4 cell of each level: every range has an exact copy and no threshold leaves a miss.
# These geometries take their hits and misses from the flat plane with a few pixels raised (SPECKLED).
SPECKLED = {(2, 3), (2, 5)}


def plane_of(kind, W, H, seed):
    """test_gpu_parity._random_plane's kinds ("flat" cropped to W×H when a side is no multiple of 4)."""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    if kind in ("flat", "speckled"):
        cells = rng.integers(0, 3, ((H + 3) // 4, (W + 3) // 4), dtype=np.uint8) * 60
        p = np.ascontiguousarray(cells.repeat(4, 0).repeat(4, 1)[:H, :W])
        if kind == "speckled":  # one pixel in sixteen raised by 1 … 30: near copies (small errors) and misses
            mask = rng.random((H, W)) < 1.0 / 16.0
            p[mask] += rng.integers(1, 31, int(mask.sum()), dtype=np.uint8)
        return p
    from fractencode_amd.synth import value_noise
    return value_noise(W, H, int(rng.integers(1 << 30)))


def templated_case(n, S, side, mode):
    """(plane, domains, ranges, T, classifier, thr) of a templated geometry in a mode."""
    T, cls, thr, kind = MODES[mode]
    if thr == "flat":
        thr = FLAT_THR[(n, S)]
        if (n, S) in SPECKLED:
            kind = "speckled"
    seed = 7000 + 100 * n + S
    p = plane_of(kind, side, side, seed)
    assert p.shape == (side, side)
    return p, grid(side, side, S, max(1, S // 2)), grid(side, side, n, n), T, cls, thr


# --- C. off the grid -------------------------------------------------------------------------------------

# name, S, n, source plane (W, H), target plane (W, H), domain step, range step, ranges kept
OffGrid = namedtuple("OffGrid", "name S n src tgt dstep rstep keep")
OFFGRID = [
    OffGrid("16to4", 16, 4, (96, 80), (72, 56), 9, 7, 50),
    OffGrid("10to3", 10, 3, (70, 62), (54, 46), 7, 5, 60),
    OffGrid("130to65", 130, 65, (420, 400), (300, 280), 67, 69, 11),
]


def offgrid_case(c: OffGrid):
    """(source, target, domains, ranges): two planes of different widths, domains from (3, 5) and ranges from
    (1, 2) with odd steps (test_unaligned_origins' grids), the ranges permuted and cut to c.keep."""
    rng = np.random.default_rng(900 + c.S)
    if c.n >= 32:  # both regimes at large sizes
        src = two_regime(c.src[0], c.src[1], 11, 8)
        tgt = two_regime(c.tgt[0], c.tgt[1], 12, 8)
    else:
        src = rng.integers(0, 256, (c.src[1], c.src[0]), dtype=np.uint8)
        tgt = rng.integers(0, 256, (c.tgt[1], c.tgt[0]), dtype=np.uint8)
    doms = grid(c.src[0], c.src[1], c.S, c.dstep, 3, 5)
    rngs = grid(c.tgt[0], c.tgt[1], c.n, c.rstep, 1, 2)
    assert len(rngs) > c.keep
    rngs = rngs[rng.permutation(len(rngs))[:c.keep]]
    return src, tgt, doms, rngs


# --- D. fp32-regime ties ---------------------------------------------------------------------------------

TIE_SIDE = 192
TIE_KINDS = ("blocks8", "binary")
TIE_GEOMETRIES = ((48, 24), (64, 32))  # domain, range; domains at stride = the range size


def tie_plane(kind):
    """test_gpu_parity._extreme_plane's 0/255 frames "blocks8" and "binary", 192²."""
    import zlib
    rng = np.random.default_rng(zlib.crc32(("sampled" + kind).encode()))
    S = TIE_SIDE
    if kind == "binary":
        return (rng.integers(0, 2, (S, S)) * 255).astype(np.uint8)
    return np.ascontiguousarray((rng.integers(0, 2, (S // 8, S // 8)) * 255).astype(np.uint8).repeat(8, 0).repeat(8, 1))


def tie_case(kind, S, n):
    p = tie_plane(kind)
    return p, grid(TIE_SIDE, TIE_SIDE, S, n), grid(TIE_SIDE, TIE_SIDE, n, n)


# image/transform.h:32-41
_KMAP = ((1, 0, 0, 0, 0, 1, 0, 0), (0, 1, 0, 0, -1, 0, 1, 0), (-1, 0, 1, 0, 0, -1, 0, 1), (0, -1, 0, 1, 1, 0, 0, 0),
         (1, 0, 0, 0, 0, -1, 0, 1), (0, 1, 0, 0, 1, 0, 0, 0), (-1, 0, 1, 0, 0, 1, 0, 0), (0, -1, 0, 1, -1, 0, 1, 0))


def fp32_candidate_errors(src, tgt, doms, rngs, T):
    """F[range, domain, t]: a plain numpy float32 replay of RootMeanSquare's different-size branch
    (image/metrics.h:42-48) for every candidate — the 2×2 sample sum M under transform t at
    (x·⌊Sw/nw⌋, y·⌊Sh/nh⌋) with the sampler's edge clamp, val = r − M/4 and the fp32 sum of val² over the range's
    pixels in row-major order (np.cumsum in float32 adds one element at a time)."""
    s = src.astype(np.int64)
    nw, nh = int(rngs["w"][0]), int(rngs["h"][0])
    Sw, Sh = int(doms["w"][0]), int(doms["h"][0])
    yy, xx = np.mgrid[0:nh, 0:nw]
    lx, ly = xx * (Sw // nw), yy * (Sh // nh)
    lx = np.where(lx == Sw - 1, lx - 1, lx)
    ly = np.where(ly == Sh - 1, ly - 1, ly)
    r = np.stack([tgt[int(g["y"]):int(g["y"]) + nh, int(g["x"]):int(g["x"]) + nw].reshape(-1) for g in rngs])
    r = r.astype(np.float32)
    F = np.zeros((len(rngs), len(doms), T), np.float32)
    for i, d in enumerate(doms):
        for t in range(T):
            a = _KMAP[t]
            px = int(d["x"]) + a[0] * lx + a[1] * ly + a[2] * (Sw - 1) + a[3] * (Sh - 1)
            py = int(d["y"]) + a[4] * lx + a[5] * ly + a[6] * (Sw - 1) + a[7] * (Sh - 1)
            M = s[py, px] + s[py + a[4], px + a[0]] + s[py + a[5], px + a[1]] + s[py + a[4] + a[5], px + a[0] + a[1]]
            val = r - (M.reshape(-1).astype(np.float32) / np.float32(4.0))[None, :]
            F[:, i, t] = np.cumsum(val * val, axis=1, dtype=np.float32)[:, -1]
    return F
