"""Host-side frames for the SEA engine's tests (test_sea_frames.py checks their properties against the
oracle on the CPU, test_gpu_sea.py runs both SEA forms on them).  Plain numpy, fixed seeds.

The successive-elimination bound (fracenc_sea.hip) is LB = (ΣR − ΣD4)²/n² + (cR − cD)² ≤ S16.  It is an
equality when range and domain are both constant, so a constant range's best constant domain sits exactly on
the edge of the window the bound allows: a bound one unit too tight loses the winner.
"""
from __future__ import annotations

import numpy as np

# seeds for which test_sea_frames.py holds (the frames are deterministic: the GPU tests use the same ones)
LEVELS_SEED = 3
CLOSE_LEVELS_SEED = 5
SMOOTH_SEED = 77
# 248×200 with the classifier: the tiled form bounds a window per group of 256 ranges of one bucket, so at this
# size it prunes only where a bucket has more than 256 ranges (a second, small group); seed 85 has one
SMOOTH_PRUNE_SEED = 85
OUTLIERS_SEED = 9
FLAT_SEED = 41

DELTAS = tuple(range(-5, 6))


def levels(seed: int, S: int = 256, spacing: int = 10, deltas=DELTAS, nlevels: int = 21):
    """(src, tgt), two S×S planes for set_planes.

    src: constant 16×16 blocks at levels 20 + spacing·k (k < nlevels: {20, 30, …, 220} by default), drawn
    block by block in raster order from the levels that are not exactly `spacing` away from the block to the
    left or the block above.  Domains (16×16 at stride 8) that lie on one block, or on neighbours of one
    level, are constant; the others straddle levels at least 2·spacing apart.
    tgt: constant 8×8 cells, each a level b that occurs in src plus δ ∈ deltas.  Every (level, δ) pair occurs
    (S²/64 cells ≥ levels · deltas), in shuffled order.

    A constant range a against a constant domain b: S16 = 1024·(a − b)², all of it the bound's mean term.  A
    domain made of quarters at levels b_q costs 256·Σ_q (a − b_q)²; with a = b + δ, |δ| ≤ spacing/2 and no two
    neighbours `spacing` apart that is more than 1024·δ², so the least error is attained by exactly the
    constant domains of the nearest level (of both nearest levels for |δ| = spacing/2): many domains of one
    ΣD4, spread over the ΣD4-sorted tiles and chunks, of which the earliest in domain order must win.
    δ = 0 is an exact copy (a hit at thr = 0: the first domain, t = 0).  With spacing 10 and thr = 1.5
    (H = 6144) the hits are |δ| ≤ 2, all of one ΣD4 per range; with spacing 4 and δ = ±2 a range's hits are
    the constant domains of two levels, so its first hit in domain order can sort after another hit.
    """
    assert S % 16 == 0 and 20 + spacing * (nlevels - 1) + max(deltas) <= 255 and 20 + min(deltas) >= 0
    rng = np.random.default_rng(seed)
    nb = S // 16
    lv = np.zeros((nb, nb), np.int64)
    for y in range(nb):
        for x in range(nb):
            ok = np.ones(nlevels, bool)
            for ny, nx in ((y, x - 1), (y - 1, x)):
                if ny >= 0 and nx >= 0:
                    for k in (lv[ny, nx] - 1, lv[ny, nx] + 1):
                        if 0 <= k < nlevels:
                            ok[k] = False
            lv[y, x] = rng.choice(np.flatnonzero(ok))
    src = (20 + spacing * lv).astype(np.uint8).repeat(16, 0).repeat(16, 1)
    present = np.unique(lv)
    pairs = np.array([(20 + spacing * k, d) for k in present for d in deltas], np.int64)
    nc = (S // 8) ** 2
    assert len(pairs) <= nc
    pick = np.concatenate([np.arange(len(pairs)), rng.integers(0, len(pairs), nc - len(pairs))])
    rng.shuffle(pick)
    cells = (pairs[pick, 0] + pairs[pick, 1]).reshape(S // 8, S // 8)
    tgt = cells.astype(np.uint8).repeat(8, 0).repeat(8, 1)
    return np.ascontiguousarray(src), np.ascontiguousarray(tgt)


def close_levels(seed: int, S: int = 256):
    """levels() with the levels 4 apart and δ ∈ {−2 … 2}: at thr = 1.5 every range is a hit and the ranges
    with δ = ±2 hit the constant domains of two levels (two different ΣD4)."""
    return levels(seed, S, spacing=4, deltas=(-2, -1, 0, 1, 2))


def smooth(seed: int, W: int, H: int) -> np.ndarray:
    """A low-frequency frame (the project's value noise): the best error is small against the spread of
    ΣD4, so the windows are narrow."""
    from fractencode_amd.synth import value_noise
    return value_noise(W, H, seed)


def flat(seed: int, W: int, H: int) -> np.ndarray:
    """test_gpu_parity.py's "flat" kind: 4×4 constant cells at three levels (exact matches, ties, hits)."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 3, (H // 4, W // 4), dtype=np.uint8) * 60).repeat(4, 0).repeat(4, 1)


def outliers(seed: int, S: int = 128):
    """(src, tgt, kinds): src is value noise scaled into [64, 192] with one constant 32×32 patch at 64 and
    one at 192; tgt is src with every 7th 8×8 range all 0 and every 7th (offset 3) all 255; kinds[y, x] of
    the range grid is −1 (all 0), +1 (all 255) or 0 (ordinary).  ΣR = 0 lies below every ΣD4 and
    ΣR = 4·64·255 above, so one side of the sorted order is closed before the first step.  The patches keep
    the outliers in the exact regime: S16 = 64·(4·64)² = 2^22 and 64·(4·63)² against them, below 2^24."""
    assert S % 32 == 0 and S >= 96
    src = (64 + (smooth(seed, S, S).astype(np.uint32) * 128) // 255).astype(np.uint8)
    src[8:40, 8:40] = 64
    src[S - 40:S - 8, S - 40:S - 8] = 192
    tgt = src.copy()
    g = S // 8
    kinds = np.zeros((g, g), np.int8)
    idx = np.arange(g * g).reshape(g, g)
    kinds[idx % 7 == 0] = -1
    kinds[idx % 7 == 3] = 1
    full = kinds.repeat(8, 0).repeat(8, 1)
    tgt[full < 0] = 0
    tgt[full > 0] = 255
    return np.ascontiguousarray(src), np.ascontiguousarray(tgt), kinds


def bright_blocks(S: int = 256, n: int = 8) -> np.ndarray:
    """The frame of test_fp32_regime_through_the_fallback_grid: isolated bright n×n blocks 4n apart on a
    black frame.  Every domain is mostly dark, so each bright range's best S16 is at least 2^24."""
    p = np.zeros((S, S), np.uint8)
    for y in range(n, S - n, 4 * n):
        for x in range(n, S - n, 4 * n):
            p[y:y + n, x:x + n] = 255
    return p


def constant_errors(src: np.ndarray, tgt: np.ndarray, n: int = 8):
    """For planes whose n×n ranges are constant: the exact S16 of every (range, domain) pair, which does not
    depend on the transform (a permutation of the domain's cells against a constant):
    S16 = n²·(4a)² − 2·4a·ΣD4 + ΣD4².  Returns (E [nr, nd] int64, a [nr], ΣD4 [nd], constant-domain mask
    [nd]) in the uniform grids' row-major order (ranges n at stride n, domains 2n at stride n)."""
    s = src.astype(np.int64)
    H, W = s.shape
    d4 = s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2]  # decimated plane, cells of 2×2 sums
    ny, nx = (H - 2 * n) // n + 1, (W - 2 * n) // n + 1
    h = n // 2
    sd = np.zeros(ny * nx, np.int64)
    qd = np.zeros(ny * nx, np.int64)
    const = np.zeros(ny * nx, bool)
    for j in range(ny):
        for i in range(nx):
            c = d4[j * h:j * h + n, i * h:i * h + n]
            sd[j * nx + i] = c.sum()
            qd[j * nx + i] = (c * c).sum()
            const[j * nx + i] = (s[j * n:j * n + 2 * n, i * n:i * n + 2 * n] == s[j * n, i * n]).all()
    t = tgt.astype(np.int64)
    a = t[0::n, 0::n][:t.shape[0] // n, :t.shape[1] // n].reshape(-1)
    E = n * n * 16 * a[:, None] ** 2 - 8 * a[:, None] * sd[None, :] + qd[None, :]
    return E, a, sd, const
