"""Frames for AUTO's pruned route (test_gpu_auto_prune.py) and a numpy restatement of the tiled form's window rule
(fracenc_tp.hip: tp_seed_work, tp_seed_reduce, tp_windows) that predicts, on the CPU, the share of the run's
block × tile pairs the windows hold.  The route is decided by that share against kAutoPruneBudget, so a test
frame is useful only when its prediction is far from the budget: the pruned cases use frames predicted at
most a quarter of it, the fallback cases frames predicted exactly 1 (test_auto_prune_frames.py checks both).

Why not plain value noise or a ramp at 256×256: a frame of 1,024 ranges is four groups of 256 ΣR-sorted ranges,
each spanning a quarter of the ΣR distribution, and on a smooth frame ΣD4 (a local mean) is distributed as
ΣR is — every window holds a quarter of the tiles or more.  Predicted shares: value noise (seed 77) 0.694 at
256×256 and 0.708 at 264×248, the diagonal ramp 0.589.  Those frames are kept as cases whose route follows
from their prediction (over the budget: the fallback).  `mosaic` is the frame that prunes at this size: four
levels, one per group, each 8×8 range flat at one of them (plus optional low noise) and placed at random, so
only the few domains whose four quadrants share a level sit at a level's ΣD4 and every other domain lies
between levels, outside every window.
"""
from __future__ import annotations

import numpy as np

BUDGET = 0.375         # kAutoPruneBudget (fracenc_plan.hip)
EXACT_LIMIT = 1 << 24  # kExactLimit: above it tp_seed_reduce gives no bound

# levels whose sums of four (a domain's quadrants) meet 4·L only as L + L + L + L, and miss it by 31 or more
LEVELS = (16, 80, 177, 241)
MOSAIC_SEED, NOISE_SEED = 11, 5


def mosaic_cells(W: int, H: int, seed: int = MOSAIC_SEED) -> np.ndarray:
    """The level index (0..3) of each 8×8 cell, row-major as the range grid: equal numbers (the highest level
    takes the shortfall), shuffled."""
    ny, nx = H // 8, W // 8
    per = -(-ny * nx // len(LEVELS))
    cells = np.repeat(np.arange(len(LEVELS)), per)[:ny * nx]
    np.random.default_rng(seed).shuffle(cells)
    return cells


def mosaic(W: int, H: int, seed: int = MOSAIC_SEED, amp: int = 0, noise_seed: int = 0) -> np.ndarray:
    """8×8 cells at LEVELS (mosaic_cells); amp > 0 adds i.i.d. integers in [−amp, amp] per pixel, which keeps
    every ΣR of a level below every ΣR of the next."""
    ny, nx = H // 8, W // 8
    p = np.asarray(LEVELS, np.int64)[mosaic_cells(W, H, seed)].reshape(ny, nx).repeat(8, 0).repeat(8, 1)
    if amp:
        p = p + np.random.default_rng(noise_seed).integers(-amp, amp + 1, p.shape)
    out = np.zeros((H, W), np.int64)
    out[:p.shape[0], :p.shape[1]] = p
    out[p.shape[0]:, :] = out[p.shape[0] - 1:p.shape[0], :]  # (heights that are no multiple of 8: repeat the edge)
    return np.clip(out, 0, 255).astype(np.uint8)


def mosaic_shard(W: int, H: int, seed: int = MOSAIC_SEED, top: int = 32) -> np.ndarray:
    """Range indices of a shard whose ΣR-sorted groups stay one level each: every range of the three lower
    levels and the first `top` of the highest — groups of 8, 8, 8 and top / 32 blocks."""
    c = mosaic_cells(W, H, seed)
    return np.sort(np.concatenate([np.flatnonzero(c < 3), np.flatnonzero(c == 3)[:top]]))


def ramp(W: int, H: int) -> np.ndarray:
    y, x = np.mgrid[0:H, 0:W]
    return np.minimum((x + y) // 2, 255).astype(np.uint8)


def noise(W: int, H: int, seed: int = NOISE_SEED) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


def grid(W: int, H: int, size: int, step: int):
    """createUniformGrid's origins, row-major: (x, y) int arrays."""
    ys, xs = np.meshgrid(np.arange(0, H - size + 1, step), np.arange(0, W - size + 1, step), indexing="ij")
    return xs.reshape(-1), ys.reshape(-1)


def _d4(p: np.ndarray, x: int, y: int) -> np.ndarray:
    d = p[y:y + 16, x:x + 16].astype(np.int64)
    return d[0::2, 0::2] + d[0::2, 1::2] + d[1::2, 0::2] + d[1::2, 1::2]


def seed_bound(p: np.ndarray, rx, ry, dx, dy) -> np.ndarray:
    """Per range the least exact S16 = Σ(4r − D4)² over the given domains and the four rotations."""
    R = np.stack([4 * p[y:y + 8, x:x + 8].astype(np.int64) for x, y in zip(rx, ry)])        # [nr, 8, 8]
    D = np.stack([np.rot90(_d4(p, x, y), k) for x, y in zip(dx, dy) for k in range(4)])      # [4·nd, 8, 8]
    e = (R * R).sum((1, 2))[:, None] - 2 * np.einsum("rij,dij->rd", R, D) + (D * D).sum((1, 2))[None, :]
    return e.min(1)


def predict(p: np.ndarray, dstep: int = 8, hitH: int = -1, ranges=None, bound=seed_bound, rcat=None, dcat=None):
    """The window rule restated.  Returns a dict: share (the windows' block × tile pairs ÷ all), pairs, full,
    seed_pairs (blocks with a seed tile), evals / seed_evals ((range, domain) pairs in the windows / the seed
    tiles), eligible ((range, domain) pairs of one bucket) and groups [(range indices, seed domain indices)].
    `ranges` selects a sub-list of the 8×8 grid; rcat / dcat are the classifier's categories of the (selected)
    ranges and of the domains (None: one bucket); `bound(p, rx, ry, dx, dy)` gives the per-range seed bound
    (the GPU test passes the VALU engine's)."""
    H, W = p.shape
    rx, ry = grid(W, H, 8, 8)
    if ranges is not None:
        rx, ry = rx[ranges], ry[ranges]
    dx, dy = grid(W, H, 16, dstep)
    ii = np.zeros((H + 1, W + 1), np.int64)
    ii[1:, 1:] = p.astype(np.int64).cumsum(0).cumsum(1)
    box = lambda x, y, s: ii[y + s, x + s] - ii[y, x + s] - ii[y + s, x] + ii[y, x]
    SRall, SDall = 4 * box(rx, ry, 8), box(dx, dy, 16)
    rcat = np.zeros(len(rx), np.int64) if rcat is None else np.asarray(rcat)
    dcat = np.zeros(len(dx), np.int64) if dcat is None else np.asarray(dcat)
    out = dict(pairs=0, full=0, seed_pairs=0, evals=0, seed_evals=0, eligible=0, groups=[])
    for cat in np.unique(rcat):  # buckets in category order; inside one, the items keep their order
        ri, di = np.flatnonzero(rcat == cat), np.flatnonzero(dcat == cat)
        if not len(di):
            continue  # no domain: no group, the bucket's ranges keep the default record
        SR, SD = SRall[ri], SDall[di]
        ro, do = np.argsort(SR, kind="stable"), np.argsort(SD, kind="stable")  # (the radix sort is stable)
        nd, nr = len(do), len(ro)
        nt, nb = (nd + 31) // 32, (nr + 31) // 32
        tmin = SD[do[0::32]]
        tmax = SD[do[np.minimum(np.arange(nt) * 32 + 31, nd - 1)]]
        out["eligible"] += nr * nd
        for g0 in range(0, nb, 8):
            gy = min(8, nb - g0)
            mid = g0 + gy // 2
            SRm = (SR[ro[mid * 32]] + SR[ro[min(mid * 32 + 31, nr - 1)]]) // 2
            seed = min(int(np.searchsorted(tmax, SRm, "left")), nt - 1)
            sd = di[do[seed * 32:seed * 32 + 32]]
            rs = ro[g0 * 32:min((g0 + gy) * 32, nr)]
            u = int(np.max(bound(p, rx[ri[rs]], ry[ri[rs]], dx[sd], dy[sd])))
            t0, t1 = 0, nt
            if u < EXACT_LIMIT:
                D = int(np.sqrt(64.0 * (max(u, hitH) + 0.5))) + 1
                lo, hi = SR[rs[0]] - D, SR[rs[-1]] + D
                t0 = int(np.searchsorted(tmax, lo, "left"))
                t1 = max(t0, t0 + int(np.searchsorted(tmin[t0:], hi, "right")))
            out["pairs"] += gy * (t1 - t0)
            out["full"] += gy * nt
            out["seed_pairs"] += gy
            out["evals"] += len(rs) * max(0, min(t1 * 32, nd) - t0 * 32)
            out["seed_evals"] += len(rs) * len(sd)
            out["groups"].append((ri[rs], sd))
    out["share"] = out["pairs"] / max(out["full"], 1)
    return out
