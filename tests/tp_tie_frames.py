"""Frames whose least error is attained in several 4-tile chunks of the tiled form's window, and a numpy restatement
of the layout that says where (fracenc_tp.hip, search_dft CHUNKED): per classifier bucket the domains in a stable
argsort of ΣD4, tiles of 32 of them, chunks of 4 tiles counted from the window's t0; a domain's row in its tile is
its sorted position mod 32 and its row half (row // 4) % 2.  The window rule is auto_prune_frames.predict's, restated
here for separate source and target planes.

The search keeps, per range slot and row half, the window's maximum, how many chunks attain it and the first two of
them (one record); the resolve evaluates the listed chunks, or the whole window when more than two attain it.  So
what matters for a range is how many chunks attain its least error in one row half, and in which order they come:

  planted(seed, plants)   256², source and target uniform integers in [32, 224); constant 16×16 blocks in the source
                          at (48 + 48·k, 48), each optionally with its first 8×8 quarter at a second level; the
                          target's range at (104, 104) constant at 128.  Against that range a constant domain at
                          level b costs 1024·(128 − b)², a 128 block with a quarter at 120 costs 16·32² = 16384, and
                          every noise domain several hundred thousand.  The group of the constant range also holds
                          255 noise ranges, whose seed bound is huge: the window is the whole bucket and t0 = 0.

test_tp_tie_frames.py checks each case's property on the CPU; test_gpu_tp_records.py runs them.
"""
from __future__ import annotations

import numpy as np

from auto_prune_frames import EXACT_LIMIT, grid

S = 256
RANGE_XY = (104, 104)     # the constant range of a planted frame
RANGE_INDEX = (104 // 8) * (S // 8) + 104 // 8
LEVEL = 128

# name → (seed, plants, thr); a plant is (level, quarter level or None)
CASES = {
    "two": (1, ((124, None), (132, None)), 0.0),
    "three": (4, ((124, None), (128, 120), (132, None)), 0.0),
    "superseded": (10, ((124, None), (128, 120), (129, None)), 0.0),
    "two_hits": (1, ((124, None), (132, None)), 4.0),   # H = 16384: both tied domains are hits
    "exact": (2, ((128, None),), 0.0),
}


def planted(seed: int, plants):
    rng = np.random.default_rng(seed)
    src = rng.integers(32, 224, (S, S)).astype(np.uint8)
    tgt = rng.integers(32, 224, (S, S)).astype(np.uint8)
    for k, (level, quarter) in enumerate(plants):
        x, y = 48 + 48 * k, 48
        src[y:y + 16, x:x + 16] = level
        if quarter is not None:
            src[y:y + 8, x:x + 8] = quarter
    x, y = RANGE_XY
    tgt[y:y + 8, x:x + 8] = LEVEL
    return src, tgt


INNER_SEED = 3
DECOY = 68  # the domain at (48, 16)


def inner_bucket():
    """(src, tgt, rcat, dcat): "three" with the walk's end at stake.  A fourth block at 124 is planted at (48, 16):
    domain DECOY, which costs the constant range the least error too and comes first in domain order — but it
    is put, by hand, in a second category with the last 19 domains, and every range in the first.  The first
    bucket's 941 domains are 30 tiles, so its window's last chunk (tiles 28, 29) would run on into tile 30: the
    second bucket's only tile, where the decoy sits, in the row half of the three attaining chunks.  A walk over
    the whole window that ends at the chunk's fourth tile, not at the window's t1, would pick the decoy."""
    src, tgt = planted(INNER_SEED, CASES["three"][1])
    src[16:32, 48:64] = 124
    dcat = np.zeros((S // 8 - 1) ** 2, np.int64)
    dcat[DECOY] = 1
    dcat[-19:] = 1
    return src, tgt, np.zeros((S // 8) ** 2, np.int64), dcat


def case(name: str):
    """(src, tgt, thr) of a named case."""
    seed, plants, thr = CASES[name]
    return planted(seed, plants) + (thr,)


def _box(p, x, y, s):
    ii = np.zeros((p.shape[0] + 1, p.shape[1] + 1), np.int64)
    ii[1:, 1:] = p.astype(np.int64).cumsum(0).cumsum(1)
    return ii[y + s, x + s] - ii[y, x + s] - ii[y + s, x] + ii[y, x]


def _d4(p, x, y):
    d = p[y:y + 16, x:x + 16].astype(np.int64)
    return d[0::2, 0::2] + d[0::2, 1::2] + d[1::2, 0::2] + d[1::2, 1::2]


def errors(src, tgt, rx, ry, dx, dy):
    """[nr, nd] the least exact S16 = Σ(4r − D4)² over the four rotations."""
    R = np.stack([4 * tgt[y:y + 8, x:x + 8].astype(np.int64) for x, y in zip(rx, ry)])
    D = np.stack([np.rot90(_d4(src, x, y), k) for x, y in zip(dx, dy) for k in range(4)])
    e = (R * R).sum((1, 2))[:, None] - 2 * np.einsum("rij,dij->rd", R, D) + (D * D).sum((1, 2))[None, :]
    return e.reshape(len(rx), len(dx), 4).min(2)


def layout(src, tgt, hitH: int = -1, ranges=None, rcat=None, dcat=None):
    """The tiled form's layout and windows.  Returns a dict:
    dom_tile, dom_row [nd]  each domain's tile (global index) and row in it (−1: its bucket has no range group);
    rng_group [nr]          each (selected) range's group (−1: its bucket has no domain);
    groups                  [(first tile of the bucket, t0, t1, blocks, range indices, seed tile)];
    pairs, full, seed_pairs, evals, seed_evals, eligible   the counters of auto_prune_frames.predict."""
    H, W = src.shape
    rx, ry = grid(tgt.shape[1], tgt.shape[0], 8, 8)
    if ranges is not None:
        rx, ry = rx[ranges], ry[ranges]
    dx, dy = grid(W, H, 16, 8)
    SRall, SDall = 4 * _box(tgt, rx, ry, 8), _box(src, dx, dy, 16)
    rcat = np.zeros(len(rx), np.int64) if rcat is None else np.asarray(rcat)
    dcat = np.zeros(len(dx), np.int64) if dcat is None else np.asarray(dcat)
    out = dict(pairs=0, full=0, seed_pairs=0, evals=0, seed_evals=0, eligible=0, groups=[],
               dom_tile=np.full(len(dx), -1), dom_row=np.full(len(dx), -1), rng_group=np.full(len(rx), -1))
    tile_first = 0
    for cat in np.unique(np.concatenate([rcat, dcat])):  # buckets in category order (tiles of range-less ones too)
        ri, di = np.flatnonzero(rcat == cat), np.flatnonzero(dcat == cat)
        if not len(di):
            continue
        SR, SD = SRall[ri], SDall[di]
        ro, do = np.argsort(SR, kind="stable"), np.argsort(SD, kind="stable")
        nd, nr = len(do), len(ro)
        nt, nb = (nd + 31) // 32, (nr + 31) // 32
        out["dom_tile"][di[do]] = tile_first + np.arange(nd) // 32
        out["dom_row"][di[do]] = np.arange(nd) % 32
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
            u = int(errors(src, tgt, rx[ri[rs]], ry[ri[rs]], dx[sd], dy[sd]).min(1).max())
            t0, t1 = 0, nt
            if u < EXACT_LIMIT:
                D = int(np.sqrt(64.0 * (max(u, hitH) + 0.5))) + 1
                lo, hi = SR[rs[0]] - D, SR[rs[-1]] + D
                t0 = int(np.searchsorted(tmax, lo, "left"))
                t1 = max(t0, t0 + int(np.searchsorted(tmin[t0:], hi, "right")))
            out["rng_group"][ri[rs]] = len(out["groups"])
            out["groups"].append((tile_first, tile_first + t0, tile_first + t1, gy, ri[rs], tile_first + seed))
            out["pairs"] += gy * (t1 - t0)
            out["full"] += gy * nt
            out["seed_pairs"] += gy
            out["evals"] += len(rs) * max(0, min(t1 * 32, nd) - t0 * 32)
            out["seed_evals"] += len(rs) * len(sd)
        tile_first += nt
    out["share"] = out["pairs"] / max(out["full"], 1)
    return out


def attaining(src, tgt, lay, r: int = RANGE_INDEX, hitH: int = -1):
    """For range r (one bucket): (least error, [(domain, tile, chunk, half, error)] of the domains attaining it, or
    of the hits when the least error is within hitH, in tile order, the same for every other domain inside the
    window).  chunk counts from the window's t0 of r's group."""
    rx, ry = grid(tgt.shape[1], tgt.shape[0], 8, 8)
    dx, dy = grid(src.shape[1], src.shape[0], 16, 8)
    e = errors(src, tgt, rx[r:r + 1], ry[r:r + 1], dx, dy)[0]
    _, t0, t1, _, _, _ = lay["groups"][lay["rng_group"][r]]
    inside = (lay["dom_tile"] >= t0) & (lay["dom_tile"] < t1)  # (one bucket's tiles: other buckets lie outside)
    least = int(e[inside].min())
    want = inside & ((e <= hitH) if least <= hitH else (e == least))

    def rows(sel):
        d = np.flatnonzero(sel)
        d = d[np.lexsort((lay["dom_row"][d], lay["dom_tile"][d]))]
        return [(int(k), int(lay["dom_tile"][k]), int((lay["dom_tile"][k] - t0) // 4), int((lay["dom_row"][k] // 4) % 2),
                 int(e[k])) for k in d]

    return least, rows(want), rows(inside & ~want)
