#!/usr/bin/env python3
"""A CPU model of the pruned route's windows on the C3 frame (4096² value noise, seed 1234; 8×8 ranges, 16×16
domains at stride 8, one bucket), and of how long the windowed search's workgroups take in a given order
(DESIGN §7.10).  numpy only, about 20 s.

The rule is launch_tp's (fracenc_tp.hip): domains sorted by ΣD4 into 32-row tiles, ranges by ΣR = 4Σr into
32-slot blocks, 8 blocks per group; the seed tile of a group is the first whose greatest ΣD4 reaches the middle
block's (first + last) / 2; U_r is the least Σ(4r − D4)² over the seed tile's rows and the four rotations; the
window holds the tiles whose [min, max] ΣD4 meets [min ΣR − D, max ΣR + D] with D = ⌊√(64·(max U + ½))⌋ + 1.

It prints the windows' share of the block × tile pairs — which must equal the library's evaluated share on the same
frame (frac_stats.matrix_flops without the seed, over 6·32768·full pairs; 0.0102 at C3): that is its check — the
window sizes, and the makespan, in tiles, of list scheduling the groups (a workgroup goes to the first free place)
in ΣR order, longest first exactly, and longest first in the 32 classes tp_plan sorts into:
  places  512 independent places (two workgroups per CU that do not slow each other: the latency-bound reading);
  cus     256 CUs of two places whose residents share one tile per unit time (the issue-bound reading).
usage: tools/tp_window_model.py [size] [seed]"""
import heapq
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fractencode_amd.synth import value_noise  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
p = value_noise(S, S, int(sys.argv[2]) if len(sys.argv) > 2 else 1234).astype(np.int64)

# ranges [nr, 8, 8] as 4r; domains [nd, 8, 8] as the 2×2 sums D4
nb, ndx = S // 8, (S - 16) // 8 + 1
R = 4 * p.reshape(nb, 8, nb, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
q = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]  # [S/2, S/2]
win = np.lib.stride_tricks.sliding_window_view(q, (8, 8))[::4, ::4][:ndx, :ndx]
D4 = win.reshape(-1, 8, 8)
SR, SD = R.sum((1, 2)), D4.sum((1, 2))
ro, do = np.argsort(SR, kind="stable"), np.argsort(SD, kind="stable")
nr, nd = len(ro), len(do)
nt, nblk = (nd + 31) // 32, (nr + 31) // 32
tmin = SD[do[0::32]]
tmax = SD[do[np.minimum(np.arange(nt) * 32 + 31, nd - 1)]]

sizes, blocks = [], []
for g0 in range(0, nblk, 8):
    gy = min(8, nblk - g0)
    mid = g0 + gy // 2
    srm = (SR[ro[mid * 32]] + SR[ro[min(mid * 32 + 31, nr - 1)]]) // 2
    seed = min(int(np.searchsorted(tmax, srm, "left")), nt - 1)
    rs = ro[g0 * 32:min((g0 + gy) * 32, nr)]
    d = D4[do[seed * 32:seed * 32 + 32]]
    rot = np.stack([np.rot90(d, k, (1, 2)) for k in range(4)]).reshape(-1, 64)
    r = R[rs].reshape(-1, 64)
    e = (r * r).sum(1)[:, None] - 2 * r @ rot.T + (rot * rot).sum(1)[None, :]
    u = int(e.min(1).max())
    dd = int(np.sqrt(64.0 * (u + 0.5))) + 1
    lo, hi = SR[rs[0]] - dd, SR[rs[-1]] + dd
    t0 = int(np.searchsorted(tmax, lo, "left"))
    t1 = max(t0, t0 + int(np.searchsorted(tmin[t0:], hi, "right")))
    sizes.append(t1 - t0)
    blocks.append(gy)
sizes, blocks = np.array(sizes), np.array(blocks)
pairs, full = int((sizes * blocks).sum()), int(blocks.sum()) * nt
print(f"groups {len(sizes)}, tiles {nt}, pairs {pairs} of {full}: share {pairs / full:.5f}")
k = len(sizes) // 50 or 1
print(f"window tiles: mean {sizes.mean():.1f}, median {int(np.median(sizes))}, p90 {int(np.percentile(sizes, 90))}, "
      f"max {sizes.max()}; first groups {sizes[:k].mean():.0f}, middle {sizes[len(sizes) // 2 - k:len(sizes) // 2 + k].mean():.0f}, "
      f"last {sizes[-k:].mean():.0f}")


def places(order, n=512):
    free = [0.0] * n
    heapq.heapify(free)
    end = 0.0
    for g in order:
        t = heapq.heappop(free) + sizes[g]
        end = max(end, t)
        heapq.heappush(free, t)
    return end


def cus(order, n=256, slots=2):
    """Every CU gives its residents one tile per unit time in all; a finished workgroup's place takes the next."""
    left = [[] for _ in range(n)]  # remaining tiles of each CU's residents
    nxt, now, order = 0, 0.0, list(order)
    # (the first 2n workgroups go round the CUs in turn, as the dispatcher fills an empty device)
    for i in range(min(len(order), n * slots)):
        left[i % n].append(float(sizes[order[i]]))
        nxt = i + 1
    while any(left):
        # time until the next workgroup anywhere ends: its remaining tiles times its CU's residents
        dt, cmin = min((min(x) * len(x), c) for c, x in enumerate(left) if x)
        now += dt
        for c, x in enumerate(left):
            if x:
                step = dt / len(x)
                left[c] = [v - step for v in x]
        done = [c for c, x in enumerate(left) if any(v <= 1e-9 for v in x)]
        for c in done:
            left[c] = [v for v in left[c] if v > 1e-9]
            while len(left[c]) < slots and nxt < len(order):
                left[c].append(float(sizes[order[nxt]]))
                nxt += 1
    return now


ident = np.arange(len(sizes))
w = sizes * blocks  # tp_plan sorts by pairs[g]
exact = np.argsort(-w, kind="stable")
cls = 31 - (w * 32) // (w.max() + 1)
classes = np.argsort(cls, kind="stable")
for name, f, ideal in (("places", places, sizes.sum() / 512), ("cus", cus, sizes.sum() / 256)):
    print(f"{name}: in order {f(ident):.0f}, longest first {f(exact):.0f}, 32 classes {f(classes):.0f}, ideal {ideal:.0f}")
