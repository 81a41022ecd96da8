#!/usr/bin/env python3
"""The rate–distortion-pruned quadtree partition beside the split distance's, in one process on one GPU, at the C4
configuration (classifier on, levels 16/8/4, T = 4, 5 + 7 bits) on two frames: the benchmark's C4 frame (the 2048²
crop of the S1 value noise, seed 1234) and the whole 4096² value-noise frame.  Per frame the full tree is searched
once (Engine.quadtree_rate); then, for a handful of budgets that are the split-distance route's own stream sizes
(rate_fit at fractions of the way from the smallest to the largest stream), both routes answer from that state:

  threshold   rate_fit + rate_stream: the smallest split distance that fits
  rd          rd_fit + rd_stream: the multiplier whose pruned partition fits

and the tool reports, per budget and route, the stream's bytes, the summed distortion (Σ q over the leaves,
q = 16 × the block's squared error; the threshold route's from rate_leaves on the host, the RD route's as rd_fit
reports it — the tool asserts that rd_leaves gives the same sum), the PSNR of decode_frq1 against the frame — of the
stream itself (5 + 7 bits, with the contrast and brightness ranges its one quantizer pair spans) and of the same
leaves packed with 16 + 16 bits, which shows the partition without the quantizer — and the time of the two calls
(a host clock around calls that end synchronised; the routes alternate within each repeat).  Beside it: rd_sizes of 64 multipliers in one call against 64 calls of one.  Every path is warmed up;
times are medians with their range over the repeats.  One JSON line per frame.
usage: tools/quadtree_rd.py [reps] [--out FILE]"""
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import fractencode_amd as F  # noqa: E402
from fractencode_amd.synth import value_noise  # noqa: E402

SIZES, T = (16, 4), 4
FRACTIONS = (0.05, 0.15, 0.3, 0.5, 0.75)  # of the way from the smallest to the largest stream


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3),
            "n": len(ms)}


def take(args, flag, default):
    if flag not in args:
        return default
    k = args.index(flag)
    v = args[k + 1]
    del args[k:k + 2]
    return v


def distortion(leaves) -> int:
    """Σ q over QT_LEAF leaves: q = rint(distance · 64n²), 0 for a negative or NaN distance."""
    n = (1 << (leaves["code"] >> 28)).astype(np.float64)
    d = leaves["distance"]
    return int(np.rint(np.where(d > 0, d, 0.0) * 64.0 * n * n).astype(np.int64).sum())


def psnr(e, stream, plane) -> float:
    out = e.decode_frq1(stream)[0]
    mse = float(np.mean((out.astype(np.float64) - plane.astype(np.float64)) ** 2))
    return round(10.0 * math.log10(255.0 ** 2 / mse), 4) if mse > 0 else float("inf")


def quality(e, stream, leaves, plane) -> dict:
    """PSNR of the stream, its quantizer ranges, and the PSNR of the same leaves at 16 + 16 bits."""
    H, W = plane.shape
    h = F.frq1_info(stream)
    fine = F.pack_frq1(leaves, W, H, SIZES[0], SIZES[1], T, True, 16, 16)
    return {"psnr_db": psnr(e, stream, plane), "psnr_16_16_db": psnr(e, fine, plane),
            "contrast_range": [h["contrast_min"], h["contrast_max"]],
            "brightness_range": [h["brightness_min"], h["brightness_max"]]}


def clock(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def measure(name, plane, reps):
    H, W = plane.shape
    with F.Engine(0, T, True) as e:
        e.set_frame(plane)
        e.quadtree_rate(*SIZES)
        ends, _, _ = e.rate_sizes([-1.0, np.inf])
        largest, smallest = int(ends[0]), int(ends[1])
        rd_ends = e.rd_sizes([0, 1 << 32])
        budgets = []
        for f in FRACTIONS:  # the threshold route's own size at or below the target
            b = e.rate_fit(int(smallest + f * (largest - smallest)))[1]
            if b not in budgets:
                budgets.append(b)

        def threshold(b):
            t, size, n = e.rate_fit(b)
            return (t, size, n), e.rate_stream(t)

        def rd(b):
            lam, size, n, dist = e.rd_fit(b)
            return (lam, size, n, dist), e.rd_stream(lam)

        rows = []
        for b in budgets:
            for _ in range(2):  # warm-up: buffers allocated, kernels loaded
                threshold(b)
                rd(b)
            tw, rw = [], []
            for _ in range(reps):  # the two routes alternate
                (tf, ts), ms = clock(lambda: threshold(b))
                tw.append(ms)
                (rf, rs), ms = clock(lambda: rd(b))
                rw.append(ms)
            assert len(ts) == tf[1] <= b and len(rs) == rf[1] <= b
            rl = e.rd_leaves(rf[0])
            assert len(rl) == rf[2] and distortion(rl) == rf[3], "rd_fit's distortion is not its leaves'"
            assert rs == F.pack_frq1(rl, W, H, SIZES[0], SIZES[1], T, True), "rd_stream differs from the host packer"
            tl = e.rate_leaves(tf[0])
            td = distortion(tl)
            rows.append({"budget_bytes": b,
                         "threshold": {"split_distance": tf[0], "bytes": tf[1], "leaves": tf[2], "distortion": td,
                                       **quality(e, ts, tl, plane), **stats(tw)},
                         "rd": {"lambda": rf[0], "bytes": rf[1], "leaves": rf[2], "distortion": rf[3],
                                **quality(e, rs, rl, plane), **stats(rw)}})
            r = rows[-1]
            r["distortion_ratio"] = round(rf[3] / td, 4) if td else None
            r["psnr_gain_db"] = round(r["rd"]["psnr_db"] - r["threshold"]["psnr_db"], 4)
            r["psnr_16_16_gain_db"] = round(r["rd"]["psnr_16_16_db"] - r["threshold"]["psnr_16_16_db"], 4)
        # 64 multipliers: one call against 64 calls of one
        lams = np.unique(np.round(np.logspace(0, 32 * math.log10(2), 96)).astype(np.uint64))[-64:]
        assert len(lams) == 64
        for _ in range(2):
            one = e.rd_sizes(lams)
            each = [e.rd_sizes(lams[i:i + 1]) for i in range(64)]
        assert all(np.array_equal(np.concatenate([x[k] for x in each]), one[k]) for k in range(4))
        w1, w64 = [], []
        for _ in range(reps):
            w1.append(clock(lambda: e.rd_sizes(lams))[1])
            w64.append(clock(lambda: [e.rd_sizes(lams[i:i + 1]) for i in range(64)])[1])
    return {"tool": "quadtree_rd", "frame": name, "size": [W, H], "sizes": [16, 8, 4], "transforms": T,
            "classifier": True, "smallest_bytes": smallest, "largest_bytes": largest,
            "rd_ends": {"lambda_0": {"bytes": int(rd_ends[0][0]), "distortion": int(rd_ends[3][0])},
                        "lambda_2^32": {"bytes": int(rd_ends[0][1]), "distortion": int(rd_ends[3][1])}},
            "budgets": rows, "sizes64": {"one_call": stats(w1), "calls_of_one": stats(w64)},
            "build_id": F.build_info()["build_id"]}


def main():
    args = sys.argv[1:]
    out_path = take(args, "--out", None)
    reps = max(12, int(args[0])) if args else 12
    s1 = value_noise(4096, 4096, 1234)
    frames = {"c4": s1[:2048, :2048].copy(), "value_noise": s1}
    lines = [json.dumps(measure(name, p, reps)) for name, p in frames.items()]
    print("\n".join(lines), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
