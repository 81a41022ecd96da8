#!/usr/bin/env python3
"""Cost of the quadtree rate sweep at the C4 configuration (2048², classifier on, levels 16/8/4, T = 4, 5 + 7
bits), in one process on one GPU, on two frames: the 2048² crop of the S1 value noise (seed 1234) and uniform
random noise (seed 7).  Per frame:

  build      Engine.quadtree_rate: the full tree searched once, keys sorted and counted
  fit        Engine.rate_fit for a budget half-way between the smallest and the largest stream
  sizes64    one Engine.rate_sizes call of 64 thresholds spread over the candidates' range
  emit       Engine.rate_leaves at the fit's split distance t*, into pinned memory
  enc_tstar  the fixed-threshold encode_quadtree(leaves=True) at t*, into pinned memory
  enc_full   the same at split distance −1, which searches the same nodes as the build: what the build's
             search costs without the state it keeps
  bisect     a host bisection over encode_quadtree(leaves=True) + pack_frq1 (encode_quadtree_stream's two
             steps) for the same budget between 0 and the default record's distance (1e5).  It cannot know when
             it has the best answer; it stops when, with probes on both sides of the budget behind it, a probe
             returns the partition of the previous probe on its side, or after 64 probes.  Its probe count,
             total time, and whether its answer is the exact one

Each path is warmed up; a host clock surrounds calls that end synchronised, and events on the engine's stream
give the device span of the same calls.  The tool asserts that emit returns the leaves of enc_tstar and that the
fit's size is the packed stream's, and prints one JSON line per frame (medians and spread in ms).
usage: tools/quadtree_rate.py [reps] [--out FILE]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fractencode_amd as F  # noqa: E402
from fractencode_amd.synth import value_noise  # noqa: E402

S, SIZES, T = 2048, (16, 4), 4


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3),
            "p10_ms": round(ms[len(ms) // 10], 3), "p90_ms": round(ms[(len(ms) * 9) // 10], 3), "n": len(ms)}


def take(args, flag, default):
    if flag not in args:
        return default
    k = args.index(flag)
    v = args[k + 1]
    del args[k:k + 2]
    return v


def same_partition(a, b):
    return len(a) == len(b) and np.array_equal(a["x"], b["x"]) and np.array_equal(a["y"], b["y"]) and \
        np.array_equal(a["code"] >> 28, b["code"] >> 28)


def bisect(e, budget):
    """(probes, split distance, bytes) of a host bisection for the smallest split distance within the budget."""
    lo, hi, best = 0.0, 1e5, None
    end = {True: None, False: None}  # the last probe's leaves on either side of the budget
    for probe in range(1, 65):
        mid = 0.5 * (lo + hi)
        leaves, _ = e.encode_quadtree(SIZES[0], SIZES[1], mid, leaves=True)
        size = len(F.pack_frq1(leaves, S, S, SIZES[0], SIZES[1], T, True))
        fits = size <= budget
        repeat = end[fits] is not None and end[not fits] is not None and same_partition(leaves, end[fits])
        end[fits] = leaves
        if fits:
            hi, best = mid, (mid, size)
        else:
            lo = mid
        if repeat:
            break
    return probe, best


def measure(name, plane, reps):
    cap = (S // SIZES[1]) ** 2
    pinned = torch.zeros(cap * F.QT_LEAF.itemsize, dtype=torch.uint8).pin_memory().numpy().view(F.QT_LEAF)
    with F.Engine(0, T, True) as e:
        stream = torch.cuda.ExternalStream(e.stream_handle())
        e.set_frame(plane)
        e.quadtree_rate(*SIZES)
        ends, _, _ = e.rate_sizes([-1.0, np.inf])
        budget = int(ends[0] + ends[1]) // 2
        tstar, fit_bytes, fit_leaves = e.rate_fit(budget)
        sweep = np.linspace(0.0, 2.0 * max(tstar, 1.0), 64)
        paths = {
            "build": lambda: e.quadtree_rate(*SIZES),
            "fit": lambda: e.rate_fit(budget),
            "sizes64": lambda: e.rate_sizes(sweep),
            "emit": lambda: e.rate_leaves(tstar, out=pinned),
            "enc_tstar": lambda: e.encode_quadtree(SIZES[0], SIZES[1], tstar, out=pinned, leaves=True)[0],
            "enc_full": lambda: e.encode_quadtree(SIZES[0], SIZES[1], -1.0, out=pinned, leaves=True)[0],
        }
        wall = {k: [] for k in paths}
        dev = {k: [] for k in paths}

        def timed(k):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            t0 = time.perf_counter()
            r = paths[k]()
            w = (time.perf_counter() - t0) * 1e3
            b.record(stream)
            b.synchronize()
            wall[k].append(w)
            dev[k].append(a.elapsed_time(b))
            return r

        # every reader needs the state, which the fixed-threshold encodes end: the build runs before the readers
        order = ("enc_tstar", "enc_full", "build", "fit", "sizes64", "emit")
        for _ in range(2):  # warm-up: buffers allocated, kernels loaded
            for k in order:
                paths[k]()
        for _ in range(reps):
            fixed = timed("enc_tstar").copy()
            timed("enc_full")
            timed("build")
            assert timed("fit") == (tstar, fit_bytes, fit_leaves)
            timed("sizes64")
            got = timed("emit")
            assert np.array_equal(got, fixed), "emit differs from the fixed-threshold encode at t*"
        assert len(F.pack_frq1(got, S, S, SIZES[0], SIZES[1], T, True)) == fit_bytes <= budget
        for k in wall:  # the first two timed calls still pay for first-use effects the warm-up left
            wall[k], dev[k] = wall[k][2:], dev[k][2:]
        bis = []
        for _ in range(3):
            t0 = time.perf_counter()
            probes, best = bisect(e, budget)
            bis.append((time.perf_counter() - t0) * 1e3)
    line = {"tool": "quadtree_rate", "frame": name, "size": [S, S], "sizes": [16, 8, 4], "transforms": T,
            "classifier": True, "budget_bytes": budget, "smallest_bytes": int(ends[1]), "largest_bytes": int(ends[0]),
            "fit": {"split_distance": tstar, "bytes": fit_bytes, "leaves": fit_leaves},
            "bisect": {"probes": probes, "split_distance": best[0] if best else None,
                       "bytes": best[1] if best else None, "exact": bool(best and best[1] == fit_bytes),
                       **stats(bis)},
            "wall": {k: stats(v) for k, v in wall.items()}, "device": {k: stats(v) for k, v in dev.items()},
            "build_id": F.build_info()["build_id"]}
    w = {k: line["wall"][k]["median_ms"] for k in wall}
    line["answer_ms"] = round(w["build"] + w["fit"] + w["emit"], 3)
    line["build_over_enc_full"] = round(w["build"] / w["enc_full"], 3)
    line["answer_over_enc_tstar"] = round(line["answer_ms"] / w["enc_tstar"], 3)
    line["bisect_over_answer"] = round(line["bisect"]["median_ms"] / line["answer_ms"], 3)
    line["answer_cheaper_than_bisect"] = line["answer_ms"] < line["bisect"]["min_ms"]
    return line


def main():
    args = sys.argv[1:]
    out_path = take(args, "--out", None)
    reps = max(12, int(args[0])) if args else 12
    frames = {"value_noise": value_noise(4096, 4096, 1234)[:S, :S].copy(),
              "random": np.random.default_rng(7).integers(0, 256, (S, S), dtype=np.uint8)}
    lines = [json.dumps(measure(name, p, reps)) for name, p in frames.items()]
    print("\n".join(lines), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
