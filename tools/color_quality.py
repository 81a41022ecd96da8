#!/usr/bin/env python3
"""Cost of steering the colour quadtree encoder by decoded RGB quality, in one process on one GPU: an RGB frame
whose channels are three value-noise planes (seeds 1234, 1235, 1236), at 512² and 2048², levels 16/8/4, T = 4,
5 + 7 bits.  Per frame, after one ColorEncoder.quadtree_rate (three full-tree searches, not timed), the quality rule
of ColorEncoder.rate_quality for a target half-way between the decoded errors of the smallest and the largest
candidate of the union, by two routes:

  device     ColorEncoder.rate_quality: per probe the three planes' rate_stream, pack_frc3 and
             Engine.decode_error_frc3 against the RGB frame that stayed on the device; three sums come back
  host_loop  the same bisection with the call that existed before: per probe the same container through
             Engine.decode_frc3 on a long-lived engine (what decode_color_stream calls, without a context per
             probe), the whole RGB frame back across PCIe, the squared error in numpy

The tool asserts that both routes give the same split distance, error and probe count.  The routes alternate
inside one loop; a host clock surrounds each call (all end synchronised).  One JSON line per frame: medians with
min–max in ms.
usage: tools/color_quality.py [reps] [--out FILE] [--sizes 512,2048]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import fractencode_amd as F  # noqa: E402
from fractencode_amd.color import ColorEncoder  # noqa: E402
from fractencode_amd.synth import value_noise  # noqa: E402

SIZES, T, SEEDS = (16, 4), 4, (1234, 1235, 1236)


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


def host_sse(dec, ref16, rw, rh):
    """Σ over the three channels of (decoded − reference)² over rw × rh from the origin, in numpy."""
    d = dec[:rh, :rw].astype(np.int16) - ref16[:rh, :rw]
    return int(np.einsum("ijk,ijk->", d, d, dtype=np.int64))


def host_bisect(enc, cands, ref16, rect, max_sse):
    """The quality rule through rate_stream + decode_frc3 + numpy → (index or None, sse, probes)."""
    made = 0

    def E(i):
        nonlocal made
        made += 1
        return host_sse(enc.engines[0].decode_frc3(enc.rate_stream(float(cands[i])))[0], ref16, *rect)

    m = len(cands)
    last = E(m - 1)
    if last <= max_sse:
        return m - 1, last, made
    first = E(0) if m > 1 else last
    if first > max_sse:
        return None, first, made
    lo, hi, best = 0, m - 1, first
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        v = E(mid)
        if v <= max_sse:
            lo, best = mid, v
        else:
            hi = mid
    return lo, best, made


def measure(S, reps):
    rgb = np.ascontiguousarray(np.stack([value_noise(S, S, seed) for seed in SEEDS], axis=-1))
    ref16 = rgb.astype(np.int16)
    g = SIZES[0]
    rect = (min(S - S % g, 2 * (S // 2 - S // 2 % g)),) * 2
    with ColorEncoder(0, transforms=T) as enc:
        enc.load(rgb)
        enc.quadtree_rate(*SIZES)
        cands = enc.rate_candidates()
        ends, _, end_bytes = enc.rate_errors([float(cands[0]), float(cands[-1])])
        target = (int(ends[0]) + int(ends[1])) // 2
        wall = {"device": [], "host_loop": []}

        def timed(k, fn):
            t0 = time.perf_counter()
            r = fn()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            return r

        dev = host = None
        agree = True
        for rep in range(reps + 2):  # the first two rounds warm up: buffers allocated, kernels loaded
            dev = timed("device", lambda: enc.rate_quality(max_sse=target))
            host = timed("host_loop", lambda: host_bisect(enc, cands, ref16, rect, target))
            agree = host[0] is not None and dev["pixels"] == rect[0] * rect[1] and \
                (float(cands[host[0]]), host[1], host[2]) == (dev["split_distance"], dev["sse"], dev["probes"])
            if not agree:
                break
        for k in wall:
            wall[k] = wall[k][2:] or wall[k]
    line = {"tool": "color_quality", "frame": "value_noise_rgb", "size": [S, S], "sizes": [16, 8, 4],
            "transforms": T, "classifier": False, "candidates": len(cands), "target_sse": target,
            "error_at_ends": [int(ends[0]), int(ends[1])], "bytes_at_ends": [int(end_bytes[0]), int(end_bytes[1])],
            "answer": dev, "host_answer": {"index": host[0], "sse": host[1], "probes": host[2]}, "agree": agree,
            "wall": {k: stats(v) for k, v in wall.items()}, "build_id": F.build_info()["build_id"]}
    w = line["wall"]
    line["host_loop_over_device"] = round(w["host_loop"]["median_ms"] / w["device"]["median_ms"], 3)
    # outside the spread: the slowest call of the device route still beats the fastest call of the host loop;
    # overlap: neither route's range lies wholly below the other's
    line["device_outside_spread"] = w["device"]["max_ms"] < w["host_loop"]["min_ms"]
    line["ranges_overlap"] = not (w["device"]["max_ms"] < w["host_loop"]["min_ms"] or
                                  w["host_loop"]["max_ms"] < w["device"]["min_ms"])
    return line


def main():
    args = sys.argv[1:]
    out_path = take(args, "--out", None)
    sizes = [int(v) for v in take(args, "--sizes", "512,2048").split(",")]
    reps = max(12, int(args[0])) if args else 12
    lines = []
    for S in sizes:
        lines.append(measure(S, reps))
        print(json.dumps(lines[-1]), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(json.dumps(line) for line in lines) + "\n")
    assert all(line["agree"] for line in lines), "the device route and the host loop disagree"


if __name__ == "__main__":
    main()
