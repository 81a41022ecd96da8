#!/usr/bin/env python3
"""Cost of steering the quadtree encoder by decoded quality at the C4 configuration (2048², classifier on, levels
16/8/4, T = 4, 5 + 7 bits), in one process on one GPU, on two frames: the 2048² crop of the S1 value noise (seed
1234) and uniform random noise (seed 7).  Per frame, after one Engine.quadtree_rate:

  quality      Engine.rate_quality for a target half-way between the decoded errors of the smallest and the
               largest candidate: the stated bisection (include/fracenc.h) with every probe's stream packed,
               decoded and compared on the device
  host_loop    the same bisection on the host through the calls that existed before: per probe rate_stream,
               decode_frq1 (the plane comes back, 4 MiB) and the squared error in numpy.  Its candidates are the
               tree's split keys, from the upper levels' distances searched with Engine.search (set-up, not timed)
  error        one Engine.decode_error of the answer's stream
  host_error   decode_frq1 of that stream plus the numpy sum

The tool asserts that both bisections give the same split distance, error and probe count, and that decode_error
equals the host's sum.  The two routes alternate inside one loop; a host clock surrounds each call (all end
synchronised).  One JSON line per frame: medians with min–max in ms.
usage: tools/quadtree_quality.py [reps] [--out FILE] [--size S]"""
import json
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


def candidates(plane, max_size, min_size, transforms=T, classifier=True):
    """The rate state's candidates {0.0} ∪ {e(v)}, e(v) = min(d(v), e(parent(v))), ascending and distinct, from
    the distances of the levels above min_size: each level's nodes (level 0 the max_size grid, row-major; below
    it every node's quadrants TL, TR, BL, BR) searched against createUniformGrid(2n, n) with Engine.search."""
    H, W = plane.shape
    keys, e_prev = [np.zeros(1)], None
    nodes = F.create_uniform_grid(W, H, max_size, max_size)
    n = max_size
    with F.Engine(0, transforms, classifier) as e:
        e.set_frame(plane)
        while n > min_size and len(nodes):
            e.set_domains(F.create_uniform_grid(W, H, 2 * n, n))
            d = e.search(nodes)[0]["distance"].astype(np.float64)
            e_prev = d if e_prev is None else np.minimum(d, np.repeat(e_prev, 4))
            keys.append(e_prev)
            h = n // 2
            nxt = np.zeros(4 * len(nodes), dtype=F.GRID_ITEM)
            for q, (qx, qy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
                nxt["x"][q::4], nxt["y"][q::4] = nodes["x"] + qx * h, nodes["y"] + qy * h
            nxt["w"] = nxt["h"] = h
            nxt["category"] = -1
            nodes, n = nxt, h
    return np.unique(np.concatenate(keys))


def host_sse(plane, frame32, g):
    """Σ(decoded − frame)² over the rectangle the g × g grid covers, in numpy."""
    H, W = plane.shape
    ch, cw = H - H % g, W - W % g
    d = plane[:ch, :cw].astype(np.int32) - frame32[:ch, :cw]
    return int(np.einsum("ij,ij->", d, d, dtype=np.int64))


def host_bisect(e, cands, frame32, max_sse):
    """frac_quadtree_rate_quality's rule through rate_stream + decode_frq1 + numpy → (index or None, sse, probes)."""
    made = 0

    def E(i):
        nonlocal made
        made += 1
        return host_sse(e.decode_frq1(e.rate_stream(float(cands[i])))[0], frame32, SIZES[0])

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


def measure(name, plane, reps):
    S = plane.shape[0]
    cands = candidates(plane, *SIZES)
    frame32 = plane.astype(np.int32)
    with F.Engine(0, T, True) as e:
        e.set_frame(plane)
        e.quadtree_rate(*SIZES)
        ends, end_bytes, _ = e.rate_errors([float(cands[0]), float(cands[-1])])
        target = (int(ends[0]) + int(ends[1])) // 2
        wall = {k: [] for k in ("quality", "host_loop", "error", "host_error")}

        def timed(k, fn):
            t0 = time.perf_counter()
            r = fn()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            return r

        dev = host = None
        for rep in range(reps + 2):  # the first two rounds warm up: buffers allocated, kernels loaded
            dev = timed("quality", lambda: e.rate_quality(max_sse=target))
            host = timed("host_loop", lambda: host_bisect(e, cands, frame32, target))
            stream = e.rate_stream(dev[0])
            err = timed("error", lambda: e.decode_error(stream))
            herr = timed("host_error", lambda: host_sse(e.decode_frq1(stream)[0], frame32, SIZES[0]))
            agree = host[0] is not None and (float(cands[host[0]]), host[1], host[2]) == (dev[0], dev[3], dev[4]) \
                and err["sse"] == herr == dev[3] and len(stream) == dev[1]
            if not agree:
                break
        for k in wall:
            wall[k] = wall[k][2:] or wall[k]
    t, size, leaves, sse, probes = dev
    line = {"tool": "quadtree_quality", "frame": name, "size": [S, S], "sizes": [16, 8, 4], "transforms": T,
            "classifier": True, "candidates": len(cands), "target_sse": target,
            "error_at_ends": [int(ends[0]), int(ends[1])], "bytes_at_ends": [int(end_bytes[0]), int(end_bytes[1])],
            "answer": {"split_distance": t, "bytes": size, "leaves": leaves, "sse": sse, "psnr": err["psnr"],
                       "probes": probes, "decode_iterations": err["iterations"]},
            "host_answer": {"index": host[0], "sse": host[1], "probes": host[2]}, "agree": agree,
            "wall": {k: stats(v) for k, v in wall.items()}, "build_id": F.build_info()["build_id"]}
    w = line["wall"]
    line["host_loop_over_quality"] = round(w["host_loop"]["median_ms"] / w["quality"]["median_ms"], 3)
    line["host_error_over_error"] = round(w["host_error"]["median_ms"] / w["error"]["median_ms"], 3)
    # outside the spread: the slower call of the device route still beats the faster call of the host loop
    line["quality_outside_spread"] = w["quality"]["max_ms"] < w["host_loop"]["min_ms"]
    line["error_outside_spread"] = w["error"]["max_ms"] < w["host_error"]["min_ms"]
    return line


def main():
    args = sys.argv[1:]
    out_path = take(args, "--out", None)
    S = int(take(args, "--size", 2048))
    reps = max(12, int(args[0])) if args else 12
    frames = {"value_noise": value_noise(4096, 4096, 1234)[:S, :S].copy(),
              "random": np.random.default_rng(7).integers(0, 256, (S, S), dtype=np.uint8)}
    lines = [measure(name, p, reps) for name, p in frames.items()]
    text = "\n".join(json.dumps(line) for line in lines)
    print(text, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    assert all(line["agree"] for line in lines), "the device fit and the host loop disagree"


if __name__ == "__main__":
    main()
