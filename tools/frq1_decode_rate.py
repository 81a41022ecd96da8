#!/usr/bin/env python3
"""Decode rate of the C4 quadtree frame (2048² crop of the S1 value noise seed 1234, classifier on, levels
16/8/4, T = 4, 5 + 7 bits; one encode_quadtree(leaves=True) plus pack_frq1), max_iter = 10, in one process on
one GPU:

  A    Engine.decode(records, …) over records_from_leaves' 64-byte records, built beforehand and carrying the
       stream's dequantized contrast / brightness (so that A and B decode the same numbers): the item decoder,
       its record upload and host checks included — the only route to pixels without frac_decode_frq1
  B    Engine.decode_frq1(stream, …)
  B2   B at scale = 2 (4096²)

Where the reference's int32 sum of squared differences wraps negative at step 0, Decoder2 (and every path
here, bit for bit) stops after one iteration whatever max_iter says.  A_all and B_all repeat A and B with
rms_eps = −inf, which no rms is below, so all ten iterations run: the decoders' kernels themselves
(decode_fused, one wave per item, against frq1dec_step, a lane per four pixels).

Each path is warmed up; A and B alternate; a host clock surrounds calls that end synchronised (both return
the plane on the host).  The tool asserts that A and B return identical planes, counts and rms, and prints
one JSON line (medians and spread in ms, the leaf count per size).
usage: tools/frq1_decode_rate.py [reps] [--split D] [--out FILE]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import fractencode_amd as F  # noqa: E402
from fractencode_amd import codec  # noqa: E402
from fractencode_amd.synth import value_noise  # noqa: E402

S, SIZES, T, ITERS = 2048, (16, 4), 4, 10


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


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


def main():
    args = sys.argv[1:]
    out_path = take(args, "--out", None)
    split = float(take(args, "--split", 0.05))
    reps = max(20, int(args[0])) if args else 20
    p = value_noise(4096, 4096, 1234)[:S, :S].copy()
    with F.Engine(0, T, True) as e:
        e.set_frame(p)
        leaves, _ = e.encode_quadtree(SIZES[0], SIZES[1], split, leaves=True)
        stream = F.pack_frq1(leaves, S, S, SIZES[0], SIZES[1], T, True)
        # records_from_leaves' 64-byte records with the stream's dequantized contrast / brightness: what both
        # paths must decode for their planes to be comparable at all
        items, _ = codec.unpack_quadtree_stream(stream)
        exact = F.records_from_leaves(leaves, S)
        assert all(np.array_equal(items[k], exact[k]) for k in ("x", "y", "w", "h", "dx", "dy", "sw", "sh", "transform"))
        ninf = float("-inf")

        def path_a():
            return e.decode(items, S, S, max_iter=ITERS)

        def path_b():
            return e.decode_frq1(stream, max_iter=ITERS)

        def path_b2():
            return e.decode_frq1(stream, scale=2, max_iter=ITERS)

        def path_a_all():
            return e.decode(items, S, S, max_iter=ITERS, rms_eps=ninf)

        def path_b_all():
            return e.decode_frq1(stream, max_iter=ITERS, rms_eps=ninf)

        for fn in (path_a, path_b, path_b2, path_a_all, path_b_all):  # warm-up: buffers allocated, kernels loaded
            fn()
            fn()
        ms = {"A": [], "B": [], "B2": [], "A_all": [], "B_all": []}
        for _ in range(reps):
            ta, ra = timed(path_a)
            tb, rb = timed(path_b)
            ms["A"].append(ta)
            ms["B"].append(tb)
            assert (ra[1], ra[2]) == (rb[1], rb[2]) and np.array_equal(ra[0], rb[0]), "A and B differ"
        for _ in range(reps):
            ta, fa = timed(path_a_all)
            tb, fb = timed(path_b_all)
            ms["A_all"].append(ta)
            ms["B_all"].append(tb)
            assert (fa[1], fa[2]) == (fb[1], fb[2]) and np.array_equal(fa[0], fb[0]), "A_all and B_all differ"
        for _ in range(reps):
            ms["B2"].append(timed(path_b2)[0])
        info = F.frq1_info(stream)
    sizes, counts = np.unique(items["w"], return_counts=True)
    line = {"tool": "frq1_decode_rate", "frame": [S, S], "sizes": list(SIZES), "split_distance": split, "transforms": T,
            "max_iter": ITERS, "iterations": ra[1], "iterations_all": fa[1], "leaves": int(len(leaves)),
            "leaves_by_size": {int(a): int(b) for a, b in zip(sizes, counts)},
            "domainless_leaves": int((items["sw"] == 0).sum()), "record_bits": info["record_bits"],
            "stream_bytes": len(stream), "items_bytes": int(items.nbytes), "build_id": F.build_info()["build_id"],
            **{k: stats(v) for k, v in ms.items()}}
    line["B_not_slower_than_A"] = line["B"]["median_ms"] <= line["A"]["median_ms"]
    line["B_all_beats_A_all_beyond_spread"] = line["B_all"]["median_ms"] < line["A_all"]["min_ms"]
    text = json.dumps(line)
    print(text, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
