#!/usr/bin/env python3
"""Decode rate of the C3 stream (4096² S1 value noise seed 1234, 8×8 ranges, T = 4, 5 + 7 bits; one
search plus pack_frc1), max_iter = 10, in one process on one GPU:

  A    Engine.decode(items, …) with the items unpacked beforehand: the item decoder, its 16 MiB
       record upload included
  A'   codec.unpack_stream + A: the only way from a stream to pixels without frac_decode_frc1
  B    Engine.decode_frc1(stream, …)
  B2   B at scale = 2 (8192²)

At 4096² the reference's int32 sum of squared differences wraps negative at step 0, so Decoder2 (and
every path here, bit for bit) stops after one iteration whatever max_iter says: the four paths above
time one iteration.  A_all and B_all repeat A and B with rms_eps = −inf, which no rms is below, so all
ten iterations run: the decoders' kernels themselves.

Each path is warmed up; A and B alternate; a host clock surrounds calls that end synchronised (both
return the plane on the host).  The tool asserts that A and B return identical planes and counts, and
prints one JSON line (medians and spread in ms).  usage: tools/frc1_decode_rate.py [reps] [--out FILE]"""
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

S, N, T, ITERS = 4096, 8, 4, 10


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3),
            "p10_ms": round(ms[len(ms) // 10], 3), "p90_ms": round(ms[(len(ms) * 9) // 10], 3), "n": len(ms)}


def main():
    args = sys.argv[1:]
    out_path = None
    if "--out" in args:
        k = args.index("--out")
        out_path = args[k + 1]
        del args[k:k + 2]
    reps = max(20, int(args[0])) if args else 20
    p = value_noise(S, S, 1234)
    with F.Engine(0, T) as e:
        e.set_frame(p)
        e.set_domains(F.create_uniform_grid(S, S, 2 * N, N))
        e.search(F.create_uniform_grid(S, S, N, N))
        stream = e.pack_frc1()
        items, _ = codec.unpack_stream(stream)

        def path_a():
            return e.decode(items, S, S, max_iter=ITERS)

        def path_a_prime():
            return e.decode(codec.unpack_stream(stream)[0], S, S, max_iter=ITERS)

        def path_b():
            return e.decode_frc1(stream, max_iter=ITERS)

        def path_b2():
            return e.decode_frc1(stream, scale=2, max_iter=ITERS)

        def path_a_all():
            return e.decode(items, S, S, max_iter=ITERS, rms_eps=float("-inf"))

        def path_b_all():
            return e.decode_frc1(stream, max_iter=ITERS, rms_eps=float("-inf"))

        for fn in (path_a, path_b, path_b2, path_a_all, path_b_all):  # warm-up: buffers allocated, kernels loaded
            fn()
            fn()
        ms = {"A": [], "A_prime": [], "B": [], "B2": [], "A_all": [], "B_all": []}
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
        for _ in range(5):
            ms["A_prime"].append(timed(path_a_prime)[0])
        for _ in range(reps):
            ms["B2"].append(timed(path_b2)[0])
        info = F.frc1_info(stream)
    line = {"tool": "frc1_decode_rate", "frame": [S, S], "range_size": N, "transforms": T, "max_iter": ITERS,
            "iterations": ra[1], "iterations_all": fa[1], "record_bits": info["record_bits"], "stream_bytes": len(stream),
            "items_bytes": int(items.nbytes), "build_id": F.build_info()["build_id"],
            **{k: stats(v) for k, v in ms.items()}}
    line["B_not_slower_than_A"] = line["B"]["median_ms"] <= line["A"]["median_ms"]
    text = json.dumps(line)
    print(text, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
