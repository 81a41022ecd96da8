#!/usr/bin/env python3
"""Cost of turning a quadtree partition into FRQ1 bytes, on the host and on the device, at the C4 configuration
(2048², classifier on, levels 16/8/4, T = 4, 5 + 7 bits), in one process on one GPU, on the two frames of
tools/quadtree_rate.py: the 2048² crop of the S1 value noise (seed 1234) and uniform random bytes (seed 7).  The
budget is half-way between the smallest and the largest stream, t* the fit's split distance.  Per frame:

  a_emit       Engine.rate_leaves(t*) into pinned memory (the leaves cross PCIe, 32 bytes each)
  a_pack       pack_frq1 of those leaves: the host packer on its own
  a            the two together: today's answer-to-bytes
  b            Engine.rate_stream(t*): the same bytes laid out, quantized and packed on the device
  c_enc        encode_quadtree(leaves=True) at t*
  c_pack       pack_frq1 of those leaves
  c            the two together: encode_quadtree_stream(host_pack=True)'s two steps
  d            encode_quadtree_stream(host_pack=False) at t* (frac_encode_quadtree_stream)
  e_host       encode_quadtree_to_size(budget, host_pack=True)
  e_dev        encode_quadtree_to_size(budget, host_pack=False)

Every path is warmed up; the paths of a repetition run back to back; a host clock surrounds calls that end
synchronised.  Every repetition asserts that the streams of a and b, of c and d, and of e_host and e_dev are
equal.  One JSON line per frame: median, min and max in ms, the PCIe bytes per route (32 × leaves against the
stream's size), per pair whether the device route's max is below the host route's min, and (x_minus_y) the host
route's time minus the device route's within each repetition.
usage: tools/frq1_pack_rate.py [reps] [--out FILE]"""
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
            "n": len(ms)}


def take(args, flag, default):
    if flag not in args:
        return default
    k = args.index(flag)
    v = args[k + 1]
    del args[k:k + 2]
    return v


def measure(name, plane, reps):
    cap = (S // SIZES[1]) ** 2
    pinned = torch.zeros(cap * F.QT_LEAF.itemsize, dtype=torch.uint8).pin_memory().numpy().view(F.QT_LEAF)
    wall = {k: [] for k in ("a_emit", "a_pack", "a", "b", "c_enc", "c_pack", "c", "d", "e_host", "e_dev",
                            "a_minus_b", "c_minus_d", "e_host_minus_e_dev")}

    def timed(k, fn):
        t0 = time.perf_counter()
        r = fn()
        wall[k].append((time.perf_counter() - t0) * 1e3)
        return r

    def pack(leaves):
        return F.pack_frq1(leaves, S, S, SIZES[0], SIZES[1], T, True)

    with F.Engine(0, T, True) as e:
        e.set_frame(plane)
        e.quadtree_rate(*SIZES)
        ends, _, _ = e.rate_sizes([-1.0, np.inf])
        budget = int(ends[0] + ends[1]) // 2
        tstar, fit_bytes, fit_leaves = e.rate_fit(budget)

        def rep():
            e.quadtree_rate(*SIZES)  # the readers need the state, which every encode ends
            leaves = timed("a_emit", lambda: e.rate_leaves(tstar, out=pinned))
            a = timed("a_pack", lambda: pack(leaves))
            wall["a"].append(wall["a_emit"][-1] + wall["a_pack"][-1])
            b = timed("b", lambda: e.rate_stream(tstar))
            assert a == b, "rate_stream differs from pack_frq1(rate_leaves)"
            leaves = timed("c_enc", lambda: e.encode_quadtree(SIZES[0], SIZES[1], tstar, out=pinned, leaves=True)[0])
            c = timed("c_pack", lambda: pack(leaves))
            wall["c"].append(wall["c_enc"][-1] + wall["c_pack"][-1])
            d = timed("d", lambda: e.encode_quadtree_stream(SIZES[0], SIZES[1], tstar, host_pack=False)[0])
            assert c == d == a, "encode_quadtree_stream differs from pack_frq1(encode_quadtree leaves)"
            eh = timed("e_host", lambda: e.encode_quadtree_to_size(budget, *SIZES, host_pack=True)[0])
            ed = timed("e_dev", lambda: e.encode_quadtree_to_size(budget, *SIZES, host_pack=False)[0])
            assert eh == ed == a, "encode_quadtree_to_size: the two routes differ"
            for host, dev in (("a", "b"), ("c", "d"), ("e_host", "e_dev")):  # the gain within this repetition
                wall[f"{host}_minus_{dev}"].append(wall[host][-1] - wall[dev][-1])
            return a

        for _ in range(3):  # warm-up: buffers allocated, kernels loaded
            rep()
        for k in wall:
            wall[k].clear()
        for _ in range(reps):
            stream = rep()
    assert len(stream) == fit_bytes <= budget
    w = {k: stats(v) for k, v in wall.items()}
    below = lambda dev, host: w[dev]["max_ms"] < w[host]["min_ms"]  # noqa: E731
    return {"tool": "frq1_pack_rate", "frame": name, "size": [S, S], "sizes": [16, 8, 4], "transforms": T,
            "classifier": True, "bits": [5, 7], "budget_bytes": budget, "split_distance": tstar,
            "leaves": fit_leaves, "stream_bytes": fit_bytes, "pcie_bytes_host_route": 32 * fit_leaves,
            "pcie_bytes_device_route": fit_bytes, "wall": w,
            "device_below_host": {"b_vs_a": below("b", "a"), "d_vs_c": below("d", "c"),
                                  "e_dev_vs_e_host": below("e_dev", "e_host")},
            "equal_streams_every_rep": True, "build_id": F.build_info()["build_id"]}


def main():
    args = sys.argv[1:]
    out_path = take(args, "--out", None)
    reps = max(18, int(args[0])) if args else 18
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
