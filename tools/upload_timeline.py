#!/usr/bin/env python3
"""Where a frame's upload lies against the previous run's kernels, from a rocprofv3 kernel trace and memory-copy
trace of tools/c3_once.py auto N e2e (tracing only, CSV output).  A step begins at its tp_keys launch.  Prints
per step (µs, relative to the previous step's windowed search_dft start): the previous step's last search_dft and
resolve_dft_groups intervals, the frame's host-to-device copy interval, the part of the copy during which a
kernel ran (hidden), and the idle gap between the last kernel before tp_keys and tp_keys; then the medians as
one JSON line.
usage: tools/upload_timeline.py KERNEL_TRACE.csv MEMORY_COPY_TRACE.csv [skip_steps]"""
import csv
import json
import statistics
import sys


def rows(path):
    with open(path, newline="") as f:
        return list(csv.DictReader(f))


def main():
    kt, mt = rows(sys.argv[1]), rows(sys.argv[2])
    skip = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    ker = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in kt)
    # the frame uploads: host-to-device copies of at least 100 µs (the lists and tables are far shorter)
    ups = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in mt
                 if "HOST_TO_DEVICE" in r.get("Direction", "").upper()
                 and int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) >= 100_000)
    keys = [k for k in ker if k[2].startswith("tp_keys") or "::tp_keys" in k[2]]
    out = []
    for prev, cur in zip(keys, keys[1:]):
        step = [k for k in ker if prev[0] <= k[0] < cur[0]]
        search = [k for k in step if "search_dft" in k[2]]
        resolve = [k for k in step if "resolve_dft_groups" in k[2]]
        up = [u for u in ups if prev[0] < u[1] <= cur[0]]
        if not search or not resolve or not up:
            continue
        s, r, u = search[-1], resolve[-1], up[-1]
        hidden = 0
        for k in step:  # kernels of one stream: their intervals do not overlap
            hidden += max(0, min(k[1], u[1]) - max(k[0], u[0]))
        last_end = max(k[1] for k in step)
        t0 = s[0]
        out.append({"search": ((s[0] - t0) / 1e3, (s[1] - t0) / 1e3), "resolve": ((r[0] - t0) / 1e3, (r[1] - t0) / 1e3),
                    "copy": ((u[0] - t0) / 1e3, (u[1] - t0) / 1e3), "copy_us": (u[1] - u[0]) / 1e3,
                    "hidden_us": hidden / 1e3, "gap_before_tp_keys_us": (cur[0] - max(last_end, u[1])) / 1e3,
                    "idle_before_tp_keys_us": (cur[0] - last_end) / 1e3, "step_us": (cur[0] - prev[0]) / 1e3})
    out = out[skip:]
    for k, o in enumerate(out):
        print(k, {a: (tuple(round(x, 1) for x in b) if isinstance(b, tuple) else round(b, 1)) for a, b in o.items()})
    if out:
        med = {a: round(statistics.median(o[a] for o in out), 1)
               for a in ("copy_us", "hidden_us", "gap_before_tp_keys_us", "idle_before_tp_keys_us", "step_us")}
        med["hidden_share"] = round(med["hidden_us"] / med["copy_us"], 3) if med["copy_us"] else 0.0
        med["steps"] = len(out)
        print(json.dumps(med))


if __name__ == "__main__":
    main()
