#!/usr/bin/env python3
"""What the tuple sink costs the finish phase, by route and by where the sink lies: the C3 frame (4096² S1
value noise, 8×8 ranges, 16×16 domains stride 8, T = 4) under FRAC_ENGINE_AUTO (the pruned route: the sorted
resolve) and under AUTO | FRAC_FLAG_EXHAUSTIVE (the slot walk of the exhaustive Fourier search), with no sink, a
device sink and a pinned host sink.  Per combination one JSON line: ms_finish from the library's own events
(timing_history), median and min–max over `runs` runs after `warmup` warm-ups, with the library's build id.
It only measures; an A/B of two builds is this program run once per library (FRAC_LIB), alternating.
usage: tools/sink_probe.py [runs] [warmup]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fractencode_amd as F  # noqa: E402
from fractencode_amd.synth import value_noise  # noqa: E402

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 20
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 5
S = 4096

import torch  # noqa: E402

p = value_noise(S, S, 1234)
rngs = F.create_uniform_grid(S, S, 8, 8)
doms = F.create_uniform_grid(S, S, 16, 8)
nbytes = len(rngs) * F.TUPLE.itemsize
sinks = {"none": None,
         "device": torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0"),
         "pinned": torch.zeros(nbytes, dtype=torch.uint8).pin_memory()}
build = F.build_info()
for route, flags in (("auto", 0), ("exhaustive", F.FLAG_EXHAUSTIVE)):
    with F.Engine(0, 4, False, 0.0, -1.0, F.ENGINE_AUTO, timing=True, flags=flags) as e:
        e.set_frame(p)
        e.set_domains(doms)
        e.set_ranges(rngs)
        for kind, buf in sinks.items():
            e.set_tuple_sink(buf.data_ptr() if buf is not None else None)
            for _ in range(warmup):
                e.run()
            e.sync()
            e.timing_history()
            for _ in range(runs):
                e.run()
            e.sync()
            h = e.timing_history()
            _, st = e.fetch()
            fin = np.asarray(h["ms_finish"])
            print(json.dumps({
                "route": route, "sink": kind, "form": F.FORM_NAMES[st["search_form"]], "runs": len(fin),
                "ms_finish": {"median": round(float(np.median(fin)), 4), "min": round(float(fin.min()), 4),
                              "max": round(float(fin.max()), 4)},
                "ms_search_median": round(float(np.median(h["ms_search"])), 4),
                "ms_device_median": round(float(np.median(h["ms_device"])), 4),
                "build_id": build.get("build_id"), "lib": os.path.relpath(F.LIB_PATH, ROOT)}), flush=True)
        e.set_tuple_sink(None)
