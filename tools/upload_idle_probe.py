#!/usr/bin/env python3
"""set_frame with the context's stream idle (nothing to overlap): host ms of set_frame alone and of
set_frame + run + sync ([min, median, max] of 30 rounds), C3 frame from pinned memory, pruned and exhaustive route.
usage: [FRAC_LIB=LIB.so] tools/upload_idle_probe.py"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fractencode_amd as F  # noqa: E402
from fractencode_amd.synth import value_noise  # noqa: E402

S = 4096
p = torch.from_numpy(value_noise(S, S, 1234)).pin_memory().numpy()
doms, rngs = F.create_uniform_grid(S, S, 16, 8), F.create_uniform_grid(S, S, 8, 8)
for name, eng in (("auto", F.ENGINE_AUTO), ("mfma", F.ENGINE_MFMA)):
    with F.Engine(0, 4, False, 0.0, -1.0, eng) as e:
        e.set_frame(p)
        e.set_domains(doms)
        e.set_ranges(rngs)
        up, tot = [], []
        for r in range(34):
            t0 = time.perf_counter()
            e.set_frame(p)
            t1 = time.perf_counter()
            e.run()
            e.sync()
            t2 = time.perf_counter()
            if r >= 4:
                up.append(1e3 * (t1 - t0))
                tot.append(1e3 * (t2 - t0))
    print(json.dumps({"lib": os.path.basename(os.environ.get("FRAC_LIB", "product")), "route": name,
                      "set_frame_ms": [round(float(np.percentile(up, q)), 4) for q in (0, 50, 100)],
                      "step_ms": [round(float(np.percentile(tot, q)), 4) for q in (0, 50, 100)]}), flush=True)
