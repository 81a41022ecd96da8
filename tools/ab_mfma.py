#!/usr/bin/env python3
"""Interleaved in-process A/B of MFMA search variants on the C3 frame; prints per-variant
median/min search-kernel and finish (resolve + fit) ms (library HIP events).
Variants: "d" = the C4-Fourier search as shipped (FRAC_MFMA_DFT=1; variant 35, also "fub"), "ft" = the same
always carrying the winning chunk's tile mask (37), "d6" = its exact epilogue (21, the A/B of the guard),
"fM" / "fV" / "fB" / "f0" = the ablations of 35 (240 – 243: MFMAs with a one-value epilogue, the epilogue
without MFMAs, no barrier, no LDS-DMA / barrier; wrong results by design), an integer v = the direct
search_mfma with FRAC_MFMA_VARIANT=v (FRAC_MFMA_DFT=0).  The search forms retired since (DESIGN §7.2,
Appendix A) ran under letters this table no longer has.
Ablation variants need the tuning library: python tools/build_tuning.py, then
FRAC_LIB=fractencode_amd/libfracenc_tuning.so tools/ab_mfma.py ...
usage: tools/ab_mfma.py d,2 [rounds]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fractencode_amd as F  # noqa: E402
from fractencode_amd.synth import value_noise  # noqa: E402

variants = sys.argv[1].split(",") if len(sys.argv) > 1 else ["d", "2"]
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
S = int(os.environ.get("AB_SIZE", "4096"))
REPS = int(os.environ.get("AB_REPS", "1"))
p = value_noise(S, S, 1234)
ref = None
with F.Engine(0, 4, False, 0.0, -1.0, F.ENGINE_MFMA, timing=True) as e:
    e.set_frame(p)
    e.set_domains(F.create_uniform_grid(S, S, 16, 8))
    e.set_ranges(F.create_uniform_grid(S, S, 8, 8))
    res = {v: [] for v in variants}
    fin = {v: [] for v in variants}
    for r in range(rounds + 1):
        for v in variants:
            os.environ["FRAC_MFMA_DFT"] = "1" if not v.isdigit() else "0"
            os.environ["FRAC_MFMA_VARIANT"] = {"d": "35", "fub": "35", "ft": "37", "d6": "21", "fM": "240", "fV": "241",
                                              "fB": "242", "f0": "243"}.get(v, v)
            for _ in range(REPS):  # back-to-back runs: the last one is timed (the clock settles under load)
                e.run()
            out, st = e.fetch()
            if ref is None:
                ref = out.tobytes()
            if v in ("d", "fub", "ft", "d6") or (v.isdigit() and (int(v) < 8 or int(v) in (32, 64, 96, 98, 128, 130))):  # 8, 16 are ablations (results intentionally wrong)
                assert out.tobytes() == ref, f"variant {v} differs"
            if r:
                res[v].append(st["ms_search"])
                fin[v].append(st["ms_finish"])
    for v in variants:
        a = np.array(res[v])
        print(f"variant {v}: search median {np.median(a):.3f} ms  min {a.min():.3f} ms  finish median "
              f"{np.median(fin[v]):.3f} ms  (n={len(a)})", flush=True)
