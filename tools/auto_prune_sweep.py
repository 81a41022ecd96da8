#!/usr/bin/env python3
"""The two measurements behind FRAC_ENGINE_AUTO's pruned route, on the product library (or the
one FRAC_LIB names), one box, one process.  Within a table the configurations of a frame alternate run by run,
`--reps` (at least 10) timed runs each after 2 warm-ups; every figure is a median with its min – max.

  min   kAutoPruneMinPairs: an i.i.d. noise frame (default_rng(seed)), which always falls back, under AUTO with
        FRAC_FLAG_PRUNE (sorts, seed, windows, host turnaround, then the exhaustive search) against
        FRAC_FLAG_EXHAUSTIVE, at 1024², 2048², 4096² and 4096² with a 1/8 and a 1/4 shard of the ranges.  End to end:
        frame upload from pinned memory + run + sync, wall clock.
  budget kAutoPruneBudget: 4096² value noise blended with i.i.d. noise at several amplitudes; the tiled form
        searching its windows whatever their size (ENGINE_SEA: the kernels of AUTO's pruned route without the
        budget) against the exhaustive search.  Per frame the pair share (evaluated_mappings ÷ eligible pairs)
        and both device times (library events: prep, search, finish).
  worst the 4096² noise frame under plain AUTO (the product's routing) against FRAC_FLAG_EXHAUSTIVE, end to end.
        A library from before the flags (FRAC_LIB) runs its AUTO alone: alternate the two libraries' processes.

usage: tools/auto_prune_sweep.py [min] [budget] [worst] [--reps K] [--out FILE]   (default: all three)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fractencode_amd as F  # noqa: E402
from fractencode_amd.synth import value_noise  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("tables", nargs="*", default=["min", "budget", "worst"])
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=None)
ap.add_argument("--seed", type=int, default=42)
args = ap.parse_args()
assert args.reps >= 10, "at least 10 repetitions per configuration"

import torch  # noqa: E402  (pinned host memory for the uploads)

lines = []


def emit(row):
    row = {"lib": os.path.basename(os.environ.get("FRAC_LIB", "libfracenc.so")), "build": F.build_info()["build_id"],
           **row}
    lines.append(json.dumps(row))
    print(lines[-1], flush=True)


def mmm(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def pinned(p):
    return torch.from_numpy(np.ascontiguousarray(p)).pin_memory().numpy()


def engines(p, configs, S, shard=1):
    """One engine per configuration (engine id, flags), prepared on the frame."""
    doms, rngs = F.create_uniform_grid(S, S, 16, 8), F.create_uniform_grid(S, S, 8, 8)
    rngs = rngs[:len(rngs) // shard]
    out = {}
    for name, (eng, flags) in configs.items():
        e = F.Engine(0, 4, False, 0.0, -1.0, eng, timing=True, flags=flags)
        e.set_frame(p)
        e.set_domains(doms)
        e.set_ranges(rngs)
        out[name] = e
    return out, len(rngs), len(doms)


def alternate(es, p, reps):
    """reps rounds, each configuration once per round: wall-clock ms of upload + run + sync, and the run's
    library events."""
    wall = {k: [] for k in es}
    for r in range(reps + 2):
        for k, e in es.items():
            t0 = time.perf_counter()
            e.set_frame(p)
            e.run()
            e.sync()
            if r >= 2:
                wall[k].append(1e3 * (time.perf_counter() - t0))
    ev = {k: e.timing_history()[-reps:] for k, e in es.items()}
    st = {k: e.fetch()[1] for k, e in es.items()}
    return wall, ev, st


def noise_table(name, cases, configs):
    for S, shard in cases:
        p = pinned(np.random.default_rng(args.seed).integers(0, 256, (S, S), dtype=np.uint8))
        es, nr, nd = engines(p, configs, S, shard)
        wall, ev, st = alternate(es, p, args.reps)
        row = {"table": name, "size": S, "shard": shard, "ranges": nr, "domains": nd,
               "block_tile_pairs": ((nr + 31) // 32) * ((nd + 31) // 32)}
        for k in es:
            row[k] = {"e2e_ms": mmm(wall[k]), "device_ms": mmm(ev[k]["ms_device"]),
                      "form": F.FORM_NAMES[st[k]["search_form"]]}
            es[k].close()
        if len(es) == 2:
            a, b = list(es)
            row[f"{b}_over_{a}"] = round(row[b]["e2e_ms"]["median"] / row[a]["e2e_ms"]["median"], 4)
        emit(row)


if "min" in args.tables:
    noise_table("min_pairs", [(1024, 1), (2048, 1), (4096, 8), (4096, 4), (4096, 1)],
                {"exhaustive": (F.ENGINE_AUTO, F.FLAG_EXHAUSTIVE), "forced_fallback": (F.ENGINE_AUTO, F.FLAG_PRUNE)})

if "worst" in args.tables:
    configs = {"exhaustive": (F.ENGINE_AUTO, F.FLAG_EXHAUSTIVE), "auto": (F.ENGINE_AUTO, 0)}
    try:
        F.Engine(0, 4, False, 0.0, -1.0, F.ENGINE_AUTO, flags=F.FLAG_EXHAUSTIVE).close()
    except Exception:  # a library from before the flags (FRAC_LIB): its AUTO alone, for a run-by-run A/B
        del configs["exhaustive"]
    noise_table("worst_case", [(4096, 1)], configs)

if "budget" in args.tables:
    S = 4096
    base = value_noise(S, S, 1234).astype(np.int32)
    iid = np.random.default_rng(args.seed).integers(0, 256, (S, S), dtype=np.uint8).astype(np.int32)
    for amp in (0, 8, 16, 32, 64, 96, 128, 192, 256):
        # amp = 256: the noise alone; below, the value noise plus the noise scaled to ±amp/2
        p = iid if amp == 256 else np.clip(base + ((iid - 128) * amp) // 256, 0, 255)
        p = pinned(p.astype(np.uint8))
        es, nr, nd = engines(p, {"exhaustive": (F.ENGINE_AUTO, F.FLAG_EXHAUSTIVE), "windows": (F.ENGINE_SEA, 0)}, S)
        wall, ev, st = alternate(es, p, args.reps)
        row = {"table": "budget", "size": S, "noise_amplitude": amp,
               "pair_share": round(st["windows"]["evaluated_mappings"] / (nr * nd), 5)}
        for k in es:
            # the SEA engine's second boundary follows its resolve: search + finish is the comparable span
            sf = ev[k]["ms_search"] + ev[k]["ms_finish"]
            row[k] = {"search_finish_ms": mmm(sf), "prep_ms": mmm(ev[k]["ms_prep"]), "device_ms": mmm(ev[k]["ms_device"]),
                      "e2e_ms": mmm(wall[k])}
            es[k].close()
        row["windows_over_exhaustive_search_finish"] = round(
            row["windows"]["search_finish_ms"]["median"] / row["exhaustive"]["search_finish_ms"]["median"], 4)
        emit(row)

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
