#!/usr/bin/env python3
"""Decode rate of an inter-coded frame, and what P frames buy on synthetic frames, in one process on one GPU.

Rate.  Two consecutive frames of a pan over the S1 value noise (seed 1234; frame k is the 2048² crop at (8k, 4k),
3k brighter), quadtree 16/8/4, T = 4, 5 + 7 bits.  Frame 0 is coded as an I frame and decoded; frame 1 is coded as
a P frame against that reconstruction (set_planes on the device, encode_quadtree_stream).  Of the P stream:

  inter_dev    Engine.decode_inter, device reference to device plane (the call returns synchronised)
  inter_host   Engine.decode_inter through the host (reference up, plane down)
  frq1         Engine.decode_frq1 of the same bytes: the iterative decoder, the same per-pass work N times
               (its iteration count is reported; the reference's int32 rms sum may end it early)
  frq1_1 / frq1_10   the same with rms_eps = −inf at max_iter 1 and 10: (frq1_10 − frq1_1) / 9 is one iteration of
               frq1dec_step with its check, free of the call's fixed costs
  copy         a device-to-device copy of one plane (torch), synchronised per call: the floor of a call that reads
               and writes W·H bytes; copy_x100 / 100 is the same without the per-call latency
  err_dev      Engine.inter_error (compared in registers, two scalars come back)
  err_host     the same number through the host: decode_inter on the device, the plane copied down, numpy's sum

The paths alternate; a host clock surrounds calls that end synchronised.  inter_dev and inter_host must return the
same plane, err_dev and err_host the same sum.

Quality.  Six frames of the same pan at 1024², once all-I (gop = 1) and once I + 5 P (gop = 6), one split distance:
bytes and PSNR of the reconstruction per frame.

Prints one JSON line.  --kernels: a short run (3 calls per path, no quality part) for a kernel trace.
usage: tools/inter_decode_rate.py [reps] [--split D] [--out FILE] [--kernels]"""
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
QS, QFRAMES = 1024, 6


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


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


def pan(noise, k, size):
    crop = noise[4 * k:4 * k + size, 8 * k:8 * k + size].astype(np.int32) + 3 * k
    return np.clip(crop, 0, 255).astype(np.uint8)


def psnr(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    return F._psnr(int((d * d).sum()), a.size)


def sequence(noise, split, gop):
    out = []
    with F.SequenceEncoder(transforms=T, max_size=SIZES[0], min_size=SIZES[1], split_distance=split, gop=gop) as enc:
        for k in range(QFRAMES):
            f = pan(noise, k, QS)
            kind, s = enc.push(f)
            out.append({"kind": kind, "bytes": len(s), "psnr": round(psnr(enc.reconstruction().cpu().numpy(), f), 3)})
    return out


def main():
    args = sys.argv[1:]
    out_path = take(args, "--out", None)
    split = float(take(args, "--split", 10.0))
    kernels = "--kernels" in args
    if kernels:
        args.remove("--kernels")
    reps = 3 if kernels else (max(8, int(args[0])) if args else 20)
    noise = value_noise(4096, 4096, 1234)
    f0, f1 = pan(noise, 0, S), pan(noise, 1, S)
    dev = torch.device("cuda", 0)
    with F.Engine(0, T) as e:
        e.set_frame(f0)
        istream, _ = e.encode_quadtree_stream(SIZES[0], SIZES[1], split)
        rec0 = e.decode_frq1(istream)[0]
        d_rec0, d_f1 = torch.from_numpy(rec0).to(dev), torch.from_numpy(f1).to(dev)
        e.set_planes(d_rec0, d_f1)
        pstream, _ = e.encode_quadtree_stream(SIZES[0], SIZES[1], split, host_pack=False)
        d_out, d_copy = torch.empty_like(d_rec0), torch.empty_like(d_rec0)
        ninf = float("-inf")

        def copy_once():
            d_copy.copy_(d_rec0)
            torch.cuda.synchronize()

        def copy_x100():
            for _ in range(100):
                d_copy.copy_(d_rec0)
            torch.cuda.synchronize()

        def err_host():
            p = e.decode_inter(pstream, d_rec0, out=d_out).cpu().numpy()
            d = p.astype(np.int64) - f1.astype(np.int64)
            return int((d * d).sum())

        paths = {
            "inter_dev": lambda: e.decode_inter(pstream, d_rec0, out=d_out),
            "inter_host": lambda: e.decode_inter(pstream, rec0),
            "frq1": lambda: e.decode_frq1(pstream),
            "frq1_1": lambda: e.decode_frq1(pstream, max_iter=1, rms_eps=ninf),
            "frq1_10": lambda: e.decode_frq1(pstream, max_iter=10, rms_eps=ninf),
            "copy": copy_once,
            "copy_x100": copy_x100,
            "err_dev": lambda: e.inter_error(pstream),
            "err_host": err_host,
        }
        for fn in paths.values():  # warm-up: buffers allocated, kernels loaded
            fn()
            fn()
        ms = {k: [] for k in paths}
        last = {}
        for _ in range(reps):
            for k, fn in paths.items():
                t, last[k] = timed(fn)
                ms[k].append(t)
        assert np.array_equal(last["inter_dev"].cpu().numpy(), last["inter_host"]), "the two variants differ"
        assert last["err_dev"]["sse"] == last["err_host"], "inter_error differs from the host's sum"
        info = F.frq1_info(pstream)
    med = {k: statistics.median(v) for k, v in ms.items()}
    line = {"tool": "inter_decode_rate", "frame": [S, S], "sizes": list(SIZES), "split_distance": split, "transforms": T,
            "i_stream_bytes": len(istream), "p_stream_bytes": len(pstream), "p_leaves": info["n_leaves"],
            "i_psnr": round(psnr(rec0, f0), 3), "p_psnr": round(last["err_dev"]["psnr"], 3),
            "frq1_iterations": last["frq1"][1], "build_id": F.build_info()["build_id"],
            **{k: stats(v) for k, v in ms.items()},
            "frq1_step_ms": round((med["frq1_10"] - med["frq1_1"]) / 9.0, 4),
            "copy_each_ms": round(med["copy_x100"] / 100.0, 4),
            "frq1_over_inter_dev": round(med["frq1"] / med["inter_dev"], 2)}
    if not kernels:
        qnoise = noise[:QS + 4 * QFRAMES, :QS + 8 * QFRAMES]
        line["sequence"] = {"frame": [QS, QS], "frames": QFRAMES, "all_I": sequence(qnoise, split, 1),
                            "I_P": sequence(qnoise, split, QFRAMES)}
    text = json.dumps(line)
    print(text, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
