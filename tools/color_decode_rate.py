#!/usr/bin/env python3
"""Colour decode rate at C5's geometry (4096² RGB, value noise seeds 1234..1236; 8×8 ranges, 16×16 domains,
T = 4, 5 + 7 bits): one colour encode plus pack_frc3, then, in one process on one GPU, max_iter = 10:

  a  Engine.decode_frc3(container): the three planes decoded and converted on the device, 3 B/px downloaded
  a_dev  the same into a CUDA tensor (frac_decode_frc3_device): nothing downloaded, so a − a_dev is the RGB's way
     to a fresh host array
  b  the three single-plane Engine.decode_frc1 calls on the same engine (unchanged code: the baseline),
     their sum; 1.5 B/px downloaded, no RGB
  c  the yuv2rgb fast-path kernel alone on the decoded-size planes already in HBM: device events around
     BATCH launches on the engine's stream, per launch
  d  the existing rgb2yuv fast-path kernel on the same frame the same way: it moves the same 4.5 B/px the other
     way and is the comparison kernel

a, a_dev and b alternate, c and d alternate; every path is warmed up; a host clock surrounds a, a_dev and b, which
end synchronised.  a and b return fresh host arrays (48 and 24 MiB), as the API does: their first touch is part
of the call.  At these sizes the reference's int32 sum of squared differences can wrap (tools/frc1_decode_rate.py),
so a plane may stop before max_iter; the line carries the three iteration counts, and the tool asserts that a
and b report the same ones, and that a's pixels are the host conversion's of b's planes on a sample of rows.  It
prints one JSON line (medians and spread).
usage: tools/color_decode_rate.py [reps] [--out FILE] [--size S]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import fractencode_amd as F  # noqa: E402
from fractencode_amd.color import ColorEncoder  # noqa: E402
from fractencode_amd.synth import value_noise  # noqa: E402

N, T, ITERS, BATCH = 8, 4, 10, 20


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4),
            "p10_ms": round(ms[len(ms) // 10], 4), "p90_ms": round(ms[(len(ms) * 9) // 10], 4), "n": len(ms)}


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    import torch

    args = sys.argv[1:]
    out_path, S = None, 4096
    for flag in ("--out", "--size"):
        if flag in args:
            k = args.index(flag)
            if flag == "--out":
                out_path = args[k + 1]
            else:
                S = int(args[k + 1])
            del args[k:k + 2]
    reps = max(20, int(args[0])) if args else 20
    rgb = np.stack([value_noise(S, S, 1234 + k) for k in range(3)], -1)
    with ColorEncoder(0, N, 2 * N, T) as enc:
        enc.load(rgb)
        enc.run()
        enc.sync()
        planes = [e.pack_frc1() for e in enc.engines]
        container = enc.pack_frc3()

    ts = torch.cuda.Stream()
    with F.Engine(0, T) as e:
        def path_a():
            return e.decode_frc3(container, max_iter=ITERS)

        def path_b():
            return [e.decode_frc1(s, max_iter=ITERS) for s in planes]

        dev_out = torch.empty((S, S, 3), dtype=torch.uint8, device="cuda")

        def path_a_dev():
            return e.decode_frc3(container, max_iter=ITERS, out=dev_out)

        for fn in (path_a, path_a_dev, path_b):  # warm-up: buffers allocated, kernels loaded
            fn()
            fn()
        ms = {"a_decode_frc3": [], "a_dev_decode_frc3_device": [], "b_three_decode_frc1": []}
        for _ in range(reps):
            ta, ra = timed(path_a)
            td, rd = timed(path_a_dev)
            tb, rb = timed(path_b)
            ms["a_decode_frc3"].append(ta)
            ms["a_dev_decode_frc3_device"].append(td)
            ms["b_three_decode_frc1"].append(tb)
        assert rd[1] == ra[1] and np.array_equal(rd[0].cpu().numpy(), ra[0]), "the device variant's pixels differ"
        assert ra[1] == [r[1] for r in rb] and ra[2] == [r[2] for r in rb], "a and b report different iterations / rms"
        # a's pixels against b's planes: R of a sample of rows through the fused form in long double
        y, u, v = (r[0] for r in rb)
        rows = np.arange(0, S, max(S // 64, 1))
        L = np.longdouble
        vp = v[rows // 2][:, np.arange(S) // 2].astype(L) - L(128)
        red = (L(1.402) * vp + y[rows].astype(L)).astype(np.float64)
        red = np.where(red < 0, 0, np.where(red > 255, 255, np.trunc(np.clip(red, 0, 255)))).astype(np.uint8)
        assert np.array_equal(ra[0][rows][:, :, 0], red), "decode_frc3's pixels are not the conversion of the planes"

        # c / d: the two conversion kernels alone, planes and frame in HBM, on a torch stream the engine shares
        e.set_stream(ts.cuda_stream)
        ty, tu, tv = (torch.from_numpy(p).cuda() for p in (y, u, v))
        trgb = torch.from_numpy(rgb).cuda()
        orgb = torch.empty_like(trgb)
        oy, ou, ov = torch.empty_like(ty), torch.empty_like(tu), torch.empty_like(tv)
        torch.cuda.synchronize()
        L_ = F.lib()
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

        def kern_c():
            rc = L_.frac_yuv_to_rgb_device(e._ctx, p(ty), S, S, S, p(tu), S // 2, p(tv), S // 2, p(orgb), 3 * S)
            assert rc == 0, F.last_error(e._ctx)

        def kern_d():
            rc = L_.frac_rgb_to_yuv_device(e._ctx, p(trgb), S, S, 3 * S, p(oy), S, p(ou), S // 2, p(ov), S // 2)
            assert rc == 0, F.last_error(e._ctx)

        def batch(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(ts)
            for _ in range(BATCH):
                fn()
            b.record(ts)
            b.synchronize()
            return a.elapsed_time(b) / BATCH

        for fn in (kern_c, kern_d):
            batch(fn)
        ms["c_yuv2rgb_kernel"], ms["d_rgb2yuv_kernel"] = [], []
        for _ in range(reps):
            ms["c_yuv2rgb_kernel"].append(batch(kern_c))
            ms["d_rgb2yuv_kernel"].append(batch(kern_d))
        e.sync()
        e.set_stream(None)
    line = {"tool": "color_decode_rate", "frame": [S, S], "range_size": N, "transforms": T, "max_iter": ITERS,
            "iterations": ra[1], "container_bytes": len(container), "kernel_batch": BATCH,
            "build_id": F.build_info()["build_id"], **{k: stats(v) for k, v in ms.items()}}
    bytes_moved = 4.5 * S * S  # 1.5 B/px of planes and 3 B/px of RGB, either direction
    for k in ("c_yuv2rgb_kernel", "d_rgb2yuv_kernel"):
        line[k]["GBps"] = round(bytes_moved / (line[k]["median_ms"] * 1e-3) / 1e9, 1)
    line["a_minus_b_ms"] = round(line["a_decode_frc3"]["median_ms"] - line["b_three_decode_frc1"]["median_ms"], 4)
    text = json.dumps(line)
    print(text, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
