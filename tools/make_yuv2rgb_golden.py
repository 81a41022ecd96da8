#!/usr/bin/env python3
"""Goldens of the reference's ImageIO::yuv2rgb (image/ImageIO.cpp:68-84), data only, under tests/golden/.

Runs where the reference build exists (oracle/_ref/libfracref.so, which __graft_entry__.build() makes from the
unmodified reference sources with oracle/ref/Makefile's flags); never imported by a test.  The function is
called through its mangled name.  A gsl::span argument is a by-value {ptrdiff_t size; T* data}; the
reference's last parameter is the RGB stride in pixels.

  yuv2rgb.json          sha256 digests of the reference's RGB for (a) all 2^24 (y, u, v) triples in 4 chunks
                        (tests/yuv2rgb_ref.py all_triples_planes; digest over rgb[::2, ::2]) and (b) the
                        lenna_y / lenna_u / lenna_v planes
  rgb_from_yuv_odd.npz  seeded planes and the reference's RGB for 67×101, 3×5 and 2×2 frames (width × height).
                        For an odd width or height the reference reads chroma cell x/2 = w/2 (or y/2 = h/2),
                        one past the plane; it is given chroma planes edge-replicated by one column and one
                        row, so that read is defined and equals the library's clamp.  The file stores the
                        unreplicated planes.  (Named rgb_… so that tests/golden_util.py's list of search
                        goldens, every other .npz, leaves it out.)

usage: tools/make_yuv2rgb_golden.py
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from fractencode_amd.synth import sha256  # noqa: E402
from yuv2rgb_ref import all_triples_planes, seeded_planes  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SYMBOL = "_ZN5Frac27ImageIO7yuv2rgbEN3gsl4spanIKhLln1EEEjjjS4_jS4_jNS2_IhLln1EEEj"
ODD = ((67, 101, 11), (3, 5, 12), (2, 2, 13))  # width, height, seed


class Span(C.Structure):
    _fields_ = [("size", C.c_ssize_t), ("data", C.c_void_p)]


def span(a: np.ndarray) -> Span:
    return Span(a.size, a.ctypes.data)


def ref_yuv2rgb(fn, y, u, v) -> np.ndarray:
    """The reference on contiguous planes: U and V [ch, cw] with ch > (H − 1)/2 and cw > (W − 1)/2."""
    y, u, v = (np.ascontiguousarray(a, np.uint8) for a in (y, u, v))
    H, W = y.shape
    assert u.shape == v.shape and u.shape[0] > (H - 1) // 2 and u.shape[1] > (W - 1) // 2
    rgb = np.zeros((H, W, 3), np.uint8)
    fn(span(y), W, H, W, span(u), u.shape[1], span(v), v.shape[1], span(rgb), W)
    return rgb


def main():
    lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libfracref.so"))
    fn = getattr(lib, SYMBOL)
    u32 = C.c_uint32
    fn.argtypes = [Span, u32, u32, u32, Span, u32, Span, u32, Span, u32]
    fn.restype = None

    chunks = []
    for c in range(4):
        rgb = ref_yuv2rgb(fn, *all_triples_planes(c))
        chunks.append(sha256(np.ascontiguousarray(rgb[::2, ::2])))
    planes = [np.fromfile(os.path.join(GOLD, f"lenna_{k}.u8"), dtype=np.uint8) for k in "yuv"]
    lenna = ref_yuv2rgb(fn, planes[0].reshape(512, 512), planes[1].reshape(256, 256), planes[2].reshape(256, 256))
    with open(os.path.join(GOLD, "yuv2rgb.json"), "w") as f:
        json.dump({"layout": "tests/yuv2rgb_ref.py:all_triples_planes, sha256 of rgb[::2, ::2]", "chunks": chunks,
                   "lenna": sha256(lenna)}, f, indent=1)

    odd = {}
    for W, H, seed in ODD:
        y, u, v = seeded_planes(W, H, seed)
        rgb = ref_yuv2rgb(fn, y, np.pad(u, ((0, 1), (0, 1)), mode="edge"), np.pad(v, ((0, 1), (0, 1)), mode="edge"))
        for k, a in (("y", y), ("u", u), ("v", v), ("rgb", rgb)):
            odd[f"{k}_{W}x{H}"] = a
    np.savez_compressed(os.path.join(GOLD, "rgb_from_yuv_odd.npz"), **odd)
    print("yuv2rgb goldens written:", chunks, sha256(lenna))


if __name__ == "__main__":
    main()
