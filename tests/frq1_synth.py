"""Synthetic quadtree partitions and FRQ1 streams for the codec and decoder tests: seeded random leaves on
any frame geometry, made on the host without a search.  Every seed is the caller's and fixed."""
from __future__ import annotations

import numpy as np

from fractencode_amd import ENCODE_ITEM, codec
from frc1_synth import scaled
from golden_util import oracle_records


def synth_quadtree_items(W, H, seed, sizes=(16, 8, 4), T=8, split=0.5, empty_every=0, cmax=0.6,
                         brightness=(0.0, 200.0)):
    """ENCODE_ITEM leaves of a seeded random quadtree over the createUniformGrid(sizes[0], sizes[0]) lattice of
    a W×H frame, in the canonical (FRQ1, frac_encode_quadtree) order: a square above the smallest size splits
    into its quadrants with probability `split`; the leaves of the depth-first recursion are stable-sorted
    by descending size, which is the breadth-first order.  Each leaf's domain lies on its level's (2n, n)
    lattice; a level without a domain in the frame has domain-less leaves, and with `empty_every` = k > 0
    every k-th leaf (k − 1, 2k − 1, …) is domain-less too."""
    rng = np.random.default_rng(seed)
    out = []

    def place(x, y, k):
        s = sizes[k]
        if k + 1 < len(sizes) and rng.random() < split:
            for qx, qy in ((0, 0), (1, 0), (0, 1), (1, 1)):
                place(x + qx * s // 2, y + qy * s // 2, k + 1)
        else:
            out.append((x, y, s))

    for y in range(0, H - sizes[0] + 1, sizes[0]):
        for x in range(0, W - sizes[0] + 1, sizes[0]):
            place(x, y, 0)
    out = [out[i] for i in np.argsort([-s for _, _, s in out], kind="stable")]
    n = len(out)
    items = np.zeros(n, dtype=ENCODE_ITEM)
    if n:
        items["x"], items["y"], items["w"] = np.array(out, dtype=np.int64).T
    items["h"] = items["w"]
    s = items["w"].astype(np.int64)
    dc = np.where(W >= 2 * s, (W - 2 * s) // np.maximum(s, 1) + 1, 0)
    dr = np.where(H >= 2 * s, (H - 2 * s) // np.maximum(s, 1) + 1, 0)
    has = dc * dr > 0
    if empty_every > 0:
        has[empty_every - 1::empty_every] = False
    dx, dy = rng.integers(0, np.maximum(dc, 1)) * s, rng.integers(0, np.maximum(dr, 1)) * s
    items["dx"], items["dy"] = np.where(has, dx, 0), np.where(has, dy, 0)
    items["sw"] = items["sh"] = np.where(has, 2 * s, 0)
    items["transform"] = np.where(has, rng.integers(0, T, n), 0)
    items["contrast"] = np.where(has, rng.uniform(-cmax, cmax, n), 0.0)
    items["brightness"] = np.where(has, rng.uniform(brightness[0], brightness[1], n), 0.0)
    return items


def synth_quadtree_stream(W, H, seed, sizes=(16, 8, 4), T=8, contrast_bits=5, brightness_bits=7, **kw) -> bytes:
    """codec.pack_quadtree_stream over synth_quadtree_items."""
    items = synth_quadtree_items(W, H, seed, sizes, T, **kw)
    return codec.pack_quadtree_stream(items, W, H, sizes[0], sizes[-1], transforms=T, contrast_bits=contrast_bits,
                                      brightness_bits=brightness_bits)


def oracle_decode_quadtree_stream(oracle, stream, scale=1, max_iter=-1, initial=None):
    """The oracle's decode of codec.unpack_quadtree_stream's records, scaled → (plane, iterations, rms)."""
    rec, h = codec.unpack_quadtree_stream(stream)
    return oracle.decode_sized(oracle_records(scaled(rec, scale)), scale * rec["w"], scale * h["width"],
                               scale * h["height"], max_iter, initial=initial)


def set_stream_bits(stream: bytes, offset: int, bit: int, width: int, value: int) -> bytes:
    """The stream with bits [bit, bit + width) of the section at byte `offset` overwritten by `value`, LSB first."""
    b = bytearray(stream)
    for k in range(width):
        byte, sh = offset + (bit + k) // 8, (bit + k) % 8
        b[byte] = (b[byte] & ~(1 << sh)) | (((value >> k) & 1) << sh)
    return bytes(b)


def record_fields(stream: bytes, h: dict, level: int, j: int) -> tuple[list[int], list[int], int]:
    """(field values, field widths, first bit) of record j of `level`, from codec.unpack_quadtree_stream's header dict."""
    t_bits = max(1, int(h["transforms"] - 1).bit_length())
    widths = [h["index_bits"][level], t_bits, h["contrast_bits"], h["brightness_bits"]]
    fields = codec._unpack_bits(stream[h["record_offset"][level]:], h["leaves"][level], widths)
    return [int(f[j]) for f in fields], widths, j * sum(widths)


# Partitions shared by the host codec tests and the device decoder tests: (W, H, sizes, seed, keywords of
# synth_quadtree_items) by name.
CASES = {
    "96x64": (96, 64, (16, 8, 4), 41, {}),
    "48x32_to2": (48, 32, (16, 8, 4, 2), 42, {}),
    "80x48_16_8": (80, 48, (16, 8), 43, {}),
    "24x40_8": (24, 40, (8,), 44, {}),
    "128x64_all": (128, 64, (16, 8, 4), 45, {"split": 1.0}),
    "128x64_none": (128, 64, (16, 8, 4), 46, {"split": 0.0}),
    "256x128_carry": (256, 128, (8, 4, 2), 47, {"split": 0.7}),
    "70x58_margins": (70, 58, (16, 8, 4), 48, {}),
    "96x64_empty5": (96, 64, (16, 8, 4), 49, {"empty_every": 5}),
    "20x20_nodom": (20, 20, (16,), 50, {}),
    "15x15_none": (15, 15, (16, 8, 4), 51, {}),
}


def case_items(name: str) -> np.ndarray:
    W, H, sizes, seed, kw = CASES[name]
    return synth_quadtree_items(W, H, seed, sizes, **kw)


def case_stream(name: str, contrast_bits=5, brightness_bits=7) -> bytes:
    W, H, sizes, seed, kw = CASES[name]
    return synth_quadtree_stream(W, H, seed, sizes, contrast_bits=contrast_bits, brightness_bits=brightness_bits, **kw)
