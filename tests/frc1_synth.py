"""Synthetic encode items and FRC1 streams for the decoder / packer tests: random records on any
frame geometry, made on the host without a search.  Every seed is the caller's and fixed."""
from __future__ import annotations

import numpy as np

from fractencode_amd import ENCODE_ITEM, codec
from golden_util import oracle_records

GEOMETRY = ("x", "y", "w", "h", "dx", "dy", "sw", "sh")


def _grid(extent: int, size: int, stride: int) -> int:
    return 0 if size > extent else (extent - size) // stride + 1


def synth_items(W, H, n, d, T, seed, *, lattice=True, cmax=1.1, empty_every=0, brightness=(-40.0, 290.0)):
    """ENCODE_ITEM records over the row-major createUniformGrid(n, n) range lattice of a W×H frame.

    Domains are d×d, random: on the (d, d/2) lattice (`lattice`, what an FRC1 stream can index) or at
    any origin inside the plane; transform random in [0, T), contrast uniform in ±cmax, brightness
    uniform in `brightness`.  With `empty_every` = k > 0 every k-th record (k − 1, 2k − 1, …) has no
    domain; when no d×d domain fits the frame, none has."""
    rng = np.random.default_rng(seed)
    rc, rr = _grid(W, n, n), _grid(H, n, n)
    nr = rc * rr
    items = np.zeros(nr, dtype=ENCODE_ITEM)
    r = np.arange(nr)
    items["x"], items["y"] = (r % max(rc, 1)) * n, (r // max(rc, 1)) * n
    items["w"] = items["h"] = n
    if lattice:
        s = d // 2
        dc, dr = _grid(W, d, s), _grid(H, d, s)
        dx, dy = rng.integers(0, max(dc, 1), nr) * s, rng.integers(0, max(dr, 1), nr) * s
    else:
        dc, dr = int(W >= d), int(H >= d)
        dx, dy = rng.integers(0, max(W - d, 0) + 1, nr), rng.integers(0, max(H - d, 0) + 1, nr)
    t = rng.integers(0, T, nr)
    c = rng.uniform(-cmax, cmax, nr)
    b = rng.uniform(brightness[0], brightness[1], nr)
    has = np.full(nr, dc * dr > 0)
    if empty_every > 0:
        has[empty_every - 1::empty_every] = False
    items["dx"], items["dy"] = np.where(has, dx, 0), np.where(has, dy, 0)
    items["sw"] = items["sh"] = np.where(has, d, 0)
    items["transform"] = np.where(has, t, 0)
    items["contrast"], items["brightness"] = np.where(has, c, 0.0), np.where(has, b, 0.0)
    return items


def synth_stream(W, H, n, d, T, seed, contrast_bits=5, brightness_bits=7, **kw) -> bytes:
    """codec.pack_stream over synth_items(..., lattice=True)."""
    items = synth_items(W, H, n, d, T, seed, lattice=True, **kw)
    return codec.pack_stream(items, W, H, n, d, transforms=T, contrast_bits=contrast_bits,
                             brightness_bits=brightness_bits)


def synth_mixed_items(W, H, seed, sizes=(16, 8, 4), T=8, cmax=0.6, brightness=(0.0, 200.0)):
    """A seeded random subdivision of W×H (multiples of sizes[0]) into squares of `sizes`: a square above
    the smallest size splits into its quadrants with probability 1/2.  Domains are twice each side, at
    any origin inside the plane.  Returns (ENCODE_ITEM records, range side per record)."""
    rng = np.random.default_rng(seed)
    out = []

    def place(x, y, k):
        s = sizes[k]
        if k + 1 < len(sizes) and rng.random() < 0.5:
            for qx, qy in ((0, 0), (1, 0), (0, 1), (1, 1)):
                place(x + qx * s // 2, y + qy * s // 2, k + 1)
        else:
            out.append((x, y, s))

    for y in range(0, H, sizes[0]):
        for x in range(0, W, sizes[0]):
            place(x, y, 0)
    items = np.zeros(len(out), dtype=ENCODE_ITEM)
    for i, (x, y, s) in enumerate(out):
        items[i]["x"], items[i]["y"], items[i]["w"], items[i]["h"] = x, y, s, s
        items[i]["dx"], items[i]["dy"] = rng.integers(0, W - 2 * s + 1), rng.integers(0, H - 2 * s + 1)
        items[i]["sw"] = items[i]["sh"] = 2 * s
    items["transform"] = rng.integers(0, T, len(out))
    items["contrast"] = rng.uniform(-cmax, cmax, len(out))
    items["brightness"] = rng.uniform(brightness[0], brightness[1], len(out))
    return items, items["w"].astype(np.uint32)


def scaled(rec: np.ndarray, scale: int) -> np.ndarray:
    """The records with every coordinate and size multiplied by `scale` (transform, contrast and
    brightness are resolution-independent)."""
    rec = rec.copy()
    for k in GEOMETRY:
        rec[k] *= scale
    return rec


def oracle_decode_stream(oracle, stream, scale=1, max_iter=-1, initial=None):
    """The oracle's decode of codec.unpack_stream's records, scaled → (plane, iterations, rms)."""
    rec, h = codec.unpack_stream(stream)
    return oracle.decode(oracle_records(scaled(rec, scale)), scale * h["range_size"], scale * h["width"],
                         scale * h["height"], max_iter=max_iter, initial=initial)


def set_bits(stream: bytes, bit: int, width: int, value: int) -> bytes:
    """The stream with body bits [bit, bit + width) overwritten by `value`, LSB first."""
    b = bytearray(stream)
    for k in range(width):
        byte, sh = codec.HEADER.size + (bit + k) // 8, (bit + k) % 8
        b[byte] = (b[byte] & ~(1 << sh)) | (((value >> k) & 1) << sh)
    return bytes(b)


# Stream geometries shared by the host codec tests and the device decoder tests.
# Frames the range grid tiles, domain side 2n, every record with a domain (frc1dec_step on the device):
# (W, H, n, T, contrast bits, brightness bits, record bits, decode scales)
FAST_STREAMS = [
    (24, 40, 8, 4, 5, 7, 18, (1, 2, 16)),    # 15 records, 270 bits: partial tail byte and word; 8 domains; R = 128 > tile
    (13, 9, 1, 8, 5, 7, 22, (1, 2, 3, 16)),  # R = 1, width no multiple of 4
    (70, 6, 2, 8, 5, 7, 22, (1, 3)),         # one tile row, H < 16
    (66, 27, 3, 4, 6, 9, 25, (1, 2, 5)),     # R = 3, 6, 15
    (100, 36, 4, 8, 5, 7, 23, (1, 3)),       # W > 64 and no multiple of 64
    (72, 40, 8, 4, 2, 2, 12, (1, 2)),        # narrowest record
    (208, 48, 16, 8, 16, 16, 40, (1, 2)),
    (65, 65, 1, 8, 23, 24, 63, (1, 2)),      # 4096 domains → 13 index bits; every bit offset mod 32 occurs
    (65, 65, 1, 8, 24, 24, 64, (1,)),        # the widest record
]
# Every other stream (frc1dec_expand → item decoder), T = 8, 5 + 7 bits: (W, H, n, d, empty_every)
OTHER_STREAMS = [
    (66, 27, 3, 4, 0),    # ratio 4/3
    (72, 40, 4, 4, 0),    # ratio 1
    (100, 36, 4, 10, 0),  # ratio 2.5
    (65, 35, 5, 20, 0),   # ratio 4
    (72, 40, 8, 16, 5),   # domain-less records mixed in: each 64×16 tile holds both kinds
    (12, 40, 8, 16, 0),   # no domain fits: n_domains = 0, every record domain-less, 1 index bit
    (5, 7, 8, 16, 0),     # no range fits: header only
    (67, 45, 2, 4, 0),    # margins with the fast geometry otherwise
    (4096, 8, 8, 16, 0),  # the scale bound's stream: 512 domain-less records
]


def fast_stream(k: int) -> bytes:
    W, H, n, T, cb, bb, _, _ = FAST_STREAMS[k]
    return synth_stream(W, H, n, 2 * n, T, 100 + k, cb, bb)


def other_stream(k: int) -> bytes:
    W, H, n, d, every = OTHER_STREAMS[k]
    return synth_stream(W, H, n, d, 8, 200 + k, empty_every=every)
