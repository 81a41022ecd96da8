"""Quantized encoded stream for the search's winners.

The reference has no file format: `encode_data_statistics` (main.cpp:106-140) only
builds `Frac::Quantizerd` over the frame's (contrast, brightness) range with 5 and 7
bits (main.cpp:120-121) and prints bucket counts.  This module keeps that quantizer
bit-for-bit and defines the record the reference leaves open:

    per range: (domain index, transform, q_contrast, q_brightness)

bit-packed LSB-first at a fixed width per field.  At C3 (261,121 domains, T=4,
5+7 bits) a record is 18+2+5+7 = 32 bits, i.e. 1 MiB per 4096² frame instead of
the 16 MiB of 64-byte encode_item_t records.

Stream layout ("FRC1", little-endian)::

    0   char[4]  magic "FRC1"
    4   u16      version (1)
    6   u16      flags (bit 0: classifier was on; informational)
    8   u32      width, height
    16  u32      range_size, domain_size, domain_stride
    28  u8       transforms, contrast_bits, brightness_bits, index_bits
    32  u32      n_ranges, n_domains
    40  f64      contrast_min, contrast_max, brightness_min, brightness_max
    72  u8[]     records, ceil(n_ranges * record_bits / 8) bytes

Ranges are the createUniformGrid(range_size, range_size) lattice in row-major order
(image/partition2.hpp:109-135); domain index i is position i of
createUniformGrid(domain_size, domain_stride); index == n_domains marks a range that
had no eligible domain (the reference's default record, encode/datatypes.h:8-26).
When every value of a field is equal the quantizer would be degenerate (the reference
asserts max > min, Quantizer.hpp:19): the header then stores min == max and every
record dequantizes to exactly that value.
frac_decode_frc1 (Engine.decode_frc1) consumes this layout on the device; unpack_stream is its host restatement.

Quadtree stream layout ("FRQ1", little-endian): the leaves of frac_encode_quadtree, whose sizes differ, so
the partition itself is part of the stream::

    0   char[4]  magic "FRQ1"
    4   u16      version (1)
    6   u16      flags (bit 0: classifier was on; informational)
    8   u32      width, height
    16  u8       max_size, min_size, transforms, contrast_bits, brightness_bits, then three zero bytes
    24  u32      n_leaves, then one zero u32
    32  f64      contrast_min, contrast_max, brightness_min, brightness_max
    64  body

Levels are k = 0..L−1 with sides n_k = max_size >> k down to min_size (sides from {2, 4, 8, 16}, L ≤ 4).
The nodes of level 0 are createUniformGrid(max_size, max_size) in row-major order; the nodes of level k+1
are, for each split node of level k in that level's order, its quadrants top-left, top-right, bottom-left,
bottom-right (N_{k+1} = 4·S_k).  This is the order frac_encode_quadtree emits its leaves in.  The body holds,
per level in level order:

    split bitmap  for k < L−1 only: N_k bits, LSB first, 1 = split; zero-padded to a whole dword (the
                  padding bits must be 0); no bytes when N_k = 0
    records       the level's M_k = N_k − S_k leaves in node order (the last level has no bitmap: every
                  node is a leaf): (domain index, transform, q_contrast, q_brightness) bit-packed LSB first
                  exactly as FRC1, index_bits_k = max(1, bitlen(nd_k)) wide with nd_k the count of
                  createUniformGrid(2·n_k, n_k); index == nd_k: no domain; zero-padded to a whole dword

One quantizer pair covers the whole stream, built over every leaf's contrast and brightness as FRC1's.
frac_decode_frq1 (Engine.decode_frq1) consumes this layout on the device, frac_pack_frq1 writes it from
32-byte leaves; pack_quadtree_stream / unpack_quadtree_stream are the host restatement.

Colour container layout ("FRC3", little-endian): one colour frame, the three plane streams of a colour
encode (fractencode_amd.color) in one buffer::

    0   char[4]  magic "FRC3"
    4   u16      version (1)
    6   u16      flags (reserved, 0)
    8   u32      width, height          the RGB frame's; both >= 2 and <= 65535
    16  u32      len_y, len_u, len_v    bytes of each plane stream
    28  u32      reserved, 0
    32  the Y, U, V plane streams in that order, each a complete FRC1 or FRQ1 stream (told apart by its own
        magic, kinds may be mixed), each zero-padded to a multiple of 8 bytes

The Y stream's frame is width × height, the U and V streams' (width/2) × (height/2), as rgb2yuv makes the
planes (image/ImageIO.cpp:43-58).  frac_decode_frc3 (Engine.decode_frc3) decodes the three planes on the
device and converts them to packed RGB there (ImageIO::yuv2rgb, ImageIO.cpp:68-84); frac_pack_frc3 /
frac_frc3_info write and parse the container; pack_color_stream / unpack_color_stream are the host restatement.

Sequence container layout ("FRCS", little-endian): the frames of one closed-loop sequence (SequenceEncoder) in
one buffer.  An I frame is an ordinary stream, decoded iteratively; a P frame's records read their domains in the
previous decoded frame and are applied to it once (frac_decode_inter).  The streams themselves are unchanged FRC1 /
FRQ1 bytes: only this container says which is which.  Host only (pack_sequence / unpack_sequence)::

    0   char[4]  magic "FRCS"
    4   u16      version (1)
    6   u16      flags (reserved, 0)
    8   u32      width, height          every frame's; both in 1..65535
    16  u32      n_frames
    20  per frame, 8 bytes: u8 kind ('I' = 0x49 or 'P' = 0x50), three zero bytes, u32 length of its stream
    20 + 8·n_frames  the streams in frame order, each a complete FRC1 or FRQ1 stream of a width × height frame,
        each zero-padded to a multiple of 8 bytes

The first frame is an I frame.
"""
from __future__ import annotations

import struct
from fractions import Fraction

import numpy as np

MAGIC = b"FRC1"
VERSION = 1
HEADER = struct.Struct("<4sHHIIIIIBBBBIIdddd")
assert HEADER.size == 72
CONTRAST_BITS = 5  # main.cpp:120
BRIGHTNESS_BITS = 7  # main.cpp:121


class Quantizer:
    """Frac::Quantizer<double> (encode/Quantizer.hpp:7-45).

    step = |max − min| / 2^bits; quantized(v) = min(2^bits − 1, floor((v − min) / step));
    value(q) = q·step + min + step/2, where the built reference contracts q·step + min
    into one FMA (verified against oracle/_ref's fr_quantize), reproduced here exactly
    through a per-code table computed in rational arithmetic.
    """

    def __init__(self, vmin: float, vmax: float, bits: int):
        if not (vmax > vmin):
            raise ValueError("Quantizer: max must exceed min (Quantizer.hpp:19)")
        if not (1 < bits <= 24):
            raise ValueError("Quantizer: bits must be in (1, 24]")
        self.min = float(vmin)
        self.max = float(vmax)
        self.bits = int(bits)
        self.step = abs(self.max - self.min) / float(1 << self.bits)
        self.max_quantized = (1 << self.bits) - 1
        if not self.step > 0.0:
            raise ValueError("Quantizer: zero step (Quantizer.hpp:22)")
        self._table = None

    def quantized(self, v) -> np.ndarray:
        v = np.asarray(v, dtype=np.float64)
        q = np.floor((v - self.min) / self.step)
        return np.minimum(float(self.max_quantized), q).astype(np.uint64)

    def _values(self, codes) -> np.ndarray:
        """fl(fl(q·step + min) + step/2) per code, the first rounding fused (one rounding of the exact rational)."""
        step, mn, half = Fraction(self.step), Fraction(self.min), self.step / 2
        fused = [float(int(q) * step + mn) for q in codes]
        return np.array(fused, dtype=np.float64) + half

    def table(self) -> np.ndarray:
        """value(q) for every code q: 2^bits rationals, for small `bits` only (value() does not need it)."""
        if self._table is None:
            self._table = self._values(range(self.max_quantized + 1))
        return self._table

    def value(self, q) -> np.ndarray:
        q = np.asarray(q, dtype=np.uint64)
        if q.size and int(q.max()) > self.max_quantized:
            raise ValueError("Quantizer: code out of range (Quantizer.hpp:34)")
        # only the codes present: a 24-bit field has 2^24 codes, a stream a few thousand of them
        codes, inv = np.unique(q, return_inverse=True)
        return self._values(codes)[inv.reshape(q.shape)]


def psnr(a: np.ndarray, b: np.ndarray, peak: float = 255.0) -> float:
    """10·log10(peak² / MSE) over two equally shaped u8 planes (inf when identical)."""
    a = np.asarray(a, dtype=np.int64)
    b = np.asarray(b, dtype=np.int64)
    if a.shape != b.shape:
        raise ValueError("psnr: shape mismatch")
    mse = float(((a - b) ** 2).sum()) / a.size
    return float("inf") if mse == 0.0 else 10.0 * np.log10(peak * peak / mse)


def _grid_cols_rows(width: int, height: int, size: int, stride: int) -> tuple[int, int]:
    """Column / row count of createUniformGrid (image/partition2.hpp:123-133)."""
    if size > width or size > height:
        return 0, 0
    return (width - size) // stride + 1, (height - size) // stride + 1


class _Field:
    def __init__(self, v: np.ndarray, bits: int):
        lo, hi = (float(v.min()), float(v.max())) if len(v) else (0.0, 0.0)
        self.min, self.max, self.bits = lo, hi, bits
        self.q = None if not hi > lo else Quantizer(lo, hi, bits)

    def codes(self, v: np.ndarray) -> np.ndarray:
        return np.zeros(len(v), np.uint64) if self.q is None else self.q.quantized(v)


def _pack_bits(fields: list[tuple[np.ndarray, int]], n: int) -> bytes:
    """Record i's fields, concatenated LSB-first, occupy bits [i·width, (i+1)·width) of the body."""
    width = sum(b for _, b in fields)
    bits = np.zeros((n, width), dtype=np.uint8)
    shift = 0
    for vals, b in fields:
        v = vals.astype(np.uint64)
        if n and int(v.max()) >> b:
            raise ValueError("pack: field value does not fit its width")
        for k in range(b):
            bits[:, shift + k] = (v >> np.uint64(k)) & np.uint64(1)
        shift += b
    return np.packbits(bits.reshape(-1), bitorder="little").tobytes()


def _unpack_bits(buf: bytes, n: int, widths: list[int]) -> list[np.ndarray]:
    width = sum(widths)
    raw = np.frombuffer(buf, dtype=np.uint8)
    bits = np.unpackbits(raw, bitorder="little")[: n * width].reshape(n, width).astype(np.uint64)
    out, shift = [], 0
    for b in widths:
        w = np.zeros(n, dtype=np.uint64)
        for k in range(b):
            w |= bits[:, shift + k] << np.uint64(k)
        out.append(w)
        shift += b
    return out


def pack_stream(items: np.ndarray, width: int, height: int, range_size: int, domain_size: int | None = None,
                transforms: int = 4, use_classifier: bool = False, contrast_bits: int = CONTRAST_BITS,
                brightness_bits: int = BRIGHTNESS_BITS) -> bytes:
    """Quantize and pack encode_item_t records (fractencode_amd.ENCODE_ITEM, range order) into FRC1."""
    from . import ENCODE_ITEM

    items = np.ascontiguousarray(items, dtype=ENCODE_ITEM)
    dsz = domain_size or 2 * range_size
    dstride = dsz // 2  # latticeSize = 2 (encode/encode_parameters.h:8), main.cpp:147
    rc, rr = _grid_cols_rows(width, height, range_size, range_size)
    if len(items) != rc * rr:
        raise ValueError(f"pack_stream: {len(items)} records, the range grid has {rc * rr}")
    exp_x = (np.arange(rc * rr) % max(rc, 1)) * range_size
    exp_y = (np.arange(rc * rr) // max(rc, 1)) * range_size
    if len(items) and (np.any(items["x"] != exp_x) or np.any(items["y"] != exp_y)):
        raise ValueError("pack_stream: records are not in row-major range-grid order")
    dc, dr = _grid_cols_rows(width, height, dsz, dstride)
    nd = dc * dr
    has = (items["sw"] != 0) & (items["sh"] != 0)
    if np.any(has & ((items["dx"] % dstride != 0) | (items["dy"] % dstride != 0))):
        raise ValueError("pack_stream: a winner is not on the domain lattice")
    idx = np.where(has, (items["dy"] // dstride) * dc + items["dx"] // dstride, nd).astype(np.uint64)
    if np.any(has & (idx >= nd)):
        raise ValueError("pack_stream: a winner lies outside the domain grid")
    index_bits = max(1, int(nd).bit_length())
    t_bits = max(1, int(transforms - 1).bit_length())
    s_f = _Field(items["contrast"], contrast_bits)
    o_f = _Field(items["brightness"], brightness_bits)
    hdr = HEADER.pack(MAGIC, VERSION, 1 if use_classifier else 0, width, height, range_size, dsz, dstride, transforms,
                      contrast_bits, brightness_bits, index_bits, len(items), nd, s_f.min, s_f.max, o_f.min, o_f.max)
    body = _pack_bits([(idx, index_bits), (items["transform"].astype(np.uint64), t_bits),
                       (s_f.codes(items["contrast"]), contrast_bits), (o_f.codes(items["brightness"]), brightness_bits)],
                      len(items))
    return hdr + body


def read_header(buf: bytes) -> dict:
    if len(buf) < HEADER.size:
        raise ValueError("FRC1: truncated header")
    f = HEADER.unpack_from(buf, 0)
    if f[0] != MAGIC or f[1] != VERSION:
        raise ValueError("FRC1: bad magic or version")
    keys = ("magic", "version", "flags", "width", "height", "range_size", "domain_size", "domain_stride", "transforms",
            "contrast_bits", "brightness_bits", "index_bits", "n_ranges", "n_domains", "contrast_min",
            "contrast_max", "brightness_min", "brightness_max")
    return dict(zip(keys, f))


def unpack_stream(buf: bytes) -> tuple[np.ndarray, dict]:
    """FRC1 → (encode_item_t records with dequantized contrast/brightness, header dict).
    `distance` is not carried by the stream and comes back as 0."""
    from . import ENCODE_ITEM

    h = read_header(buf)
    n, nd = h["n_ranges"], h["n_domains"]
    t_bits = max(1, int(h["transforms"] - 1).bit_length())
    widths = [h["index_bits"], t_bits, h["contrast_bits"], h["brightness_bits"]]
    need = (n * sum(widths) + 7) // 8
    if len(buf) < HEADER.size + need:
        raise ValueError("FRC1: truncated records")
    idx, t, qs, qo = _unpack_bits(buf[HEADER.size:HEADER.size + need], n, widths)
    rc, _ = _grid_cols_rows(h["width"], h["height"], h["range_size"], h["range_size"])
    dc, _ = _grid_cols_rows(h["width"], h["height"], h["domain_size"], h["domain_stride"])
    out = np.zeros(n, dtype=ENCODE_ITEM)
    r = np.arange(n)
    out["x"] = (r % max(rc, 1)) * h["range_size"]
    out["y"] = (r // max(rc, 1)) * h["range_size"]
    out["w"] = out["h"] = h["range_size"]
    has = idx < nd
    if np.any(idx > nd):
        raise ValueError("FRC1: domain index out of range")
    di = np.where(has, idx, 0).astype(np.int64)
    out["dx"] = np.where(has, (di % max(dc, 1)) * h["domain_stride"], 0)
    out["dy"] = np.where(has, (di // max(dc, 1)) * h["domain_stride"], 0)
    out["sw"] = out["sh"] = np.where(has, h["domain_size"], 0)
    out["transform"] = t.astype(np.int32)

    def deq(codes, lo, hi, bits):
        if not hi > lo:
            return np.full(n, lo)
        return Quantizer(lo, hi, bits).value(codes)

    out["contrast"] = np.where(has, deq(qs, h["contrast_min"], h["contrast_max"], h["contrast_bits"]), 0.0)
    out["brightness"] = np.where(has, deq(qo, h["brightness_min"], h["brightness_max"], h["brightness_bits"]), 0.0)
    out["transform"] = np.where(has, out["transform"], 0)
    return out, h


# ---- FRQ1: the quadtree stream (layout in the module docstring) ---------------------------------

QT_MAGIC = b"FRQ1"
QT_HEADER = struct.Struct("<4sHHIIBBBBB3xIIdddd")
assert QT_HEADER.size == 64
QT_SIZES = (2, 4, 8, 16)


def quadtree_levels(max_size: int, min_size: int) -> list[int]:
    """The level sides max_size, max_size / 2, …, min_size."""
    if max_size not in QT_SIZES or min_size not in QT_SIZES or min_size > max_size:
        raise ValueError("FRQ1: sizes must be 2, 4, 8 or 16, min_size at most max_size")
    out = [max_size]
    while out[-1] > min_size:
        out.append(out[-1] // 2)
    return out


def _level0_nodes(width: int, height: int, n: int) -> tuple[np.ndarray, np.ndarray]:
    rc, rr = _grid_cols_rows(width, height, n, n)
    r = np.arange(rc * rr, dtype=np.int64)
    return (r % max(rc, 1)) * n, (r // max(rc, 1)) * n


def _children(x: np.ndarray, y: np.ndarray, n: int) -> tuple[np.ndarray, np.ndarray]:
    """The quadrants (top-left, top-right, bottom-left, bottom-right) of the nodes, node by node."""
    h = n // 2
    return ((x[:, None] + np.array([0, h, 0, h])).reshape(-1), (y[:, None] + np.array([0, 0, h, h])).reshape(-1))


def _pad4(b: bytes) -> bytes:
    return b + bytes(-len(b) % 4)


def pack_quadtree_stream(items: np.ndarray, width: int, height: int, max_size: int, min_size: int,
                         transforms: int = 4, use_classifier: bool = False, contrast_bits: int = CONTRAST_BITS,
                         brightness_bits: int = BRIGHTNESS_BITS) -> bytes:
    """Quantize and pack quadtree leaves (ENCODE_ITEM records in frac_encode_quadtree's output order) into FRQ1."""
    from . import ENCODE_ITEM

    items = np.ascontiguousarray(items, dtype=ENCODE_ITEM)
    sizes = quadtree_levels(max_size, min_size)
    if not (0 < width <= 65535 and 0 < height <= 65535):
        raise ValueError("FRQ1: width and height must be in 1..65535")
    if np.any(items["w"] != items["h"]) or not np.isin(items["w"], sizes).all():
        raise ValueError("pack_quadtree_stream: a leaf's size is none of the levels'")
    if len(items) > 1 and np.any(np.diff(items["w"].astype(np.int64)) > 0):
        raise ValueError("pack_quadtree_stream: leaves are not in level order")
    s_f = _Field(items["contrast"], contrast_bits)
    o_f = _Field(items["brightness"], brightness_bits)
    t_bits = max(1, int(transforms - 1).bit_length())
    if len(items) and int(items["transform"].max()) >= transforms or len(items) and int(items["transform"].min()) < 0:
        raise ValueError("pack_quadtree_stream: a transform outside the stream's")
    body = b""
    x, y = _level0_nodes(width, height, sizes[0])
    for k, n in enumerate(sizes):
        lv = items[items["w"] == n]
        key, lkey = y * 65536 + x, lv["y"].astype(np.int64) * 65536 + lv["x"]
        leaf = np.isin(key, lkey)
        if int(leaf.sum()) != len(lv) or np.any(key[leaf] != lkey):
            raise ValueError(f"pack_quadtree_stream: the {n}-level's leaves are not its nodes in canonical order")
        if k + 1 < len(sizes):
            body += _pad4(np.packbits((~leaf).astype(np.uint8), bitorder="little").tobytes())
        elif not leaf.all():
            raise ValueError("pack_quadtree_stream: a node of the last level has no leaf")
        dc, dr = _grid_cols_rows(width, height, 2 * n, n)
        nd = dc * dr
        has = (lv["sw"] != 0) & (lv["sh"] != 0)
        if np.any(has & ((lv["sw"] != 2 * n) | (lv["sh"] != 2 * n) | (lv["dx"] % n != 0) | (lv["dy"] % n != 0))):
            raise ValueError("pack_quadtree_stream: a winner is not on its level's domain lattice")
        idx = np.where(has, (lv["dy"] // n).astype(np.int64) * dc + lv["dx"] // n, nd).astype(np.uint64)
        if np.any(has & ((idx >= nd) | (lv["dx"] // n >= max(dc, 1)))):
            raise ValueError("pack_quadtree_stream: a winner lies outside its level's domain grid")
        body += _pad4(_pack_bits([(idx, max(1, int(nd).bit_length())), (lv["transform"].astype(np.uint64), t_bits),
                                  (s_f.codes(lv["contrast"]), contrast_bits),
                                  (o_f.codes(lv["brightness"]), brightness_bits)], len(lv)))
        x, y = _children(x[~leaf], y[~leaf], n)
    hdr = QT_HEADER.pack(QT_MAGIC, VERSION, 1 if use_classifier else 0, width, height, max_size, min_size, transforms,
                         contrast_bits, brightness_bits, len(items), 0, s_f.min, s_f.max, o_f.min, o_f.max)
    return hdr + body


def read_quadtree_header(buf: bytes) -> dict:
    if len(buf) < QT_HEADER.size:
        raise ValueError("FRQ1: truncated header")
    f = QT_HEADER.unpack_from(buf, 0)
    if f[0] != QT_MAGIC or f[1] != VERSION:
        raise ValueError("FRQ1: bad magic or version")
    keys = ("magic", "version", "flags", "width", "height", "max_size", "min_size", "transforms", "contrast_bits",
            "brightness_bits", "n_leaves", "reserved", "contrast_min", "contrast_max", "brightness_min",
            "brightness_max")
    h = dict(zip(keys, f))
    if h.pop("reserved") or any(buf[21:24]):
        raise ValueError("FRQ1: a reserved byte or word is not zero")
    if not (0 < h["width"] <= 65535 and 0 < h["height"] <= 65535):
        raise ValueError("FRQ1: width and height must be in 1..65535")
    quadtree_levels(h["max_size"], h["min_size"])
    if not 1 <= h["transforms"] <= 8:
        raise ValueError("FRQ1: transforms outside 1..8")
    if not (2 <= h["contrast_bits"] <= 24 and 2 <= h["brightness_bits"] <= 24):
        raise ValueError("FRQ1: contrast / brightness bits outside [2, 24]")
    if not all(np.isfinite(h[k]) for k in ("contrast_min", "contrast_max", "brightness_min", "brightness_max")):
        raise ValueError("FRQ1: non-finite quantizer bound")
    return h


def unpack_quadtree_stream(buf: bytes) -> tuple[np.ndarray, dict]:
    """FRQ1 → (encode_item_t records in the stream's order with dequantized contrast/brightness, header dict).
    The dict also carries what the walk derives: levels and, per level, nodes, leaves, n_domains, index_bits,
    record_bits, bitmap_offset and record_offset (bytes from the start of the stream), and body_bytes.
    `distance` is not carried by the stream and comes back as 0."""
    from . import ENCODE_ITEM

    buf = bytes(buf)
    h = read_quadtree_header(buf)
    sizes = quadtree_levels(h["max_size"], h["min_size"])
    W, H = h["width"], h["height"]
    t_bits = max(1, int(h["transforms"] - 1).bit_length())
    for k in ("nodes", "leaves", "n_domains", "index_bits", "record_bits", "bitmap_offset", "record_offset"):
        h[k] = [0] * 4
    h["levels"] = len(sizes)
    parts = []
    pos = QT_HEADER.size
    x, y = _level0_nodes(W, H, sizes[0])
    for k, n in enumerate(sizes):
        N = len(x)
        split = np.zeros(N, dtype=bool)
        h["bitmap_offset"][k] = pos
        if k + 1 < len(sizes):
            nb = (N + 31) // 32 * 4
            if len(buf) < pos + nb:
                raise ValueError("FRQ1: truncated split bitmap")
            bits = np.unpackbits(np.frombuffer(buf, np.uint8, nb, pos), bitorder="little")
            if bits[N:].any():
                raise ValueError("FRQ1: a padding bit of a split bitmap is set")
            split = bits[:N].astype(bool)
            pos += nb
        dc, dr = _grid_cols_rows(W, H, 2 * n, n)
        nd = dc * dr
        widths = [max(1, int(nd).bit_length()), t_bits, h["contrast_bits"], h["brightness_bits"]]
        M = N - int(split.sum())
        nb = (M * sum(widths) + 31) // 32 * 4
        if len(buf) < pos + nb:
            raise ValueError("FRQ1: truncated records")
        h["nodes"][k], h["leaves"][k], h["n_domains"][k] = N, M, nd
        h["index_bits"][k], h["record_bits"][k], h["record_offset"][k] = widths[0], sum(widths), pos
        idx, t, qs, qo = _unpack_bits(buf[pos:pos + nb], M, widths)
        pos += nb
        if np.any(idx > nd):
            raise ValueError("FRQ1: domain index out of range")
        out = np.zeros(M, dtype=ENCODE_ITEM)
        out["x"], out["y"] = x[~split], y[~split]
        out["w"] = out["h"] = n
        has = idx < nd
        di = np.where(has, idx, 0).astype(np.int64)
        out["dx"] = np.where(has, (di % max(dc, 1)) * n, 0)
        out["dy"] = np.where(has, (di // max(dc, 1)) * n, 0)
        out["sw"] = out["sh"] = np.where(has, 2 * n, 0)
        out["transform"] = np.where(has, t.astype(np.int32), 0)
        parts.append((out, has, qs, qo))
        x, y = _children(x[split], y[split], n)
    h["body_bytes"] = pos - QT_HEADER.size
    rec = np.concatenate([p[0] for p in parts])
    if len(rec) != h["n_leaves"]:
        raise ValueError("FRQ1: n_leaves is not the levels' leaf count")
    has = np.concatenate([p[1] for p in parts])

    def deq(codes, lo, hi, bits):
        if not hi > lo:
            return np.full(len(rec), lo)
        return Quantizer(lo, hi, bits).value(codes)

    rec["contrast"] = np.where(has, deq(np.concatenate([p[2] for p in parts]), h["contrast_min"], h["contrast_max"],
                                        h["contrast_bits"]), 0.0)
    rec["brightness"] = np.where(has, deq(np.concatenate([p[3] for p in parts]), h["brightness_min"],
                                          h["brightness_max"], h["brightness_bits"]), 0.0)
    return rec, h


# ---- FRC3: the colour container (layout in the module docstring) --------------------------------

COLOR_MAGIC = b"FRC3"
COLOR_HEADER = struct.Struct("<4sHHIIIIII")
assert COLOR_HEADER.size == 32
KIND_FRC1, KIND_FRQ1 = 1, 2


def _plane_stream_frame(buf: bytes, name: str) -> tuple[int, int, int]:
    """(kind, width, height) of a plane stream, which its own unpacker must accept."""
    magic = bytes(buf[:4])
    if magic == MAGIC:
        # frac_frc1_info's rules on the header, which unpack_stream takes on trust
        h = read_header(buf)
        if not (h["width"] and h["height"] and h["range_size"]):
            raise ValueError("FRC1: zero width, height or range size")
        if h["domain_size"] < 2 or h["domain_size"] % 2 or h["domain_stride"] != h["domain_size"] // 2:
            raise ValueError("FRC1: domain size must be even and at least 2, its stride half of it")
        if not 1 <= h["transforms"] <= 8:
            raise ValueError("FRC1: transforms outside 1..8")
        if not (2 <= h["contrast_bits"] <= 24 and 2 <= h["brightness_bits"] <= 24):
            raise ValueError("FRC1: contrast / brightness bits outside [2, 24]")
        grids = [_grid_cols_rows(h["width"], h["height"], *g) for g in
                 ((h["range_size"], h["range_size"]), (h["domain_size"], h["domain_stride"]))]
        if [h["n_ranges"], h["n_domains"]] != [c * r for c, r in grids]:
            raise ValueError("FRC1: range or domain count is not its grid's")
        if h["index_bits"] != max(1, int(h["n_domains"]).bit_length()):
            raise ValueError("FRC1: index bits do not match the domain count")
        if not all(np.isfinite(h[k]) for k in ("contrast_min", "contrast_max", "brightness_min", "brightness_max")):
            raise ValueError("FRC1: non-finite quantizer bound")
        _, h = unpack_stream(buf)
        kind = KIND_FRC1
    elif magic == QT_MAGIC:
        _, h = unpack_quadtree_stream(buf)
        kind = KIND_FRQ1
    else:
        raise ValueError(f"FRC3: the {name} stream is neither an FRC1 nor an FRQ1 stream")
    return kind, h["width"], h["height"]


def _check_color_planes(streams, width: int, height: int) -> list[int]:
    if not (2 <= width <= 65535 and 2 <= height <= 65535):
        raise ValueError("FRC3: width and height must be in 2..65535")
    if len(streams) != 3:
        raise ValueError("FRC3: three plane streams (Y, U, V)")
    kinds = []
    for k, (name, s) in enumerate(zip("YUV", streams)):
        kind, w, h = _plane_stream_frame(bytes(s), name)
        want = (width, height) if k == 0 else (width // 2, height // 2)
        if (w, h) != want:
            raise ValueError(f"FRC3: the {name} stream's frame is {w}x{h}, the plane's {want[0]}x{want[1]}")
        kinds.append(kind)
    return kinds


def pack_color_stream(streams, width: int, height: int) -> bytes:
    """The Y, U and V plane streams (FRC1 or FRQ1, kinds may be mixed) of a width × height RGB frame as one
    FRC3 container."""
    streams = [bytes(s) for s in streams]
    _check_color_planes(streams, width, height)
    out = COLOR_HEADER.pack(COLOR_MAGIC, VERSION, 0, width, height, *(len(s) for s in streams), 0)
    for s in streams:
        out += s + bytes(-len(s) % 8)
    return out


def unpack_color_stream(buf: bytes) -> tuple[list[bytes], dict]:
    """FRC3 → ([Y, U, V] plane streams without their padding, header dict).  The dict has width, height, flags
    and, per plane, kind (1 = FRC1, 2 = FRQ1), offset and length (bytes from the start of the container), and
    total_bytes.  Every plane stream is checked by its own unpacker and against the frame."""
    buf = bytes(buf)
    if len(buf) < COLOR_HEADER.size:
        raise ValueError("FRC3: truncated header")
    magic, version, flags, width, height, ly, lu, lv, reserved = COLOR_HEADER.unpack_from(buf, 0)
    if magic != COLOR_MAGIC or version != VERSION:
        raise ValueError("FRC3: bad magic or version")
    if flags or reserved:
        raise ValueError("FRC3: the flags or the reserved word are not zero")
    if not (2 <= width <= 65535 and 2 <= height <= 65535):
        raise ValueError("FRC3: width and height must be in 2..65535")
    h = {"width": width, "height": height, "flags": flags, "kind": [], "offset": [], "length": []}
    pos, streams = COLOR_HEADER.size, []
    for n in (ly, lu, lv):
        padded = n + (-n % 8)
        if len(buf) - pos < padded:
            raise ValueError("FRC3: a plane section runs past the end of the stream")
        if any(buf[pos + n:pos + padded]):
            raise ValueError("FRC3: a padding byte is not zero")
        streams.append(buf[pos:pos + n])
        h["offset"].append(pos)
        h["length"].append(n)
        pos += padded
    h["total_bytes"] = pos
    h["kind"] = _check_color_planes(streams, width, height)
    return streams, h


# ---- FRCS: the sequence container (layout in the module docstring) ------------------------------

SEQ_MAGIC = b"FRCS"
SEQ_HEADER = struct.Struct("<4sHHII")
assert SEQ_HEADER.size == 16
SEQ_COUNT = struct.Struct("<I")
SEQ_FRAME = struct.Struct("<B3sI")
SEQ_KINDS = {"I": 0x49, "P": 0x50}


def _check_sequence_frames(frames, width: int, height: int) -> None:
    for k, (kind, s) in enumerate(frames):
        if kind not in SEQ_KINDS:
            raise ValueError(f"FRCS: frame {k}: kind {kind!r} is neither I nor P")
        if k == 0 and kind != "I":
            raise ValueError("FRCS: the first frame must be an I frame")
        _, w, h = _plane_stream_frame(bytes(s), f"frame {k}")
        if (w, h) != (width, height):
            raise ValueError(f"FRCS: frame {k}'s stream is {w}x{h}, the sequence {width}x{height}")


def pack_sequence(frames, width: int, height: int) -> bytes:
    """[(kind, stream), ...] with kind "I" or "P" and each stream a complete FRC1 or FRQ1 stream of a
    width × height frame, as one FRCS container."""
    frames = [(kind, bytes(s)) for kind, s in frames]
    if not (1 <= width <= 65535 and 1 <= height <= 65535):
        raise ValueError("FRCS: width and height must be in 1..65535")
    _check_sequence_frames(frames, width, height)
    out = SEQ_HEADER.pack(SEQ_MAGIC, VERSION, 0, width, height) + SEQ_COUNT.pack(len(frames))
    for kind, s in frames:
        out += SEQ_FRAME.pack(SEQ_KINDS[kind], bytes(3), len(s))
    for _, s in frames:
        out += s + bytes(-len(s) % 8)
    return out


def unpack_sequence(buf: bytes) -> tuple[list[tuple[str, bytes]], dict]:
    """FRCS → ([(kind, stream), ...] without the padding, header dict: width, height, flags, frames, and per
    frame offset and length in bytes from the start of the container, total_bytes).  Every frame stream is
    checked by its own unpacker and against the sequence's frame."""
    buf = bytes(buf)
    if len(buf) < SEQ_HEADER.size + SEQ_COUNT.size:
        raise ValueError("FRCS: truncated header")
    magic, version, flags, width, height = SEQ_HEADER.unpack_from(buf, 0)
    if magic != SEQ_MAGIC or version != VERSION:
        raise ValueError("FRCS: bad magic or version")
    if flags:
        raise ValueError("FRCS: the flags are not zero")
    if not (1 <= width <= 65535 and 1 <= height <= 65535):
        raise ValueError("FRCS: width and height must be in 1..65535")
    (n,) = SEQ_COUNT.unpack_from(buf, SEQ_HEADER.size)
    pos = SEQ_HEADER.size + SEQ_COUNT.size
    if len(buf) - pos < n * SEQ_FRAME.size:
        raise ValueError("FRCS: the frame table runs past the end of the container")
    names = {v: k for k, v in SEQ_KINDS.items()}
    table = []
    for k in range(n):
        kind, pad, length = SEQ_FRAME.unpack_from(buf, pos)
        if any(pad):
            raise ValueError("FRCS: a padding byte is not zero")
        if kind not in names:
            raise ValueError(f"FRCS: frame {k}: kind {kind:#x} is neither I nor P")
        table.append((names[kind], length))
        pos += SEQ_FRAME.size
    h = {"width": width, "height": height, "flags": flags, "frames": n, "offset": [], "length": []}
    frames = []
    for kind, length in table:
        padded = length + (-length % 8)
        if len(buf) - pos < padded:
            raise ValueError("FRCS: a frame section runs past the end of the container")
        if any(buf[pos + length:pos + padded]):
            raise ValueError("FRCS: a padding byte is not zero")
        frames.append((kind, buf[pos:pos + length]))
        h["offset"].append(pos)
        h["length"].append(length)
        pos += padded
    h["total_bytes"] = pos
    _check_sequence_frames(frames, width, height)
    return frames, h
