"""Host-side frames and cases for the quadtree tests at small, odd sizes (test_quadtree_frames.py checks
each case's property with the oracle alone on the CPU, test_gpu_quadtree_shapes.py runs the engines on
them).  Plain numpy, fixed seeds.

Plain value noise at these sizes splits every range down to min_size, so a level never has leaves and
splits at once.  mixed() puts three kinds of content side by side: smooth noise (leaves at the large
sizes), full noise (splits) and a band of constant 4×4 cells at three levels (exact matches: leaves at
distance 0, the only ones that stop at split distance 0).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

SEED = 11
TGT_SEED = 12  # the two-plane case's target: the same recipe, another seed


def mixed(W: int, H: int, seed: int = SEED) -> np.ndarray:
    """uint8 [H, W]: two-octave value noise in the left half, seven-octave in the right half, and in the
    bottom third 4×4 constant cells at the levels 0 / 60 / 120."""
    from fractencode_amd.synth import value_noise

    p = value_noise(W, H, seed, octaves=2)
    p[:, W // 2:] = value_noise(W, H, seed)[:, W // 2:]
    rng = np.random.default_rng(seed)
    bh = H // 3
    cells = rng.integers(0, 3, ((bh + 3) // 4, (W + 3) // 4), dtype=np.uint8) * 60
    p[H - bh:] = cells.repeat(4, 0).repeat(4, 1)[:bh, :W]
    return np.ascontiguousarray(p)


class Case(NamedTuple):
    name: str
    W: int
    H: int
    max_size: int
    min_size: int
    split: float | None  # None: one_split_distance() (exactly one first-level range splits)
    cls: bool
    T: int
    thr: float = 0.0
    two_planes: bool = False
    flip: bool = False  # the frame upside down: the band of constant cells on top, first in search order

    def planes(self):
        """(source, target or None)."""
        src, tgt = mixed(self.W, self.H), (mixed(self.W, self.H, TGT_SEED) if self.two_planes else None)
        if self.flip:
            src, tgt = np.ascontiguousarray(src[::-1]), (None if tgt is None else np.ascontiguousarray(tgt[::-1]))
        return src, tgt


def one_split_distance(oracle, case: Case) -> tuple[float, np.ndarray]:
    """The midpoint between the two largest first-level distances (a split distance at which exactly the
    worst first-level range splits), and the first level's distances."""
    src, tgt = case.planes()
    n = case.max_size
    assert case.W >= 2 * n and case.H >= 2 * n
    doms = oracle.uniform_grid(case.W, case.H, 2 * n, n)
    rngs = oracle.uniform_grid(case.W, case.H, n, n)
    if case.cls:
        doms = oracle.classify(src, doms)
        rngs = oracle.classify(src if tgt is None else tgt, rngs)
    res, _, _ = oracle.estimate(src, doms, rngs, T=case.T, thr=case.thr, use_classifier=case.cls, tgt=tgt)
    d = np.sort(res["dist"])
    return float(0.5 * (d[-1] + d[-2])), res["dist"]


def run_oracle(oracle, case: Case):
    """(records, sizes, stats, split distance) of oracle.quadtree on the case."""
    src, tgt = case.planes()
    split = one_split_distance(oracle, case)[0] if case.split is None else case.split
    recs, sizes, st = oracle.quadtree(src, case.max_size, case.min_size, split, T=case.T, use_classifier=case.cls,
                                      thr=case.thr, tgt=tgt, stats=True)
    return recs, sizes, st, split


# every level has at least 3 leaves, every level above min_size at least 3 splits
MIXED = [
    Case("m98x74_16_4", 98, 74, 16, 4, 400.0, True, 4),
    Case("m98x74_8_2", 98, 74, 8, 2, 400.0, True, 4),
    Case("m98x74_16_2", 98, 74, 16, 2, 400.0, False, 8),
    Case("m130x66_16_4", 130, 66, 16, 4, 400.0, True, 4),
    Case("m130x66_8_2", 130, 66, 8, 2, 200.0, True, 4),
    Case("m130x66_16_2", 130, 66, 16, 2, 150.0, False, 8),
    Case("m70x58_16_4", 70, 58, 16, 4, 600.0, True, 4),
    Case("m70x58_8_2", 70, 58, 8, 2, 400.0, True, 4),
    Case("m70x58_16_2", 70, 58, 16, 2, 380.0, False, 8),
]
# a searched range whose bucket holds no domain (classifier on)
EMPTY = [Case("e33x47_16_8", 33, 47, 16, 8, 400.0, True, 4)]
# a side below 2·16: the 16-level has ranges and no domain.  At (16, 4) every 16-range splits, at (16, 16)
# every leaf is the default record, and under a split distance above 1e5 the default record is a leaf of a
# frame whose later levels would have domains.  15×40 has no 16-range at all (a side below max_size).
NODOM_SPLIT = [Case(f"d{w}x{h}_16_4", w, h, 16, 4, 400.0, cls, 4)
               for (w, h), cls in zip(((16, 16), (20, 20), (31, 31), (15, 40)), (True, False, True, False))]
NODOM_LEAF = [Case(f"d{w}x{h}_16_16", w, h, 16, 16, 400.0, cls, 4)
              for (w, h), cls in zip(((16, 16), (20, 20), (31, 31), (15, 40)), (False, True, False, True))]
NODOM_LEAF.append(Case("d31x31_16_4_nosplit", 31, 31, 16, 4, 1e9, True, 4))
# a frame smaller than max_size: no level, no leaf
NORANGE = [Case("z15x15", 15, 15, 16, 4, 400.0, True, 4), Case("z12x40", 12, 40, 16, 4, 400.0, False, 4)]
SPLIT_NONE = Case("s98x74_none", 98, 74, 16, 4, 1e9, True, 4)
# (min_size 2: the band's constant 4×4 cells are exact matches of the 4-level, the sizes above have none)
SPLIT_ZERO = Case("s98x74_zero", 98, 74, 16, 2, 0.0, True, 4)
# (classifier off: with it on, three first-level ranges have an empty bucket and share the largest distance, 1e5)
SPLIT_ONE = Case("s98x74_one", 98, 74, 16, 4, None, False, 4)
# a level of more than 1,024 ranges with splits in its first 1,024-range tile and after it.  Only a level above
# min_size splits, so at (16, 4) it is the 8-level: more than 256 of the 16-ranges must split (a frame of more
# than 65,536 pixels; 21 × 17 = 357 ranges of 16 here) — hence the small split distance.  Upside down, so that
# the level's ranges past the first 1,024 lie in the noise (leaves and splits), not in the band (splits only)
TILE_CARRY = Case("t342x278_16_4", 342, 278, 16, 4, 10.0, True, 4, flip=True)
# a threshold above the band's exact matches: ranges stop at their first hit, not their best domain
HIT_THR = Case("h98x74_thr", 98, 74, 16, 4, 400.0, True, 4, thr=20.0)
TWO_PLANES = Case("p98x74_two", 98, 74, 16, 4, 400.0, True, 4, two_planes=True)

# T = 4 with the 8-level last: under the SEA engine the 8-level takes the tiled form, its ranges the quadrants
# of the split 16-ranges in parent order, and the frame's statistics name that form
SEA_TILED = Case("m98x74_16_8", 98, 74, 16, 8, 400.0, True, 4)

NODOM = NODOM_SPLIT + NODOM_LEAF
ALL = MIXED + EMPTY + NODOM + NORANGE + [SPLIT_NONE, SPLIT_ZERO, SPLIT_ONE, TILE_CARRY, HIT_THR, TWO_PLANES,
                                         SEA_TILED]
BY_NAME = {c.name: c for c in ALL}
assert len(BY_NAME) == len(ALL)

# the frames one engine sees in turn (test_one_engine_across_frames): mixed, no leaves, no domains at the
# 16-level, a wider mixed frame, the first again
SEQUENCE = [Case(f"q{i}_{w}x{h}", w, h, 16, 4, 400.0, True, 4)
            for i, (w, h) in enumerate(((98, 74), (15, 15), (31, 31), (130, 66), (98, 74)))]


def domain_count(W: int, H: int, n: int) -> int:
    """Items of createUniformGrid(W, H, 2n, n) inside the frame: the n-level's domains."""
    return ((W - 2 * n) // n + 1) * ((H - 2 * n) // n + 1) if W >= 2 * n and H >= 2 * n else 0


def as_oracle(items: np.ndarray) -> np.ndarray:
    """The engine's ENCODE_ITEM records in the oracle's RESULT_DTYPE."""
    from oracle.oracle import RESULT_DTYPE

    out = np.zeros(len(items), dtype=RESULT_DTYPE)
    for a, b in (("x", "x"), ("y", "y"), ("dx", "dx"), ("dy", "dy"), ("sw", "dw"), ("sh", "dh"), ("transform", "t"),
                 ("distance", "dist"), ("contrast", "s"), ("brightness", "o")):
        out[b] = items[a]
    return out


def as_items(recs: np.ndarray, sizes: np.ndarray) -> np.ndarray:
    """The oracle's records and sizes as ENCODE_ITEM records (what the engine must return, bit for bit)."""
    import fractencode_amd as F

    out = np.zeros(len(recs), dtype=F.ENCODE_ITEM)
    for a, b in (("x", "x"), ("y", "y"), ("dx", "dx"), ("dy", "dy"), ("sw", "dw"), ("sh", "dh"), ("transform", "t"),
                 ("distance", "dist"), ("contrast", "s"), ("brightness", "o")):
        out[a] = recs[b]
    out["w"] = out["h"] = sizes
    return out


def leaves_from_records(rec: np.ndarray, W: int) -> np.ndarray:
    """numpy restatement of frac_qt_leaf packing (include/fracenc.h): the tests' independent packer."""
    import fractencode_amd as F

    n = rec["w"].astype(np.int64)
    cols = (W - 2 * n) // n + 1
    has = rec["sw"] != 0
    d = np.where(has, (rec["dy"].astype(np.int64) // n) * cols + rec["dx"].astype(np.int64) // n, F.QT_NO_DOMAIN)
    lv = np.log2(n).astype(np.int64)
    out = np.zeros(len(rec), dtype=F.QT_LEAF)
    out["x"], out["y"] = rec["x"], rec["y"]
    out["code"] = (d & 0xFFFFFF) | ((rec["transform"].astype(np.int64) & 15) << 24) | (lv << 28)
    for k in ("contrast", "brightness", "distance"):
        out[k] = rec[k]
    return out
