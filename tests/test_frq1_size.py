"""frac_frq1_size (the closed-form size of an FRQ1 stream from its per-level split counts, host only) against
len(codec.pack_quadtree_stream(...)) on synthetic partitions (frq1_synth.py): T = 1, 4, 8, the narrowest, the
default and the widest quantizer fields, levels without a node, and levels of 31, 32 and 33 nodes (the split
bitmap's dword edge).  No device."""
import numpy as np
import pytest

import fractencode_amd as F
import frq1_synth as FS
from fractencode_amd import codec

BITS = [(2, 2), (5, 7), (16, 16)]


def _splits(items, W, H, sizes):
    """(per-level split counts, per-level node counts) of a partition's leaves."""
    N = ((W - sizes[0]) // sizes[0] + 1) * ((H - sizes[0]) // sizes[0] + 1) if W >= sizes[0] and H >= sizes[0] else 0
    S, nodes = [], []
    for n in sizes:
        M = int((items["w"] == n).sum())
        nodes.append(N)
        S.append(N - M)
        N = 4 * (N - M)
    assert S[-1] == 0
    return S[:-1], nodes


def _check(items, W, H, sizes, T, cb, bb):
    S, nodes = _splits(items, W, H, sizes)
    stream = codec.pack_quadtree_stream(items, W, H, sizes[0], sizes[-1], transforms=T, contrast_bits=cb,
                                        brightness_bits=bb)
    assert F.frq1_size(W, H, sizes[0], sizes[-1], S, T, cb, bb) == len(stream), (W, H, sizes, T, cb, bb, S)
    return nodes


@pytest.mark.parametrize("T", [1, 4, 8])
@pytest.mark.parametrize("name", sorted(FS.CASES))
def test_size_equals_the_packed_stream(name, T):
    W, H, sizes, seed, kw = FS.CASES[name]
    items = FS.synth_quadtree_items(W, H, seed, sizes, T=T, **kw)
    for cb, bb in BITS:
        _check(items, W, H, sizes, T, cb, bb)


def test_levels_without_a_node():
    W, H, sizes, seed, kw = FS.CASES["128x64_none"]
    nodes = _check(FS.synth_quadtree_items(W, H, seed, sizes, **kw), W, H, sizes, 8, 5, 7)
    assert nodes[0] > 0 and nodes[1:] == [0, 0]
    W, H, sizes, seed, kw = FS.CASES["15x15_none"]
    nodes = _check(FS.synth_quadtree_items(W, H, seed, sizes, **kw), W, H, sizes, 8, 5, 7)
    assert nodes == [0, 0, 0]
    assert F.frq1_size(W, H, 16, 4, [0, 0]) == 64


@pytest.mark.parametrize("n0", [31, 32, 33])
def test_bitmap_dword_edge(n0):
    # a first level of 31, 32 and 33 nodes; with one, eight and nine of them split, a second level of 4, 32 and 36
    W, H, sizes = 8 * n0, 11, (8, 4, 2)
    seen = set()
    for seed, split in ((1, 0.0), (2, 0.25), (3, 0.5), (4, 1.0)):
        items = FS.synth_quadtree_items(W, H, seed, sizes, T=4, split=split)
        for cb, bb in BITS:
            nodes = _check(items, W, H, sizes, 4, cb, bb)
        assert nodes[0] == n0
        seen.add(nodes[1])
    assert 0 in seen and 4 * n0 in seen
    # a second level of 28, 32 and 36 nodes: its bitmap takes one dword up to 32 nodes, two above
    rb1 = max(1, (((W - 8) // 4 + 1) * ((H - 8) // 4 + 1)).bit_length()) + 2 + 5 + 7
    s = [F.frq1_size(W, H, 8, 2, [k, 0]) for k in (7, 8, 9)]
    rec = lambda n: 4 * ((n * rb1 + 31) // 32)  # noqa: E731
    no16 = 1 + 2 + 5 + 7  # no 16×16 domain fits an 11-row frame: a one-bit index
    first = lambda k: 4 * (((n0 - k) * no16 + 31) // 32)  # noqa: E731
    assert s[1] - s[0] == rec(32) - rec(28) + first(8) - first(7)
    assert s[2] - s[1] == 4 + rec(36) - rec(32) + first(9) - first(8)


def test_refusals():
    ok = dict(width=96, height=64, max_size=16, min_size=4, splits=[2, 3])
    assert F.frq1_size(**ok) > 64
    for bad in (dict(contrast_bits=1), dict(contrast_bits=17), dict(brightness_bits=1), dict(brightness_bits=17),
                dict(max_size=3), dict(max_size=32), dict(min_size=1), dict(max_size=4, min_size=8),
                dict(transforms=0), dict(transforms=9), dict(width=0), dict(height=0), dict(width=65536),
                dict(height=65536),
                dict(splits=[25, 0]),    # 24 nodes at the 16-level
                dict(splits=[2, 9]),     # 8 nodes at the 8-level
                dict(splits=[0, 1])):    # none at the 8-level
        with pytest.raises(F.FracError):
            F.frq1_size(**{**ok, **bad})
    assert F.frq1_size(**{**ok, "splits": [24, 96]}) > F.frq1_size(**{**ok, "splits": [24, 95]})
    # a single level reads no split count
    assert F.frq1_size(96, 64, 8, 8, []) == 64 + 4 * ((96 * (max(1, (11 * 7).bit_length()) + 2 + 12) + 31) // 32)
