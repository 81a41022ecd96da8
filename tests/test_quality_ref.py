"""CPU checks of the decoded-quality feature: quality_ref.py's restatement of the rules pinned on hand-made
inputs, the decoded errors of the two frames the GPU tests bisect over (through the oracle alone), and the
library's three entry points at the ABI boundary (no device call)."""
import ctypes as C

import numpy as np
import pytest

import fractencode_amd as F
import quadtree_frames as Q
import quadtree_rate_ref as R
import quality_ref as QR
from fractencode_amd import codec
from frq1_synth import oracle_decode_quadtree_stream

SYMBOLS = ("frac_decode_error", "frac_quadtree_rate_errors", "frac_quadtree_rate_quality")


def test_covered_rectangle_and_block_sums():
    assert QR.covered(98, 74, 16) == (96, 64) and QR.covered(50, 38, 12) == (48, 36)
    assert QR.covered(15, 15, 16) == (0, 0) and QR.covered(64, 32, 8) == (64, 32)
    a = np.zeros((5, 7), np.uint8)
    b = np.zeros((5, 7), np.uint8)
    a[0, 0], b[0, 1] = 255, 3      # block (0, 0): 255² + 3²
    a[2, 5], b[2, 5] = 10, 250     # block (1, 2): 240² (no uint8 wrap-around)
    a[4, 0] = a[0, 6] = 200        # outside the covered 6 × 4
    total, blocks = QR.sse(a, b, 2)
    assert blocks.shape == (2, 3) and blocks.dtype == np.int64
    assert blocks.tolist() == [[255 * 255 + 9, 0, 0], [0, 0, 240 * 240]] and total == 255 * 255 + 9 + 240 * 240
    total, blocks = QR.sse(a, b, 8)
    assert total == 0 and blocks.shape == (0, 0)
    # a full plane of the largest difference stays exact in int64
    total, _ = QR.sse(np.full((64, 64), 255, np.uint8), np.zeros((64, 64), np.uint8), 16)
    assert total == 64 * 64 * 255 * 255


def test_bisect_on_a_monotone_list():
    E = [10, 20, 30, 40, 50, 60, 70]  # the error grows with the split distance
    assert QR.bisect(E, 70) == (6, 1) and QR.bisect(E, 1000) == (6, 1)
    assert QR.bisect(E, 69) == (5, 5)   # probes 6 (fails), 0, 3, 4, 5 (all meet)
    assert QR.bisect(E, 40) == (3, 4)   # 6, 0, 3 (meets), 4 (fails)
    assert QR.bisect(E, 39) == (2, 5)   # 6, 0, 3 (fails), 1, 2 (meet)
    assert QR.bisect(E, 10) == (0, 4)   # 6, 0, 3, 1 (fail)
    assert QR.bisect(E, 9) == (None, 2)


def test_bisect_counts_its_probes():
    # the rule by hand at m = 7, target 10: probe 6 (fails), 0 (meets), mid 3 (fails, hi = 3), mid 1 (fails,
    # hi = 1): hi − lo = 1 ends it — four probes, not five
    seen = []

    class Spy(list):
        def __getitem__(self, i):
            seen.append(i)
            return list.__getitem__(self, i)

    assert QR.bisect(Spy([10, 20, 30, 40, 50, 60, 70]), 10) == (0, 4)
    assert seen == [6, 0, 3, 1]


def test_bisect_on_a_non_monotone_list():
    E = [50, 10, 60, 20, 70, 30, 80]
    # target 55: 6 fails, 0 meets, mid 3 meets (lo = 3), mid 4 fails (hi = 4): answer 3, though 5 meets too
    assert QR.bisect(E, 55) == (3, 4)
    assert E[5] <= 55 < E[4]  # the guarantee: the next larger candidate fails; not the largest that meets
    # target 50: 6 fails, 0 meets, 3 meets, 4 fails
    assert QR.bisect(E, 50) == (3, 4)
    # target 49: the smallest candidate fails although others meet: refused
    assert QR.bisect(E, 49) == (None, 2)
    # the largest candidate meets: one probe, whatever lies below
    assert QR.bisect([90, 80, 5], 5) == (2, 1)


def test_bisect_edges():
    assert QR.bisect([7], 7) == (0, 1) and QR.bisect([7], 6) == (None, 1) and QR.bisect([0], 0) == (0, 1)
    assert QR.bisect([1, 2], 1) == (0, 2) and QR.bisect([1, 2], 2) == (1, 1) and QR.bisect([3, 2], 2) == (1, 1)
    assert QR.bisect([1, 2, 3], 0) == (None, 2)          # none meets
    assert QR.bisect([1, 2, 3], 3) == (2, 1)             # all meet
    E = [100, 200, 300, 400, 500]
    for i, v in enumerate(E):                            # the target at E, E − 1 and E + 1
        assert QR.bisect(E, v)[0] == i and QR.bisect(E, v + 1)[0] == i
        assert QR.bisect(E, v - 1)[0] == (i - 1 if i else None)


def test_psnr_target_as_an_error_bound():
    assert QR.max_sse_of(10 * np.log10(255.0 ** 2), 1000) in (999, 1000)  # MSE 1 (the power rounds either way)
    assert QR.max_sse_of(20.0, 96 * 64) == int(np.floor(65025.0 * 96 * 64 / 100.0))
    assert QR.max_sse_of(30.0, 0) == 0


def _tree_items(tree, t):
    """The ENCODE_ITEM leaves of the tree's partition at split distance t, in canonical order (Tree.leaves'
    rule, before its leaf packing)."""
    recs, sizes = [], []
    reached = np.ones(len(tree.recs[0]), bool)
    for k, n in enumerate(tree.sides):
        split = reached & (tree.recs[k]["dist"] > t) if k + 1 < tree.levels else np.zeros(len(reached), bool)
        leaf = reached & ~split
        recs.append(tree.recs[k][leaf])
        sizes.append(np.full(int(leaf.sum()), n, np.uint32))
        reached = np.repeat(split, 4)
    return Q.as_items(np.concatenate(recs), np.concatenate(sizes))


@pytest.mark.parametrize("name,m", [("m98x74_16_4", 113), ("m70x58_16_4", 49)])
def test_decoded_error_is_not_monotone_in_the_split_distance(oracle, name, m):
    # the frames test_gpu_quality.py bisects over: every candidate's decoded error through the oracle alone
    # (its search, the host packer, its decoder).  All distinct and far from monotone, so any deviation from the
    # stated rule changes the answer or the probe count somewhere.
    case = Q.BY_NAME[name]
    tree = R.tree(oracle, case)
    cands = tree.candidates()
    assert len(cands) == m
    src, tgt = case.planes()
    E = []
    for t in cands:
        s = codec.pack_quadtree_stream(_tree_items(tree, float(t)), case.W, case.H, case.max_size, case.min_size,
                                       transforms=case.T, use_classifier=case.cls)
        plane = oracle_decode_quadtree_stream(oracle, s)[0]
        E.append(QR.sse(plane, src if tgt is None else tgt, case.max_size)[0])
    assert len(set(E)) == m
    assert E != sorted(E) and E != sorted(E, reverse=True)


def test_library_exports_the_quality_symbols():
    lib = F.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert getattr(lib, name).restype is C.c_int


def test_a_null_context_is_invalid():
    lib = F.lib()
    buf = (C.c_uint8 * 64)()
    t = (C.c_double * 1)(1.0)
    assert lib.frac_decode_error(None, buf, 64, -1, 1e-5, None, None, None, 0, None, None, None) == -1
    assert lib.frac_quadtree_rate_errors(None, 5, 7, t, 1, -1, 1e-5, None, None, None) == -1
    assert lib.frac_quadtree_rate_quality(None, 5, 7, 0, -1, 1e-5, None, None, None, None, None) == -1
