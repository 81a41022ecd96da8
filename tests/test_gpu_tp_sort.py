"""The tiled SEA form's sort (fracenc_tpsort.hip) through its test hook, frac_debug_sort_pairs: two sides of
(key, value) uint32 pairs through the same launches, against np.argsort(kind="stable") — keys and values, both
sides.  Sizes around the chunk (C items per workgroup: 0, 1, a wave's 63 / 64, C − 1, C, C + 1, 3C + 17), each
side paired with a different size of the list and one side empty; 16-, 17- and 19-bit keys (two and three
passes); key patterns that leave one digit or both constant, reverse the input, tie in long runs across chunk
boundaries, and — with bucket bits — are non-monotone in the input as the ranges' buckets are.  Every case runs
twice: the second output must be byte-identical.  Sizes of 64 chunks, one item more and 65 C + 17 run the scan of
the per-chunk counts (tp_sort_offsets) through its carry from one 64-chunk round to the next."""
import numpy as np
import pytest

import fractencode_amd as F

pytestmark = pytest.mark.gpu

C = F.TP_SORT_CHUNK
SIZES = [0, 1, 63, 64, C - 1, C, C + 1, 3 * C + 17]
# each size with another of the list on the other side (a rotation by three: no size meets itself)
PAIRS = [(n, SIZES[(k + 3) % len(SIZES)]) for k, n in enumerate(SIZES)]
assert all(a != b for a, b in PAIRS) and any(a == 0 for a, _ in PAIRS) and any(b == 0 for _, b in PAIRS)

PATTERNS = ["equal", "descending", "high_digit", "low_digit", "few_values", "buckets"]


def _keys(pattern, n, bits, seed):
    rng = np.random.default_rng(seed)
    top = (1 << bits) - 1
    i = np.arange(n, dtype=np.int64)
    if pattern == "equal":
        k = np.full(n, 0x1a5a5 & top)
    elif pattern == "descending":  # strictly: n ≤ 3C + 17 < 2^16
        k = top - i
    elif pattern == "high_digit":  # bits 8 and up differ, the low digit is constant
        k = ((rng.integers(0, 1 << (bits - 8), n) << 8) | 0x5a) & top
    elif pattern == "low_digit":   # only the low digit differs
        k = ((0x1a5 << 8) & top & ~0xff) | rng.integers(0, 256, n)
    elif pattern == "few_values":  # about 30 distinct keys: long runs of ties across chunk boundaries
        k = rng.integers(0, 1 << bits, 30)[rng.integers(0, 30, n)]
    else:                          # (bucket << 16) | sum with the bucket non-monotone in the input
        nb = 1 << (bits - 16)
        k = (((i * 5 + 3) % nb) << 16) | rng.integers(0, 1 << 16, n) if nb > 1 else rng.integers(0, 1 << 16, n)
    return k.astype(np.uint32)


def _want(k, v, bits):
    order = np.argsort(k & np.uint32((1 << bits) - 1), kind="stable")
    return k[order], v[order]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("bits", [16, 17, 19])
@pytest.mark.parametrize("n,nb", PAIRS, ids=[f"{a}+{b}" for a, b in PAIRS])
def test_sort_is_the_stable_order(n, nb, bits, pattern):
    assert F.lib().frac_debug_sort_chunk() == C
    ka, kb = _keys(pattern, n, bits, 1000 + n), _keys(pattern, nb, bits, 2000 + nb)
    assert ka.size == 0 or int(ka.max()) < (1 << bits)
    # values: the input index on one side (as tp_keys writes them), arbitrary words on the other
    va = np.arange(n, dtype=np.uint32)
    vb = np.random.default_rng(nb).integers(0, 1 << 32, nb, dtype=np.uint64).astype(np.uint32)
    first = F.debug_sort_pairs(ka, va, kb, vb, bits)
    again = F.debug_sort_pairs(ka, va, kb, vb, bits)
    for got, (k, v), side in ((first[:2], (ka, va), "a"), (first[2:], (kb, vb), "b")):
        wk, wv = _want(k, v, bits)
        np.testing.assert_array_equal(got[0], wk, err_msg=f"side {side}: keys")
        np.testing.assert_array_equal(got[1], wv, err_msg=f"side {side}: values")
    for x, y in zip(first, again):
        assert x.tobytes() == y.tobytes(), "two runs on the same input differ"


# 64 chunks (one round of tp_sort_offsets' scan, every lane live), 65 (a second round of one lane) and 66
LONG = [64 * C, 64 * C + 1, 65 * C + 17]
LONG_PAIRS = [(LONG[0], LONG[2]), (LONG[1], 0), (LONG[2], LONG[1]), (C + 1, LONG[0])]


@pytest.mark.parametrize("pattern", ["few_values", "buckets"])
@pytest.mark.parametrize("bits", [16, 19])
@pytest.mark.parametrize("n,nb", LONG_PAIRS, ids=[f"{a}+{b}" for a, b in LONG_PAIRS])
def test_more_chunks_than_a_wave_scans_at_once(n, nb, bits, pattern):
    test_sort_is_the_stable_order(n, nb, bits, pattern)


def test_high_key_bits_are_carried_not_sorted():
    """Bits above `bits` travel with the key and do not order it."""
    rng = np.random.default_rng(7)
    k = rng.integers(0, 1 << 32, C + 5, dtype=np.uint64).astype(np.uint32)
    v = np.arange(k.size, dtype=np.uint32)
    gk, gv, ek, ev = F.debug_sort_pairs(k, v, k[:0], v[:0], 16)
    wk, wv = _want(k, v, 16)
    np.testing.assert_array_equal(gk, wk)
    np.testing.assert_array_equal(gv, wv)
    assert ek.size == 0 and ev.size == 0
