"""The classifier buckets' stable counting sort (bksort_count / bksort_scan / bksort_scatter, fracenc_bucket.hip)
through its test hook, frac_debug_bucket_sort: two sides through one launch_bucket_sorts call, against
np.argsort(kind="stable") — the sorted indices, the bucket starts, and the hook's fill where the sort writes
nothing (past a device-side count).  Sizes around a wave, a scatter round, the tile and the switch between the
self-scanning form (at most S tiles per side) and the three-launch form, whose scan gives each lane a run of
⌈tiles / 64⌉ tiles: S + 1 tiles (runs of 9, the last lanes empty), 576 (runs of 9, every lane full), 577 and 1,018
(runs of 10 and 16).  Each size meets a different size on the other side, an empty side included; a one-tile or empty
side beside a large one goes through the scan form with it.  Every case runs twice: byte-identical outputs."""
import numpy as np
import pytest

import fractencode_amd as F

pytestmark = pytest.mark.gpu

T, S, NB = F.BK_TILE, F.BK_SELF_TILES, F.BK_KEYS
FILL = 0xFFFFFFFF

SELF_SIZES = [0, 1, 63, 64, 255, 256, T - 1, T, T + 1, 4 * T + 17, S * T]
# each size with another of the list on the other side (a rotation by four: no size meets itself)
SELF_PAIRS = [(n, SELF_SIZES[(k + 4) % len(SELF_SIZES)]) for k, n in enumerate(SELF_SIZES)]
assert all(a != b for a, b in SELF_PAIRS) and any(a == 0 for a, _ in SELF_PAIRS) and any(b == 0 for _, b in SELF_PAIRS)
SCAN_TILES = [S + 1, 576, 577, 1018]
SCAN_SIZES = [t * T - 5 for t in SCAN_TILES]
# beside a one-tile side, an empty side, and (once) another large side, on either side of the launch
SCAN_PAIRS = [(n, T - 3) for n in SCAN_SIZES] + [(0, n) for n in SCAN_SIZES] + [(SCAN_SIZES[0], SCAN_SIZES[1])]

PATTERNS = ["random", "ends", "gap", "descending", "tile_runs", "wave_runs"] + [f"all{k}" for k in range(7)]


def _keys(pattern, n, seed):
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.int64)
    if pattern == "random":
        k = rng.integers(0, 7, n)
    elif pattern == "ends":        # only the first and the last bucket
        k = rng.integers(0, 2, n) * 6
    elif pattern == "gap":         # one middle bucket empty
        k = rng.integers(0, 6, n)
        k[k >= 3] += 1
    elif pattern == "descending":  # 6 … 0 in equal runs: the input is the reverse of the output's bucket order
        k = 6 - (i * 7) // max(n, 1)
    elif pattern == "tile_runs":   # the key changes exactly at every tile boundary
        k = (i // T) % 7
    elif pattern == "wave_runs":   # … and at every wave boundary, non-monotone
        k = ((i // 64) * 5 + 3) % 7
    else:
        k = np.full(n, int(pattern[3:]))
    return k.astype(np.uint32)


def _check(keys, dn, order, first, what):
    n = len(keys)
    m = n if dn is None else min(dn, n)
    want = np.argsort(keys[:m], kind="stable").astype(np.uint32)
    np.testing.assert_array_equal(order[:m], want, err_msg=f"{what}: order")
    assert (order[m:] == FILL).all(), f"{what}: written past the count"
    np.testing.assert_array_equal(first, np.searchsorted(keys[:m][want], np.arange(NB + 1)), err_msg=f"{what}: first")


def _run(ka, kb, dn_a=None, dn_b=None):
    out = F.debug_bucket_sort(ka, kb, dn_a, dn_b)
    again = F.debug_bucket_sort(ka, kb, dn_a, dn_b)
    for x, y in zip(out, again):
        assert x.tobytes() == y.tobytes(), "two runs on the same input differ"
    _check(ka, dn_a, out[0], out[1], "side a")
    _check(kb, dn_b, out[2], out[3], "side b")


def test_constants_are_the_library_s():
    assert (F.lib().frac_debug_bucket_tile(), F.lib().frac_debug_bucket_self_tiles()) == (T, S)
    assert T % 256 == 0 and S + 1 < 576  # the scan's lane runs below: 9 tiles from S + 1 to 576


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("na,nb", SELF_PAIRS, ids=[f"{a}+{b}" for a, b in SELF_PAIRS])
def test_self_scanning_form(na, nb, pattern):
    _run(_keys(pattern, na, 100 + na), _keys(pattern, nb, 200 + nb))


@pytest.mark.parametrize("pattern", ["random", "ends", "gap", "descending", "tile_runs", "wave_runs", "all0", "all6"])
@pytest.mark.parametrize("na,nb", SCAN_PAIRS, ids=[f"{a}+{b}" for a, b in SCAN_PAIRS])
def test_three_launch_form(na, nb, pattern):
    assert max(na, nb) > S * T
    _run(_keys(pattern, na, 300 + na % 1000), _keys(pattern, nb, 400 + nb % 1000))


def _counts(n):
    return [None, 0, 1, n - 1, n, n + 7]


@pytest.mark.parametrize("n,other", [(4 * T + 17, T), (T, 63), (SCAN_SIZES[2], T - 3)],
                         ids=["self", "one_tile", "three_launch"])
def test_device_side_count(n, other):
    """dn ∈ {none, 0, 1, n − 1, n, n + 7} on either side; the keys past the count are the padding key 7, as a
    device-planned level leaves them, or live keys the sort has to ignore."""
    rng = np.random.default_rng(n)
    for dn in _counts(n):
        m = n if dn is None else min(dn, n)
        for tail in ("pad", "live"):
            ka = rng.integers(0, 7, n).astype(np.uint32)
            if tail == "pad":
                ka[m:] = 7
            kb = rng.integers(0, 7, other).astype(np.uint32)
            _run(ka, kb, dn, None)
            _run(kb, ka, _counts(other)[(m + 2) % 6], dn)


def test_padding_key_inside_the_count_sorts_last():
    """Key 7 inside the count (a level's padding when no device count is passed) is an eighth bucket after the
    seven."""
    rng = np.random.default_rng(9)
    _run(rng.integers(0, 8, 3 * T + 5).astype(np.uint32), np.full(70, 7, np.uint32))


def test_refuses_a_key_outside_the_buckets():
    k = np.array([0, 3, 8], np.uint32)
    with pytest.raises(F.FracError, match="key"):
        F.debug_bucket_sort(k, k[:0])
    _run(np.array([0, 3, 6], np.uint32), k[:0])
