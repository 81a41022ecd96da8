"""The plain classifier reference of tests/classifier_ref.py, pinned (no GPU): against the oracle, the library's
host helper, the reference's own preclassify (the two opencl_classify fixtures), and the conditions the case set of
tests/test_gpu_bucket_keys.py has to meet, so that a case cannot quietly stop testing what it is there for.  Every
comparison is exact integer equality."""
import json
import os

import numpy as np
import pytest

import classifier_ref as R
import fractencode_amd as F
from golden_util import GOLD


def _fixture(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    return z["items"], json.loads(bytes(z["meta"]).decode())


def _all_grids():
    """Every (plane name, items) the GPU tests classify: the cases' two sides and Engine.classify's grids."""
    for c in R.CASES:
        (s, t), (d, r) = (c.src, c.tgt or c.src), c.grids()
        yield c.name + ":d", s, d
        yield c.name + ":r", t, r
    for pl, g in R.CLASSIFY_CASES:
        yield f"classify:{pl}:{g}", pl, R.grid(*R.plane_size(pl), *g)


def test_rules_are_the_24_orders_but_one():
    """23 of the 24 strict orders of four values have a rule; the contradictory rule covers none, so one order
    (a3 > a2 > a1 > a4 … whichever is missing) falls to −1.  Category k has four rules."""
    import itertools

    cats = {}
    for perm in itertools.permutations((1, 2, 3, 4)):  # perm[0] is the largest
        sums = np.zeros((1, 4), np.int64)
        for rank, q in enumerate(perm):
            sums[0, q - 1] = 10 - rank
        cats[perm] = int(R.category_of_sums(sums)[0])
    assert sorted(cats.values()).count(-1) == 1
    assert [list(cats.values()).count(k) for k in range(6)] == [4, 4, 4, 4, 4, 3]
    assert cats[(4, 1, 3, 2)] == -1  # Classifier2.cpp:48 reads a4 > a1, a1 > a3, a3 > a4 for it
    # a tie anywhere leaves no strict order
    assert int(R.category_of_sums(np.array([[5, 5, 3, 1]]))[0]) == -1


def test_reference_matches_oracle_and_host_helper(oracle):
    seen = 0
    for name, pl, items in _all_grids():
        p = R.plane(pl)
        want = R.categories(p, items)
        np.testing.assert_array_equal(oracle.classify(p, items.astype(oracle.ITEM_DTYPE))["category"], want,
                                      err_msg=f"oracle, {name}")
        np.testing.assert_array_equal(F.preclassify(p, items)["category"], want, err_msg=f"preclassify, {name}")
        seen += len(items)
    assert seen > 10000


def test_reference_matches_the_reference_build_on_4x4_items(oracle):
    ref, meta = _fixture("opencl_classify")
    p = R.plane("ocl_512x512")
    from fractencode_amd.synth import sha256
    assert sha256(p) == meta["plane_sha256"]
    items = R.grid(512, 512, (4, 4), (4, 2))
    for k in ("x", "y", "w", "h"):
        np.testing.assert_array_equal(items[k], ref[k], err_msg=k)
    np.testing.assert_array_equal(R.categories(p, items), ref["category"])


def test_reference_matches_the_reference_build_on_rectangles_and_the_wrap(oracle):
    """tests/golden/opencl_classify_rect.npz: the reference's preclassify on the wrap plane's five grids.  The
    reference wins: the numpy reference, the oracle and the host helper all equal it."""
    ref, meta = _fixture("opencl_classify_rect")
    p = R.plane(R.WRAP_PLANE)
    from fractencode_amd.synth import sha256
    assert sha256(p) == meta["plane_sha256"]
    assert [tuple(g) for g in meta["grids"]] == [(*s, *o) for s, o in R.RECT_GRIDS]
    items = np.concatenate([R.grid(*R.plane_size(R.WRAP_PLANE), *g) for g in R.RECT_GRIDS])
    for k in ("x", "y", "w", "h"):
        np.testing.assert_array_equal(items[k], ref[k], err_msg=k)
    np.testing.assert_array_equal(R.categories(p, items), ref["category"], err_msg="numpy reference")
    np.testing.assert_array_equal(oracle.classify(p, items.astype(oracle.ITEM_DTYPE))["category"], ref["category"],
                                  err_msg="oracle")
    np.testing.assert_array_equal(F.preclassify(p, items)["category"], ref["category"], err_msg="frac_classify")


# ---- what the case set has to contain ---------------------------------------------------------------------------

@pytest.mark.parametrize("path", [R.ROWS, R.PAIR, R.SUMS, R.AUTO])
def test_every_key_occurs_on_every_path(path):
    seen = np.zeros(7, np.int64)
    for c in R.CASES:
        if c.path == path:
            for k in R.expected(c.name):
                seen += np.bincount(k, minlength=7)
    assert (seen > 0).all(), seen


def test_wave_kernel_cases_cover_every_key():
    seen = np.zeros(7, np.int64)
    for c in R.CASES:
        if c.path == R.ROWS:
            for items, k in zip(c.grids(), R.expected(c.name)):
                if len(items) and items["h"][0] > 64:
                    seen += np.bincount(k, minlength=7)
    assert (seen > 0).all(), seen


def _wrap_change(items):
    p = R.plane(R.WRAP_PLANE)
    return R.categories(p, items) != R.categories(p, items, wrap=False)


def test_wrap_cases_wrap_and_the_control_does_not():
    W, H = R.plane_size(R.WRAP_PLANE)
    for g in R.WRAP_GRIDS:
        ch = _wrap_change(R.grid(W, H, *g))
        assert 4 * ch.sum() >= len(ch) and len(ch) >= 40, (g, int(ch.sum()), len(ch))
    ctl = _wrap_change(R.grid(W, H, *R.CONTROL_GRID))
    assert len(ctl) == 40 and not ctl.any()
    # the tagged sides of the cases are such grids
    tagged = 0
    for c in R.CASES:
        for side, items in zip("dr", c.grids()):
            if "wrap_" + side in c.tags:
                ch = _wrap_change(items)
                assert c.src == R.WRAP_PLANE and c.tgt is None and 4 * ch.sum() >= len(ch), c.name
                tagged += 1
            if "control_" + side in c.tags:
                assert not _wrap_change(items).any() and (items["w"] // 2 == 17).all(), c.name
                tagged += 1
    assert tagged == 6
    # the wrap reaches the row kernels (≤ 64 rows), the one-wave kernel (> 64) and both orders of the pair
    heights = {(c.path, int(items["h"][0])) for c in R.CASES for side, items in zip("dr", c.grids())
               if "wrap_" + side in c.tags}
    assert {(R.ROWS, 64), (R.ROWS, 128), (R.PAIR, 64), (R.AUTO, 64)} <= heights


def test_two_valued_plane_ties():
    """Constant 2×2 blocks of two values: at least 10 % category −1 among the items whose quadrant sums are not
    all equal, at some size."""
    best = 0.0
    for pl, g in R.CLASSIFY_CASES:
        if pl.startswith("two"):
            items = R.grid(*R.plane_size(pl), *g)
            sums = R.quadrant_sums(R.plane(pl), items)
            nonflat = (sums != sums[:, :1]).any(axis=1)
            cat = R.categories(R.plane(pl), items)
            assert nonflat.sum() >= 100
            best = max(best, float((cat[nonflat] == -1).mean()))
    assert best >= 0.10, best
    # and on every path a key-kernel case on such a plane has both: ties in a tenth of its domains, and orders
    for path in (R.ROWS, R.PAIR, R.SUMS):
        assert any(10 * (kd == 0).sum() >= len(kd) and (kd != 0).any()
                   for c in R.CASES if c.path == path and c.src.startswith("two")
                   for kd in R.expected(c.name)[:1]), path


def test_row_kernel_cases_cover_every_lane_count_and_edge():
    """keys_rows_item<L>: every L = 2..64 at its exact height and a rounded-up one, with row pointers 4-aligned
    and not, half widths a multiple of 4 and not, a count of 1 and a partial last workgroup."""
    by_L = {}
    for c in R.CASES:
        if c.path != R.ROWS:
            continue
        for items in c.grids():
            h = int(items["h"][0])
            if h > 64:
                continue
            e = by_L.setdefault(R.lanes_of(h), {"h": set(), "n1": False, "partial": False, "dword": False,
                                                "byte_hw": False, "byte_ptr": False})
            e["h"].add(h)
            e["n1"] |= len(items) == 1
            e["partial"] |= (len(items) * R.lanes_of(h)) % 256 != 0 and len(items) * R.lanes_of(h) > 256
            hw4 = (items["w"] // 2) % 4 == 0
            al = items["x"] % 4 == 0  # the device plane's rows are 64-byte aligned
            e["dword"] |= bool((hw4 & al).any())
            e["byte_hw"] |= bool((~hw4).any())
            e["byte_ptr"] |= bool((hw4 & ~al).any())
    assert sorted(by_L) == [2, 4, 8, 16, 32, 64]
    for L, e in by_L.items():
        assert L in e["h"] and (L == 2 or any(h < L for h in e["h"])), (L, e)
        assert all(e[k] for k in ("n1", "partial", "dword", "byte_hw", "byte_ptr")), (L, e)
    # the one-wave kernel: 1, 3, 4, 5 items around a workgroup's four
    counts = {len(items) for c in R.CASES if c.path == R.ROWS for items in c.grids() if items["h"][0] > 64}
    assert {1, 3, 4, 5} <= counts
    assert {65, 96, 128} <= {int(items["h"][0]) for c in R.CASES if c.path == R.ROWS for items in c.grids()}


def test_pair_cases_cover_whole_and_partial_domain_groups():
    """bucket_keys_rows2<2L, L>: nb0 = ⌈nd · 2L / 256⌉ workgroups of domains, full to the last lane and not."""
    seen = {}
    for c in R.CASES:
        d, r = c.grids()
        if c.path != R.PAIR or not len(d) or not len(r):
            continue
        dh, rh = int(d["h"][0]), int(r["h"][0])
        if dh == 2 * rh and rh in (4, 8, 16):
            seen.setdefault(rh, set()).add((len(d) * dh) % 256 == 0)
    assert seen == {4: {True, False}, 8: {True, False}, 16: {True, False}}, seen
    # and the pairs that fall through to two launches
    falls = {(int(c.grids()[0]["h"][0]), int(c.grids()[1]["h"][0])) for c in R.CASES if c.path == R.PAIR}
    assert {(4, 2), (64, 32)} <= falls


def test_block_sum_cases_cover_the_lattice_and_the_fallback():
    for pl in R.SUMS_PLANES:
        W, H = R.plane_size(pl)
        assert W % 32 or H % 32, "a partial wave of frame_block_sums"
        for q in (2, 4, 8, 16):
            if 2 * q > min(W, H):
                continue
            c = next(c for c in R.CASES if c.name == f"sums_{W}x{H}_q{q}")
            d, r = c.grids()
            assert len(d) == ((W - 2 * q) // q + 1) * ((H - 2 * q) // q + 1)  # every aligned square
            al = ((r["x"] | r["y"]) & (q - 1)) == 0
            assert al.any() and (~al).any(), c.name  # one grid, aligned and unaligned items
    assert any(R.plane_size(pl)[0] % 4 for pl in R.SUMS_PLANES), "a partial 4×4 block column"
    assert any(R.plane_size(pl)[1] % 4 for pl in R.SUMS_PLANES), "a partial 4×4 block row"
    assert any(min(R.plane_size(pl)) < 32 for pl in R.SUMS_PLANES)
    assert any(c.tgt and R.plane_size(c.tgt) != R.plane_size(c.src) for c in R.CASES if c.path == R.SUMS)
