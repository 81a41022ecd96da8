"""Every classifier-key kernel of fracenc_bucket.hip against the plain reference of tests/classifier_ref.py,
through the test hook frac_debug_bucket_keys (F.debug_bucket_keys): keys_rows_item<L> at every L with its dword and
byte loads, bucket_keys (one wave per item above 64 rows), the paired launch bucket_keys_rows2, and bucket_keys_bs on
the frame_block_sums pyramid with its in-thread fallback — at the shapes where each branches, and on items whose
quadrant sums wrap the reference's uint16_t.  classify_items (Engine.classify) runs on the rectangular, wrapping,
odd-sized and tied items too.  Every comparison is exact; tests/test_classifier_ref.py pins the reference and the
case set."""
import numpy as np
import pytest

import classifier_ref as R
import fractencode_amd as F

pytestmark = pytest.mark.gpu

assert (R.AUTO, R.ROWS, R.PAIR, R.SUMS) == (F.KEYS_AUTO, F.KEYS_ROWS, F.KEYS_PAIR, F.KEYS_BLOCK_SUMS)
UNWRITTEN = 0xFFFFFFFF  # F.debug_bucket_keys fills its outputs with it


def _set_planes(e, case):
    s, t = case.planes()
    if case.tgt is None:
        e.set_frame(s)
    else:
        e.set_planes(s, t)


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_keys_match_the_reference(case):
    d, r = case.grids()
    wd, wr = R.expected(case.name)
    assert len(d) and len(r)
    with F.Engine(0) as e:
        _set_planes(e, case)
        gd, gr = F.debug_bucket_keys(e, d, r, case.path)
        np.testing.assert_array_equal(gd, wd, err_msg="domain keys")
        np.testing.assert_array_equal(gr, wr, err_msg="range keys")
        # the run's own choice is the path it should have taken
        for tag, path in (("as_sums", F.KEYS_BLOCK_SUMS), ("as_pair", F.KEYS_PAIR)):
            if tag in case.tags:
                od, orr = F.debug_bucket_keys(e, d, r, path)
                np.testing.assert_array_equal(gd, od)
                np.testing.assert_array_equal(gr, orr)
        # one side alone (the other empty): the same keys
        ad, ar = F.debug_bucket_keys(e, d, r[:0], case.path)
        np.testing.assert_array_equal(ad, wd, err_msg="domains alone")
        assert ar.size == 0
        bd, br = F.debug_bucket_keys(e, d[:0], r, case.path)
        np.testing.assert_array_equal(br, wr, err_msg="ranges alone")
        assert bd.size == 0


@pytest.mark.parametrize("pad,start", [(0, 0), (5, 1), (64, 2)])
def test_block_sums_of_device_frames(pad, start):
    """Frames given as device tensors with padded rows and an unaligned start: the plane the pyramid is built
    from is the library's own aligned copy, whatever the caller's layout."""
    import torch

    name = "noise51_100x36"
    p = R.plane(name)
    H, W = p.shape
    buf = torch.full((start + H * (W + pad) + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(buf, (H, W), (W + pad, 1), start)
    view.copy_(torch.from_numpy(p.copy()).cuda())
    with F.Engine(0) as e:
        e.set_frame(view)
        for q in (2, 4, 8, 16):
            d, r = R.grid(W, H, 2 * q, q), R.grid(W, H, 2 * q, q + 1, (1, 0))
            gd, gr = F.debug_bucket_keys(e, d, r, F.KEYS_BLOCK_SUMS)
            np.testing.assert_array_equal(gd, R.keys(p, d), err_msg=f"q = {q}: domains")
            np.testing.assert_array_equal(gr, R.keys(p, r), err_msg=f"q = {q}: ranges")


@pytest.mark.parametrize("pl,g", R.CLASSIFY_CASES, ids=[f"{pl}-{g}" for pl, g in R.CLASSIFY_CASES])
def test_classify_items_matches_the_reference(pl, g):
    p = R.plane(pl)
    items = R.grid(*R.plane_size(pl), *g)
    with F.Engine(0) as e:
        e.set_frame(p)
        got = e.classify(items)
    np.testing.assert_array_equal(got["category"], R.categories(p, items))
    for k in ("x", "y", "w", "h"):
        np.testing.assert_array_equal(got[k], items[k])


STORED = ["rows_h9_a", "rows_h64_b", "wave_wrap_32x128", "pair_16to8", "pair_64x16_32x8", "pair_64to32",
          "sums_130x70_q4", "sums_130x70_rect", "auto_16to8", "auto_128to64"]


@pytest.mark.parametrize("name", STORED)
def test_stored_categories_pass_through(name):
    case = next(c for c in R.CASES if c.name == name)
    d, r = case.grids()
    for k, items in enumerate((d, r)):  # −1, 0 … 5 in turn: a stored category is the key, −1 is classified
        items["category"] = (np.arange(len(items)) + k) % 7 - 1
    s, t = case.planes()
    wd, wr = R.keys(s, d), R.keys(t, r)
    stored = d["category"] != -1
    np.testing.assert_array_equal(wd[stored], d["category"][stored] + 1)
    with F.Engine(0) as e:
        _set_planes(e, case)
        gd, gr = F.debug_bucket_keys(e, d, r, case.path)
    np.testing.assert_array_equal(gd, wd)
    np.testing.assert_array_equal(gr, wr)


def _raw(e, d, r, path):
    """The hook without the wrapper: (return code, domain keys, range keys)."""
    kd, kr = np.full(len(d), UNWRITTEN, np.uint32), np.full(len(r), UNWRITTEN, np.uint32)
    rc = F.lib().frac_debug_bucket_keys(e._ctx, d.ctypes.data, len(d), r.ctypes.data, len(r), path, kd.ctypes.data,
                                        kr.ctypes.data)
    return rc, kd, kr


def test_refusals_leave_the_context_usable():
    """Every refusal comes before any launch (nothing is written), and the next valid call is correct."""
    E_INVALID = -1
    src, tgt = R.plane("noise61_100x36"), R.plane("value62_37x29")
    d8, r4 = R.grid(100, 36, 8, 4), R.grid(37, 29, 4, 4)
    wd, wr = R.keys(src, d8), R.keys(tgt, r4)

    def edit(items, i, **kw):
        out = items.copy()
        for k, v in kw.items():
            out[k][i] = v
        return out

    mixed_d = np.concatenate([d8, R.grid(100, 36, 16, 8)])
    mixed_r = np.concatenate([r4, R.grid(37, 29, (4, 6), (4, 6))])
    refused = [
        ("domain past the right edge", edit(d8, -1, x=93), r4, (0, 1, 2, 3)),
        ("domain past the bottom edge", edit(d8, 3, y=29), r4, (0, 1, 2, 3)),
        ("domain x wraps 32 bits", edit(d8, 0, x=0xFFFFFFFC), r4, (0, 1, 2, 3)),
        ("domain size wraps 32 bits", edit(d8, 0, w=0xFFFFFFF8, x=8), r4, (0, 1, 2, 3)),
        ("range outside the smaller target plane", d8, edit(r4, -1, x=34), (0, 1, 2, 3)),
        ("range inside the source but outside the target", d8, edit(r4, 0, x=60), (0, 1, 2, 3)),
        ("domain category 6", edit(d8, 5, category=6), r4, (0, 1, 2, 3)),
        ("range category -2", d8, edit(r4, 7, category=-2), (0, 1, 2, 3)),
        ("domains of two sizes", mixed_d, r4, (1, 2)),
        ("ranges of two heights", d8, mixed_r, (1, 2)),
        ("path 4", d8, r4, (4, -1)),
    ]
    with F.Engine(0) as e:
        rc, kd, kr = _raw(e, d8, r4, 0)
        assert rc == E_INVALID and (kd == UNWRITTEN).all() and (kr == UNWRITTEN).all(), "no plane set"
        e.set_planes(src, tgt)
        for what, d, r, paths in refused:
            for path in paths:
                rc, kd, kr = _raw(e, d, r, path)
                assert rc == E_INVALID, f"{what}, path {path}"
                assert F.last_error(e._ctx), what
                assert (kd == UNWRITTEN).all() and (kr == UNWRITTEN).all(), f"{what}: written before the refusal"
                with pytest.raises(F.FracError):
                    F.debug_bucket_keys(e, d, r, path)
                gd, gr = F.debug_bucket_keys(e, d8, r4, path if 0 <= path <= 3 else 0)
                np.testing.assert_array_equal(gd, wd, err_msg=f"after {what}")
                np.testing.assert_array_equal(gr, wr, err_msg=f"after {what}")
        # grids of two sizes are fine where every item is summed on its own: the block sums
        gd, gr = F.debug_bucket_keys(e, mixed_d, mixed_r, F.KEYS_BLOCK_SUMS)
        np.testing.assert_array_equal(gd, R.keys(src, mixed_d))
        np.testing.assert_array_equal(gr, R.keys(tgt, mixed_r))


def test_hook_changes_nothing_a_run_reads():
    """A prepared classified context searches the same after the hook ran on other grids, on every path."""
    p = R.plane("value63_130x70")
    doms, rngs = F.create_uniform_grid(130, 70, 16, 8), F.create_uniform_grid(130, 70, 8, 8)
    with F.Engine(0, 4, True) as e:
        e.set_frame(p)
        e.set_domains(doms)
        out0, st0 = e.search(rngs)
        for path, (d, r) in ((0, (R.grid(130, 70, 8, 4), R.grid(130, 70, 4, 4))),
                             (1, (R.grid(130, 70, (20, 66), 9), R.grid(130, 70, (6, 5), 3))),
                             (2, (R.grid(130, 70, 32, 16), R.grid(130, 70, 16, 16))),
                             (3, (R.grid(130, 70, 32, 16), R.grid(130, 70, 12, 5)))):
            gd, gr = F.debug_bucket_keys(e, d, r, path)
            np.testing.assert_array_equal(gd, R.keys(p, d))
            np.testing.assert_array_equal(gr, R.keys(p, r))
            out1, st1 = e.fetch()  # the last run's records are still there
            assert out1.tobytes() == out0.tobytes()
            e.run()
            out2, st2 = e.fetch()
            assert out2.tobytes() == out0.tobytes()
            assert st2["rejected_mappings"] == st0["rejected_mappings"] == st1["rejected_mappings"]
