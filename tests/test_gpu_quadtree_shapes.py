"""frac_encode_quadtree against the oracle's restatement of the same rule (oracle.quadtree) at small, odd
frames: the cases of quadtree_frames.py (test_quadtree_frames.py shows on the CPU that none is vacuous), on
the device-planned levels (ENGINE_AUTO), the host-planned levels (ENGINE_VALU) and the SEA engine under the
quadtree (host-planned; the tiled form at the 8-level for T = 4, per range otherwise).  Every field of every
leaf is the oracle's, bit for bit — the project's contract for these fields, so no tolerance — and so are the
summed counters the oracle can count.  Each engine is compared with the oracle, never with another engine."""
import numpy as np
import pytest

import fractencode_amd as F
import quadtree_frames as Q

pytestmark = pytest.mark.gpu

ENGINES = [F.ENGINE_AUTO, F.ENGINE_VALU, F.ENGINE_SEA]
ENGINE_IDS = {F.ENGINE_AUTO: "auto", F.ENGINE_VALU: "valu", F.ENGINE_SEA: "sea"}


def _ids(v):
    return v.name if isinstance(v, Q.Case) else ENGINE_IDS.get(v, str(v))


@pytest.fixture(scope="module")
def want(oracle):
    """The oracle's result per case, computed once and read-only: (records, sizes, stats, split, items)."""
    cache = {}

    def get(case):
        if case.name not in cache:
            recs, sizes, st, split = Q.run_oracle(oracle, case)
            items = Q.as_items(recs, sizes)
            for a in (recs, sizes, items):
                a.setflags(write=False)
            cache[case.name] = (recs, sizes, st, split, items)
        return cache[case.name]

    return get


def _engine(case, engine):
    return F.Engine(0, case.T, case.cls, case.thr, -1.0, engine)


def _set(e, case):
    src, tgt = case.planes()
    if tgt is None:
        e.set_frame(src)
    else:
        e.set_planes(src, tgt)


def _check(case, w, items, st):
    recs, sizes, ost, _, _ = w
    got = Q.as_oracle(items)
    assert len(items) == len(recs)
    for k in recs.dtype.names:
        if k != "pad":
            np.testing.assert_array_equal(got[k], recs[k], err_msg=f"{case.name}: {k}")
    np.testing.assert_array_equal(items["w"], sizes, err_msg=f"{case.name}: w")
    np.testing.assert_array_equal(items["h"], sizes, err_msg=f"{case.name}: h")
    assert st["items"] == len(recs)
    assert st["rejected_mappings"] == ost["rejected"]
    assert st["empty_ranges"] == ost["empty"]
    # every searched range against every domain of its level
    assert st["total_mappings"] == sum(c * Q.domain_count(case.W, case.H, n) for n, c in ost["searched"].items())


def _pinned(n, dt):
    import torch

    buf = torch.zeros(max(n, 1) * dt.itemsize, dtype=torch.uint8).pin_memory().numpy().view(dt)
    assert len(buf) == max(n, 1)
    return buf


def _cap(case):
    return max((case.W // case.min_size) * (case.H // case.min_size), 1)


@pytest.mark.parametrize("engine", ENGINES, ids=_ids)
@pytest.mark.parametrize("case", Q.ALL, ids=_ids)
def test_quadtree_equals_oracle(want, case, engine):
    w = want(case)
    with _engine(case, engine) as e:
        _set(e, case)
        items, st = e.encode_quadtree(case.max_size, case.min_size, w[3])
    _check(case, w, items, st)
    if engine == F.ENGINE_AUTO:
        assert st["engine"] == F.ENGINE_MFMA  # the device-planned levels
    if case.thr > 0:
        # a searched range is a hit exactly when its record's distance is within the threshold, and below the
        # split distance every hit is a leaf
        assert case.thr < w[3]
        assert st["hit_ranges"] == int((w[0]["dist"] <= case.thr).sum()) > 0


def test_sea_engine_runs_its_forms_under_the_quadtree(want):
    # (16, 8) at T = 4: the last level is the 8-level in the tiled form; (8, 2): the 2-level per range
    for case, form in ((Q.SEA_TILED, F.FORM_SEA_MFMA), (Q.BY_NAME["m98x74_8_2"], F.FORM_SEA)):
        with _engine(case, F.ENGINE_SEA) as e:
            _set(e, case)
            items, st = e.encode_quadtree(case.max_size, case.min_size, case.split)
        assert st["engine"] == F.ENGINE_SEA and st["search_form"] == form, case.name
        _check(case, want(case), items, st)
    # FLAG_SEA_PER_RANGE: the 8-level per range too, the same leaves
    case = Q.SEA_TILED
    with F.Engine(0, case.T, case.cls, case.thr, -1.0, F.ENGINE_SEA, flags=F.FLAG_SEA_PER_RANGE) as e:
        _set(e, case)
        items, st = e.encode_quadtree(case.max_size, case.min_size, case.split)
    assert st["search_form"] == F.FORM_SEA
    _check(case, want(case), items, st)


LEAF_CASES = Q.MIXED + Q.NODOM + Q.NORANGE


@pytest.mark.parametrize("engine", [F.ENGINE_AUTO, F.ENGINE_VALU], ids=_ids)
@pytest.mark.parametrize("case", LEAF_CASES, ids=_ids)
def test_32_byte_leaves(want, case, engine):
    recs, sizes, ost, split, items = want(case)
    expect = Q.leaves_from_records(items, case.W)
    pinned = _pinned(_cap(case) + 3, F.QT_LEAF)
    with _engine(case, engine) as e:
        _set(e, case)
        got, sg = e.encode_quadtree(case.max_size, case.min_size, split, leaves=True)
        pin, sp = e.encode_quadtree(case.max_size, case.min_size, split, out=pinned, leaves=True)
    assert got.dtype == F.QT_LEAF and len(got) == len(pin) == len(recs) == sg["items"] == sp["items"]
    np.testing.assert_array_equal(got, expect)
    np.testing.assert_array_equal(pin, expect)
    assert len(pin) == 0 or np.shares_memory(pin, pinned)
    assert not pinned[len(recs):].tobytes().strip(b"\0")  # nothing past the leaves
    np.testing.assert_array_equal(F.records_from_leaves(got, case.W), items)
    np.testing.assert_array_equal((got["code"] & 0xFFFFFF) == F.QT_NO_DOMAIN, recs["dw"] == 0)
    for s in (sg, sp):
        assert s["rejected_mappings"] == ost["rejected"] and s["empty_ranges"] == ost["empty"]


@pytest.mark.parametrize("leaves", [False, True], ids=["records", "leaves"])
@pytest.mark.parametrize("engine", [F.ENGINE_AUTO, F.ENGINE_VALU], ids=_ids)
def test_short_pinned_buffer_ends_inside_the_second_level(want, engine, leaves):
    case = Q.BY_NAME["m98x74_16_4"]
    recs, sizes, ost, split, items = want(case)
    expect = Q.leaves_from_records(items, case.W) if leaves else items
    n16, n8 = int((sizes == 16).sum()), int((sizes == 8).sum())
    m = n16 + n8 // 2
    assert n16 < m < n16 + n8 < len(recs)
    dt = F.QT_LEAF if leaves else F.ENCODE_ITEM
    pinned = _pinned(_cap(case), dt)
    with _engine(case, engine) as e:
        _set(e, case)
        part, st = e.encode_quadtree(case.max_size, case.min_size, split, out=pinned[:m], allow_short=True,
                                     leaves=leaves)
    assert st["items"] == len(recs) and len(part) == m and np.shares_memory(part, pinned)
    if leaves:
        np.testing.assert_array_equal(part, expect[:m])
    else:
        _check_prefix(part, expect[:m])
    assert not pinned[m:].tobytes().strip(b"\0")  # nothing past the capacity
    assert st["rejected_mappings"] == ost["rejected"] and st["empty_ranges"] == ost["empty"]


def _check_prefix(part, expect):
    for k in F.ENCODE_ITEM.names:
        if k != "_pad":
            np.testing.assert_array_equal(part[k], expect[k], err_msg=k)


@pytest.mark.parametrize("engine", [F.ENGINE_AUTO, F.ENGINE_VALU], ids=_ids)
@pytest.mark.parametrize("pad", [0, 5, 64])
def test_device_frame_with_padded_rows(want, pad, engine):
    import torch

    case = Q.BY_NAME["m98x74_16_4"]
    assert case.cls
    src, _ = case.planes()
    wide = torch.full((case.H, case.W + pad), 255, dtype=torch.uint8, device="cuda")
    wide[:, :case.W] = torch.from_numpy(src).cuda()
    view = wide[:, :case.W]
    assert view.stride(0) == case.W + pad and (pad == 0) == view.is_contiguous()
    with _engine(case, engine) as e:
        e.set_frame(view)
        items, st = e.encode_quadtree(case.max_size, case.min_size, case.split)
    _check(case, want(case), items, st)


@pytest.mark.parametrize("engine", ENGINES, ids=_ids)
def test_one_engine_across_frames(want, engine):
    # the cached level grids (qt_doms, qt_dvalid) and the buffers sized by an earlier, larger frame
    first = Q.SEQUENCE[0]
    with _engine(first, engine) as e:
        for case in Q.SEQUENCE:
            assert (case.T, case.cls, case.thr) == (first.T, first.cls, first.thr)
            w = want(case)
            _set(e, case)
            items, st = e.encode_quadtree(case.max_size, case.min_size, case.split)
            _check(case, w, items, st)
    lens = [len(want(c)[0]) for c in Q.SEQUENCE]
    assert lens[1] == 0 and lens[0] == lens[4] > 0 and lens[3] > lens[0]


def test_decode_of_an_odd_frame(oracle, want):
    case = Q.BY_NAME["m98x74_16_4"]
    recs, sizes, _, split, _ = want(case)
    with _engine(case, F.ENGINE_AUTO) as e:
        _set(e, case)
        items, st = e.encode_quadtree(case.max_size, case.min_size, split)
        dec, it, rms = e.decode(items, case.W, case.H)
    _check(case, want(case), items, st)
    wdec, wit, wrms = oracle.decode_sized(recs, sizes, case.W, case.H)
    assert (it, rms) == (wit, wrms)
    np.testing.assert_array_equal(dec, wdec)
    # the strip the first-level grid leaves uncovered stays as it was
    assert not dec[case.H // 16 * 16:].any() and not dec[:, case.W // 16 * 16:].any()
