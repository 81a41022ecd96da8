"""FRQ1 on the host: codec.pack_quadtree_stream / unpack_quadtree_stream (the layout's restatement) and
frac_pack_frq1 (the library's packer over 32-byte leaves), byte for byte.

The partitions are the oracle's quadtrees of quadtree_frames.ALL (the order frac_encode_quadtree emits) and
the seeded synthetic ones of frq1_synth.  Every comparison is exact."""
import functools

import numpy as np
import pytest

import fractencode_amd as F
import frq1_synth as S
import quadtree_frames as Q
from fractencode_amd import codec

GEOMETRY = ("x", "y", "w", "h", "dx", "dy", "sw", "sh", "transform")


@pytest.fixture(scope="module")
def run(oracle):
    @functools.lru_cache(maxsize=None)
    def get(name):
        recs, sizes, _, _ = Q.run_oracle(oracle, Q.BY_NAME[name])
        return Q.as_items(recs, sizes)

    return get


def _field(values, bits):
    f = codec._Field(values, bits)
    return np.full(len(values), f.min) if f.q is None else f.q.value(f.q.quantized(values))


def _check_roundtrip(items, stream, W, H, cb=5, bb=7):
    rec, h = codec.unpack_quadtree_stream(stream)
    assert len(rec) == len(items) == h["n_leaves"] == sum(h["leaves"])
    for k in GEOMETRY:
        np.testing.assert_array_equal(rec[k], items[k], err_msg=k)
    has = items["sw"] != 0
    np.testing.assert_array_equal(rec["contrast"], np.where(has, _field(items["contrast"], cb), 0.0))
    np.testing.assert_array_equal(rec["brightness"], np.where(has, _field(items["brightness"], bb), 0.0))
    assert (rec["distance"] == 0).all()
    assert len(stream) == codec.QT_HEADER.size + h["body_bytes"] and h["body_bytes"] % 4 == 0
    return rec, h


@pytest.mark.parametrize("case", Q.ALL, ids=lambda c: c.name)
def test_oracle_quadtrees_roundtrip(run, case):
    items = run(case.name)
    kw = dict(transforms=case.T, use_classifier=case.cls)
    stream = codec.pack_quadtree_stream(items, case.W, case.H, case.max_size, case.min_size, **kw)
    _, h = _check_roundtrip(items, stream, case.W, case.H)
    assert h["flags"] == int(case.cls) and h["levels"] == len(codec.quadtree_levels(case.max_size, case.min_size))
    # the library's packer over the 32-byte leaves
    assert F.pack_frq1(Q.leaves_from_records(items, case.W), case.W, case.H, case.max_size, case.min_size, **kw) == stream
    if case.name == "z15x15" or case.name.startswith("d15x40_"):
        assert len(items) == 0 and len(stream) == 64  # no level-0 node: the header alone
    if case.name == "d16x16_16_16":
        assert len(items) == 1 and h["n_domains"][0] == 0 and h["index_bits"][0] == 1
        assert (items["sw"] == 0).all() and len(stream) == 64 + 4


def test_bytes_per_leaf(run):
    # the rate the format is for: 3.3–3.6 bytes per leaf on the mixed frames, header included
    for name, leaves, size in (("t342x278_16_4", 3147, 10716), ("s98x74_zero", 1485, 4768)):
        case = Q.BY_NAME[name]
        stream = codec.pack_quadtree_stream(run(name), case.W, case.H, case.max_size, case.min_size,
                                            transforms=case.T, use_classifier=case.cls)
        assert (len(run(name)), len(stream)) == (leaves, size)


@pytest.mark.parametrize("name", list(S.CASES))
@pytest.mark.parametrize("bits", [(5, 7), (2, 16), (16, 2)], ids=lambda b: f"{b[0]}+{b[1]}")
def test_synthetic_partitions(name, bits):
    W, H, sizes, _, _ = S.CASES[name]
    items = S.case_items(name)
    stream = S.case_stream(name, *bits)
    _check_roundtrip(items, stream, W, H, *bits)
    assert F.pack_frq1(Q.leaves_from_records(items, W), W, H, sizes[0], sizes[-1], 8, False, *bits) == stream


def test_synthetic_partition_shapes():
    # the properties the synthetic cases are kept for
    h = {name: codec.unpack_quadtree_stream(S.case_stream(name))[1] for name in S.CASES}
    assert h["128x64_all"]["nodes"][:3] == [32, 128, 512] and h["128x64_all"]["leaves"][:3] == [0, 0, 512]
    s = S.case_stream("128x64_all")
    assert s[64:68] == b"\xff" * 4 and s[68 + 0:68 + 16] == b"\xff" * 16  # one all-ones dword, then four
    assert h["128x64_all"]["record_offset"][:2] == [68, 84]  # leafless levels: zero-byte record sections
    assert h["128x64_none"]["nodes"][:3] == [32, 0, 0]
    assert h["128x64_none"]["bitmap_offset"][1] == h["128x64_none"]["record_offset"][2] == len(S.case_stream("128x64_none"))
    c = h["256x128_carry"]
    assert c["nodes"][1] > 1024 and c["nodes"][2] > 3000
    bits = np.unpackbits(np.frombuffer(S.case_stream("256x128_carry"), np.uint8, (c["nodes"][1] + 7) // 8,
                                       c["bitmap_offset"][1]), bitorder="little")[:c["nodes"][1]]
    assert bits[:1024].any() and bits[1024:].any() and not bits.all()
    assert h["24x40_8"]["levels"] == 1 and h["24x40_8"]["bitmap_offset"][0] == h["24x40_8"]["record_offset"][0] == 64
    assert h["20x20_nodom"]["n_domains"][0] == 0 and h["20x20_nodom"]["index_bits"][0] == 1
    assert h["15x15_none"]["n_leaves"] == 0 and len(S.case_stream("15x15_none")) == 64
    m = S.case_items("70x58_margins")
    assert int((m["w"].astype(np.int64) ** 2).sum()) == 64 * 48 < 70 * 58
    e = S.case_items("96x64_empty5")
    assert 0 < int((e["sw"] == 0).sum()) < len(e)
    for name in ("96x64", "48x32_to2", "80x48_16_8"):
        W, H, sizes, _, _ = S.CASES[name]
        it = S.case_items(name)
        assert set(it["w"].tolist()) == set(sizes) and int((it["w"].astype(np.int64) ** 2).sum()) == W * H


def test_degenerate_fields():
    items = S.case_items("96x64")
    items["contrast"] = 0.25
    stream = codec.pack_quadtree_stream(items, 96, 64, 16, 4, transforms=8)
    rec, h = codec.unpack_quadtree_stream(stream)
    assert h["contrast_min"] == h["contrast_max"] == 0.25 and (rec["contrast"] == 0.25).all()
    assert F.pack_frq1(Q.leaves_from_records(items, 96), 96, 64, 16, 4, 8) == stream


def test_host_packer_refuses_what_is_not_canonical():
    items = S.case_items("96x64")
    for bad in (items[::-1], np.delete(items, 3), np.concatenate([items[:4], items[3:]])):
        with pytest.raises(ValueError):
            codec.pack_quadtree_stream(bad, 96, 64, 16, 4, transforms=8)


# --- frac_pack_frq1's refusals ------------------------------------------------------------------

def _pack(leaves, T=8, cb=5, bb=7, sizes=(16, 4), wh=(96, 64)):
    return F.pack_frq1(leaves, wh[0], wh[1], sizes[0], sizes[1], T, False, cb, bb)


def test_pack_frq1_refusals_leave_the_packer_usable():
    items = S.case_items("96x64")
    good = Q.leaves_from_records(items, 96)
    want = codec.pack_quadtree_stream(items, 96, 64, 16, 4, transforms=8)
    n16 = int((items["w"] == 16).sum())
    nd16 = Q.domain_count(96, 64, 16)

    def edited(fn):
        lv = good.copy()
        out = fn(lv)
        return lv if out is None else out

    def swap(lv):
        lv[[n16, n16 + 1]] = lv[[n16 + 1, n16]]  # two leaves of the 8-level

    def off_node(lv):
        lv["x"][n16] += 4  # a multiple of the finest size, but no node of the 8-level

    def index_at_count(lv):
        lv["code"][0] = (lv["code"][0] & ~np.uint32(0xFFFFFF)) | np.uint32(nd16)

    def transform(lv):
        lv["code"][0] = (lv["code"][0] & ~np.uint32(0xF << 24)) | np.uint32(5 << 24)

    def nan(lv):
        lv["contrast"][7] = np.nan

    def size_code(lv):
        lv["code"][-1] = (lv["code"][-1] & np.uint32(0x0FFFFFFF)) | np.uint32(1 << 28)  # a 2×2 leaf at (16, 4)

    bad = {
        "swapped": (edited(swap), {}, "canonical order"),
        "dropped": (np.delete(good, n16 + 2), {}, "canonical order"),
        "duplicated": (np.concatenate([good[:n16 + 1], good[n16:]]), {}, "canonical order"),
        "surplus": (np.concatenate([good, good[-1:]]), {}, "canonical order"),
        "non-node position": (edited(off_node), {}, "canonical order"),
        "size code": (edited(size_code), {}, "canonical order"),
        "index == nd": (edited(index_at_count), {}, "domain index"),
        "transform >= T": (edited(transform), {"T": 4}, "transform"),
        "nan contrast": (edited(nan), {}, "non-finite"),
        "1 contrast bit": (good, {"cb": 1}, r"\[2, 16\]"),
        "17 brightness bits": (good, {"bb": 17}, r"\[2, 16\]"),
        "size 3": (good, {"sizes": (16, 3)}, "sizes"),
        "min above max": (good, {"sizes": (4, 16)}, "sizes"),
        "zero width": (good, {"wh": (0, 64)}, "width"),
        "side above 65535": (good, {"wh": (65536, 64)}, "width"),
        "transforms 9": (good, {"T": 9}, "transforms"),
    }
    assert F.QT_NO_DOMAIN > nd16 > int(good["code"][0] & 0xFFFFFF)
    for rule, (leaves, kw, match) in bad.items():
        with pytest.raises(F.FracError, match=match):
            _pack(leaves, **kw)
        assert _pack(good) == want, rule
