"""FRQ1 quadtree streams decoded on the device (frac_decode_frq1) and the encode → stream → pixels route.

Streams are made on the host (frq1_synth: seeded random partitions through codec.pack_quadtree_stream) or by
Engine.encode_quadtree_stream on the frames of quadtree_frames; the checker is the oracle's decode_sized over
codec.unpack_quadtree_stream's records, scaled — never the library's own item decoder.  Every comparison is
exact: stream bytes, plane bytes, iteration count and rms.  What the groups reach:

  frq1dec_level   one level without a bitmap; bitmaps of exactly one and four all-ones dwords; zero-byte
                  sections; a level of more than 1,024 nodes with split bits on both sides of node 1,024 (the
                  rank carry across dwords and workgroups); record sections that end in a partial dword
  frq1dec_step    leaves of 2..256 scaled pixels: two leaves inside one lane's dword, a 6-pixel leaf boundary
                  off dword alignment, leaves larger than the tile
  frq1dec_expand  margins, domain-less leaves, a level without domains, a leafless frame, the stepwise flag
"""
import ctypes as C
import functools

import numpy as np
import pytest

import fractencode_amd as F
import frq1_synth as S
import quadtree_frames as Q
from fractencode_amd import codec
from frc1_synth import fast_stream, oracle_decode_stream

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _engine(flags=0):
    """One context per flag set for the whole module: its buffers are reused across streams of different
    sizes, as a long-lived decoder's are."""
    return F.Engine(0, 8, flags=flags)


_stream = functools.lru_cache(maxsize=None)(S.case_stream)


def _initial(shape, seed=9):
    return np.random.default_rng(seed).integers(1, 256, shape, dtype=np.uint8)


def _same(got, want):
    assert (got[1], got[2]) == (want[1], want[2])
    np.testing.assert_array_equal(got[0], want[0])


def _check_stream(oracle, e, s, scale, max_iters=(-1, 5)):
    """decode_frq1 against the oracle: with and without an initial plane, unbounded and bounded."""
    h = codec.read_quadtree_header(s)
    init = _initial((scale * h["height"], scale * h["width"]))
    out = None
    for initial in (None, init):
        for m in max_iters:
            out = e.decode_frq1(s, scale=scale, max_iter=m, initial=initial)
            _same(out, S.oracle_decode_quadtree_stream(oracle, s, scale, m, initial))
    return out, init


def _is_fast(s):
    rec, h = codec.unpack_quadtree_stream(s)
    return (len(rec) > 0 and h["width"] % h["max_size"] == 0 and h["height"] % h["max_size"] == 0
            and bool((rec["sw"] != 0).all()))


# --- the fast path --------------------------------------------------------------------------------

FAST = [("96x64", (1, 2, 3)), ("48x32_to2", (1, 3, 16)), ("80x48_16_8", (1, 2)), ("24x40_8", (1, 2)),
        ("128x64_all", (1,)), ("128x64_none", (1,)), ("256x128_carry", (1, 2))]
FAST_CASES = [pytest.param(name, scale, id=f"{name}-x{scale}") for name, scales in FAST for scale in scales]


@pytest.mark.parametrize("name,scale", FAST_CASES)
def test_fast_path(oracle, name, scale):
    s = _stream(name)
    assert _is_fast(s)
    _check_stream(oracle, _engine(), s, scale)


def test_fast_path_stream_shapes():
    # the properties the cases above are kept for
    rec, h = codec.unpack_quadtree_stream(_stream("48x32_to2"))
    two = rec[rec["w"] == 2]
    assert len(two) and (two["x"] % 4 == 0).any() and (two["x"] % 4 == 2).any()  # scale 1: two leaves in one dword
    assert {3 * int(w) for w in set(rec["w"].tolist())} == {6, 12, 24, 48}       # scale 3: boundaries off 4
    assert {16 * int(w) for w in set(rec["w"].tolist())} == {32, 64, 128, 256}   # scale 16: beyond the 64×16 tile
    h = F.frq1_info(_stream("24x40_8"))
    assert h["levels"] == 1 and h["bitmap_offset"][0] == h["record_offset"][0]   # no bitmap
    s = _stream("128x64_all")
    h = F.frq1_info(s)
    assert h["nodes"] == [32, 128, 512, 0] and s[64:68] == b"\xff" * 4 and s[68:84] == b"\xff" * 16
    h = F.frq1_info(_stream("128x64_none"))
    assert h["nodes"] == [32, 0, 0, 0] and h["body_bytes"] == 4 + h["record_offset"][1] - h["record_offset"][0]
    s = _stream("256x128_carry")
    h = F.frq1_info(s)
    assert h["nodes"][1] > 1024 and h["nodes"][2] > 3000
    bits = np.unpackbits(np.frombuffer(s, np.uint8, (h["nodes"][1] + 7) // 8, h["bitmap_offset"][1]),
                         bitorder="little")[:h["nodes"][1]]
    assert bits[:1024].any() and bits[1024:].any()


def test_one_level_stream_equals_its_frc1_stream(oracle):
    # (8, 8): the partition is the uniform grid, so the same records as FRC1 decode to the same plane
    items = S.case_items("24x40_8")
    frc1 = codec.pack_stream(items, 24, 40, 8, transforms=8)
    e = _engine()
    for scale in (1, 2):
        init = _initial((40 * scale, 24 * scale))
        _same(e.decode_frq1(_stream("24x40_8"), scale=scale, initial=init), e.decode_frc1(frc1, scale=scale, initial=init))


# --- every other stream -----------------------------------------------------------------------------

def test_margins_keep_the_initial_plane(oracle):
    s = _stream("70x58_margins")
    assert not _is_fast(s)
    for scale in (1, 2):
        (plane, _, _), init = _check_stream(oracle, _engine(), s, scale)
        np.testing.assert_array_equal(plane[:, 64 * scale:], init[:, 64 * scale:])
        np.testing.assert_array_equal(plane[48 * scale:], init[48 * scale:])
        assert (plane[:48 * scale, :64 * scale] != init[:48 * scale, :64 * scale]).any()


def test_domainless_leaves(oracle):
    s = _stream("96x64_empty5")
    rec, _ = codec.unpack_quadtree_stream(s)
    tile = rec[(rec["x"] < 64) & (rec["y"] < 16)]
    assert 0 < int((tile["sw"] == 0).sum()) < len(tile)  # the 64×16 tile at the origin holds both kinds
    for scale in (1, 2):
        _check_stream(oracle, _engine(), s, scale)
    _check_stream(oracle, _engine(F.FLAG_DECODE_STEPWISE), s, 1, max_iters=(5,))


def test_level_without_domains(oracle):
    s = _stream("20x20_nodom")
    h = F.frq1_info(s)
    assert (h["n_leaves"], h["n_domains"][0], h["index_bits"][0]) == (1, 0, 1)
    (plane, _, _), init = _check_stream(oracle, _engine(), s, 2)
    np.testing.assert_array_equal(plane, init)


def test_leafless_stream_returns_the_initial_plane(oracle):
    s = _stream("15x15_none")
    assert len(s) == 64
    (plane, _, _), init = _check_stream(oracle, _engine(), s, 2)
    np.testing.assert_array_equal(plane, init)


def test_fast_stream_stepwise(oracle):
    for name, scale in (("96x64", 2), ("48x32_to2", 1)):
        _check_stream(oracle, _engine(F.FLAG_DECODE_STEPWISE), _stream(name), scale)


# --- records ------------------------------------------------------------------------------------------

def test_out_of_range_index_fails_before_the_plane(oracle):
    s = _stream("96x64")
    h = F.frq1_info(s)
    nd = h["n_domains"][1]
    assert nd + 1 < 1 << h["index_bits"][1]
    _, widths, bit = S.record_fields(s, h, 1, 3)
    bad = S.set_stream_bits(s, h["record_offset"][1], bit, widths[0], nd + 1)
    assert F.frq1_info(bad) == h  # the header and the sections are valid
    with pytest.raises(ValueError, match="out of range"):
        codec.unpack_quadtree_stream(bad)
    e = _engine()
    with pytest.raises(F.FracError, match="index out of range"):
        e.decode_frq1(bad)
    init = _initial((64, 96))
    plane, buf = init.copy(), np.frombuffer(bad, np.uint8)
    it, rms = C.c_int(-7), C.c_double(-7.0)
    rc = F.lib().frac_decode_frq1(e._ctx, buf.ctypes.data, len(buf), 1, -1, 1e-5, plane.ctypes.data, plane.size,
                                  C.byref(it), C.byref(rms))
    assert rc != 0 and it.value == -7 and rms.value == -7.0
    np.testing.assert_array_equal(plane, init)
    # index == nd is a leaf without a domain, not an error
    none = S.set_stream_bits(s, h["record_offset"][1], bit, widths[0], nd)
    _same(e.decode_frq1(none, initial=init), S.oracle_decode_quadtree_stream(oracle, none, initial=init))
    _same(e.decode_frq1(s, initial=init), S.oracle_decode_quadtree_stream(oracle, s, initial=init))


def test_tail_record_is_decoded(oracle):
    # the last record of a section that ends in a partial dword: its transform and brightness code rewritten must
    # change the decoded range, on the oracle and on the device alike
    s = _stream("80x48_16_8")
    h = F.frq1_info(s)
    k, last = 1, h["leaves"][1] - 1
    assert h["levels"] == 2 and (h["leaves"][k] * h["record_bits"][k]) % 32 != 0
    (_, t, _, qb), widths, bit = S.record_fields(s, h, k, last)
    assert h["record_offset"][k] + (bit + h["record_bits"][k] + 7) // 8 > len(s) - 4  # it reaches into the tail dword
    edited = S.set_stream_bits(s, h["record_offset"][k], bit + widths[0], widths[1], t ^ 1)
    edited = S.set_stream_bits(edited, h["record_offset"][k], bit + sum(widths[:3]), widths[3], qb ^ 0x40)
    rec = codec.unpack_quadtree_stream(s)[0][-1]
    box = np.s_[int(rec["y"]):int(rec["y"] + rec["h"]), int(rec["x"]):int(rec["x"] + rec["w"])]
    e = _engine()
    for m in (-1, 5):
        a = S.oracle_decode_quadtree_stream(oracle, s, max_iter=m)
        b = S.oracle_decode_quadtree_stream(oracle, edited, max_iter=m)
        assert (a[0][box] != b[0][box]).any()
        _same(e.decode_frq1(edited, max_iter=m), b)
        _same(e.decode_frq1(s, max_iter=m), a)


def test_one_engine_across_streams(oracle):
    # the decoders share the plane buffers, and the layout buffers keep an earlier, larger stream's contents
    with F.Engine(0, 8) as e:
        for name in ("256x128_carry", "48x32_to2", None, "256x128_carry"):
            if name is None:
                _same(e.decode_frc1(fast_stream(0)), oracle_decode_stream(oracle, fast_stream(0)))
            else:
                _check_stream(oracle, e, _stream(name), 1)


# --- encode → FRQ1 → pixels ---------------------------------------------------------------------------

END_TO_END = Q.MIXED + Q.EMPTY + Q.NODOM + [Q.SPLIT_ZERO, Q.TILE_CARRY]


@pytest.mark.parametrize("case", END_TO_END, ids=lambda c: c.name)
def test_encode_quadtree_stream(oracle, case):
    with F.Engine(0, case.T, case.cls, case.thr) as e:
        e.set_frame(case.planes()[0])
        stream, st = e.encode_quadtree_stream(case.max_size, case.min_size, case.split)
        leaves = e._qt_leaf_buf[:st["items"]].copy()  # the same call's leaves
        assert stream == codec.pack_quadtree_stream(F.records_from_leaves(leaves, case.W), case.W, case.H,
                                                    case.max_size, case.min_size, transforms=case.T,
                                                    use_classifier=case.cls)
        h = F.frq1_info(stream)
        assert h["n_leaves"] == st["items"] and h["flags"] == int(case.cls)
        for scale in (1, 2):
            _check_stream(oracle, e, stream, scale)
    _same(F.decode_stream(stream, scale=2), S.oracle_decode_quadtree_stream(oracle, stream, 2))
