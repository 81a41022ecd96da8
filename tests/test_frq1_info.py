"""frac_frq1_info (host only): an FRQ1 stream parsed, its split bitmaps walked and every section checked
against the stream length, as frac_decode_frq1 does before any kernel reads the body.  Valid streams come
from codec.pack_quadtree_stream over frq1_synth's partitions; every rejection rule of include/fracenc.h is
produced by editing one field or bit of a valid stream."""
import os
import struct
import subprocess

import pytest

import fractencode_amd as F
import frq1_synth as S
from fractencode_amd import codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(S.CASES))
@pytest.mark.parametrize("bits", [(5, 7), (24, 24)], ids=lambda b: f"{b[0]}+{b[1]}")
def test_info_equals_the_codec_walk(name, bits):
    buf = S.case_stream(name, *bits)
    info = F.frq1_info(buf)
    _, h = codec.unpack_quadtree_stream(buf)
    assert set(info) == set(h) - {"magic", "version"}
    for k in info:
        assert info[k] == h[k], k
    t_bits = 3
    for k in range(info["levels"]):
        assert info["record_bits"][k] == info["index_bits"][k] + t_bits + sum(bits)
        assert info["leaves"][k] <= info["nodes"][k]
    assert sum(info["leaves"]) == info["n_leaves"] and info["body_bytes"] == len(buf) - 64
    assert F.frq1_info(buf + b"\xff" * 5) == info  # trailing bytes are ignored


def _edit(buf, offset, fmt, value):
    b = bytearray(buf)
    struct.pack_into(fmt, b, offset, value)
    return bytes(b)


# one header field at a time: (rule, offset, struct format, value)
EDITS = [
    ("magic", 0, "<4s", b"FRC1"),
    ("version", 4, "<H", 2),
    ("zero width", 8, "<I", 0),
    ("zero height", 12, "<I", 0),
    ("width above 65535", 8, "<I", 65536),
    ("height above 65535", 12, "<I", 1 << 20),
    ("max size 32", 16, "<B", 32),
    ("max size 12", 16, "<B", 12),
    ("min size 1", 17, "<B", 1),
    ("min size 3", 17, "<B", 3),
    ("min above max", 16, "<B", 2),
    ("transforms 0", 18, "<B", 0),
    ("transforms 9", 18, "<B", 9),
    ("contrast bits 1", 19, "<B", 1),
    ("contrast bits 25", 19, "<B", 25),
    ("brightness bits 1", 20, "<B", 1),
    ("brightness bits 25", 20, "<B", 25),
    ("reserved byte 21", 21, "<B", 1),
    ("reserved byte 23", 23, "<B", 128),
    ("reserved word", 28, "<I", 1),
    ("leaf count + 1", 24, "<I", lambda h: h["n_leaves"] + 1),
    ("leaf count - 1", 24, "<I", lambda h: h["n_leaves"] - 1),
    ("nan contrast min", 32, "<d", float("nan")),
    ("inf contrast max", 40, "<d", float("inf")),
    ("-inf brightness min", 48, "<d", float("-inf")),
    ("nan brightness max", 56, "<d", float("nan")),
]


@pytest.mark.parametrize("rule,offset,fmt,value", EDITS, ids=[e[0] for e in EDITS])
def test_info_rejects_header(rule, offset, fmt, value):
    buf = S.case_stream("96x64")
    h = F.frq1_info(buf)  # valid before the edit
    edited = _edit(buf, offset, fmt, value(h) if callable(value) else value)
    with pytest.raises(F.FracError, match="FRQ1"):
        F.frq1_info(edited)
    assert F.last_error().startswith("FRQ1: ")
    with pytest.raises(ValueError):
        codec.unpack_quadtree_stream(edited)


def test_info_rejects_wide_record():
    # 1024², levels 16..2: the 2-level has 511² = 261,121 domains → 18 index bits; T = 8 and 24 + 24 bits make
    # its record 69 bits.  At 20 + 23 bits it is 64 and accepted (no level-0 node splits: 64² leaves of 16).
    def header(cb, bb, n_leaves):
        return codec.QT_HEADER.pack(codec.QT_MAGIC, 1, 0, 1024, 1024, 16, 2, 8, cb, bb, n_leaves, 0, 0.0, 1.0, 0.0, 1.0)

    n = 64 * 64
    bitmap = bytes(n // 8)
    with pytest.raises(F.FracError, match="wider than 64"):
        F.frq1_info(header(24, 24, n) + bitmap + bytes(n * 64 // 8 * 2))
    info = F.frq1_info(header(20, 23, n) + bitmap + bytes((n * (12 + 3 + 43) + 31) // 32 * 4))
    assert info["record_bits"] == [58, 60, 62, 64] and info["leaves"] == [n, 0, 0, 0]


def test_info_rejects_a_set_padding_bit():
    buf = S.case_stream("96x64")
    h = F.frq1_info(buf)
    assert h["nodes"][0] == 24  # bits 24..31 of the level-0 bitmap's dword are padding
    for bit in (24, 31):
        with pytest.raises(F.FracError, match="padding bit"):
            F.frq1_info(S.set_stream_bits(buf, h["bitmap_offset"][0], bit, 1, 1))
    assert h["nodes"][1] % 32 == 16
    with pytest.raises(F.FracError, match="padding bit"):
        F.frq1_info(S.set_stream_bits(buf, h["bitmap_offset"][1], h["nodes"][1], 1, 1))
    # a split bit changed inside the bitmap moves every later section: the leaf count no longer adds up
    with pytest.raises(F.FracError):
        F.frq1_info(S.set_stream_bits(buf, h["bitmap_offset"][0], 0, 1, 1 - (buf[h["bitmap_offset"][0]] & 1)))


def test_info_rejects_a_stream_cut_inside_a_section():
    buf = S.case_stream("96x64")
    h = F.frq1_info(buf)
    assert h["levels"] == 3 and all(h["leaves"][:3])
    cuts = {1: "header", 63: "header"}
    for k in range(3):
        if k < 2:
            cuts[h["bitmap_offset"][k] + 1] = "split bitmap"   # inside the level's bitmap
            cuts[h["record_offset"][k] - 1] = "split bitmap"
        cuts[h["record_offset"][k] + 1] = "record section"      # inside its records
        end = h["bitmap_offset"][k + 1] if k < 2 else len(buf)
        cuts[end - 1] = "record section"
    for cut, what in cuts.items():
        with pytest.raises(F.FracError, match=what):
            F.frq1_info(buf[:cut])
    # a cut exactly between two sections ends inside the next one
    with pytest.raises(F.FracError, match="record section"):
        F.frq1_info(buf[:h["record_offset"][1]])
    assert F.frq1_info(buf[:len(buf)]) == h


def test_info_needs_no_sections_for_a_leafless_frame():
    buf = S.case_stream("15x15_none")
    assert len(buf) == 64
    h = F.frq1_info(buf)
    assert h["n_leaves"] == 0 and h["body_bytes"] == 0 and h["nodes"] == [0, 0, 0, 0]
    assert h["n_domains"] == [0, 0, 4, 0] and h["index_bits"] == [1, 1, 3, 0]


def test_cpp_layer_compiles(tmp_path):
    src = tmp_path / "frq1.cpp"
    src.write_text(
        '#include "fracenc.hpp"\n'
        "int use(fracenc::Engine& e, const std::vector<frac_qt_leaf>& leaves)\n"
        "{\n"
        "    const std::vector<uint8_t> s = fracenc::pack_frq1(leaves, 96, 64, 16, 4, 8, true);\n"
        "    const fracenc::Frq1Info i = fracenc::frq1_info(s.data(), s.size());\n"
        "    std::vector<uint8_t> plane;\n"
        "    const std::pair<int, double> r = e.decode_frq1(s, plane, 2, 10, 1e-5);\n"
        "    const std::pair<int, double> q = e.decode_frq1(s.data(), s.size(), plane);\n"
        "    return r.first + q.first + (int)i.record_bits[0] + (int)i.body_bytes + (int)i.bitmap_offset[1];\n"
        "}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)])
