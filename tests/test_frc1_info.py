"""frac_frc1_info (host only): an FRC1 header parsed and validated against the stream length, as
frac_decode_frc1 does before any kernel indexes a plane with the stream's fields.  Valid streams come
from codec.pack_stream over the committed goldens; every rejection rule of include/fracenc.h is
produced by editing one header field of a valid stream."""
import os
import struct
import subprocess

import pytest

import fractencode_amd as F
from fractencode_amd import codec
from golden_util import encode_items, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (golden, pack_stream keywords, expected record bits or None)
VALID = [
    ("crop64_t4", {}, 6 + 2 + 5 + 7),
    ("lenna_t4", {"contrast_bits": 5, "brightness_bits": 7}, 26),
    ("lenna_t4", {"contrast_bits": 7, "brightness_bits": 11}, 32),
    ("lenna_t4", {"contrast_bits": 9, "brightness_bits": 16}, 39),
    ("lenna_t8", {}, None),
    ("lenna_16to4", {"domain_size": 16}, None),
]


def _stream(name, **kw):
    rec, meta = golden(name)
    n = meta["tgt"]
    items = encode_items(rec, n)
    side = int(round(len(items) ** 0.5)) * n
    return codec.pack_stream(items, side, side, n, transforms=meta["T"], use_classifier=meta["cls"], **kw)


@pytest.mark.parametrize("name,kw,bits", VALID, ids=[f"{n}-{b}" for n, _, b in VALID])
def test_info_equals_read_header(name, kw, bits):
    buf = _stream(name, **kw)
    info = F.frc1_info(buf)
    h = codec.read_header(buf)
    assert set(info) == (set(h) - {"magic", "version"}) | {"record_bits", "body_bytes"}
    for k, v in h.items():
        if k not in ("magic", "version"):
            assert info[k] == v, k
    t_bits = max(1, (h["transforms"] - 1).bit_length())
    want = h["index_bits"] + t_bits + h["contrast_bits"] + h["brightness_bits"]
    assert info["record_bits"] == want and (bits is None or want == bits)
    assert info["body_bytes"] == (h["n_ranges"] * want + 7) // 8 == len(buf) - codec.HEADER.size
    if name == "lenna_t8":
        assert t_bits == 3
    if name == "lenna_16to4":
        assert (info["domain_size"], info["domain_stride"], info["range_size"]) == (16, 8, 4)


def _edit(buf, offset, fmt, value):
    b = bytearray(buf)
    struct.pack_into(fmt, b, offset, value)
    return bytes(b)


# one header field at a time: (rule, offset, struct format, value or function of the valid header)
EDITS = [
    ("magic", 0, "<4s", b"XRC1"),
    ("version", 4, "<H", 2),
    ("zero width", 8, "<I", 0),
    ("zero height", 12, "<I", 0),
    ("zero range size", 16, "<I", 0),
    ("domain size below 2", 20, "<I", 1),
    ("odd domain size", 20, "<I", lambda h: h["domain_size"] + 1),
    ("stride not half the size", 24, "<I", lambda h: h["domain_stride"] + 1),
    ("transforms 0", 28, "<B", 0),
    ("transforms 9", 28, "<B", 9),
    ("contrast bits 1", 29, "<B", 1),
    ("contrast bits 25", 29, "<B", 25),
    ("brightness bits 1", 30, "<B", 1),
    ("brightness bits 25", 30, "<B", 25),
    ("index bits", 31, "<B", lambda h: h["index_bits"] + 1),
    ("range count", 32, "<I", lambda h: h["n_ranges"] + 1),
    ("domain count", 36, "<I", lambda h: h["n_domains"] + 1),
    ("nan contrast min", 40, "<d", float("nan")),
    ("inf contrast max", 48, "<d", float("inf")),
    ("-inf brightness min", 56, "<d", float("-inf")),
    ("nan brightness max", 64, "<d", float("nan")),
]


@pytest.mark.parametrize("rule,offset,fmt,value", EDITS, ids=[e[0] for e in EDITS])
def test_info_rejects_header(rule, offset, fmt, value):
    buf = _stream("crop64_t4")
    h = codec.read_header(buf)
    F.frc1_info(buf)  # valid before the edit
    with pytest.raises(F.FracError):
        F.frc1_info(_edit(buf, offset, fmt, value(h) if callable(value) else value))


def test_info_rejects_wide_record():
    # 512², 2×2 ranges, 4×4 domains at stride 2: 65,025 domains → 16 index bits; T = 8 and 24 + 24 bits
    # make the record 16 + 3 + 48 = 67 bits, every other rule satisfied and the body present
    nr, nd = 256 * 256, 255 * 255
    hdr = codec.HEADER.pack(codec.MAGIC, codec.VERSION, 0, 512, 512, 2, 4, 2, 8, 24, 24, 16, nr, nd, 0.0, 1.0, 0.0, 1.0)
    with pytest.raises(F.FracError):
        F.frc1_info(hdr + bytes((nr * 67 + 7) // 8))
    # the same header at 20 + 24 bits (63-bit records) is accepted
    ok = codec.HEADER.pack(codec.MAGIC, codec.VERSION, 0, 512, 512, 2, 4, 2, 8, 20, 24, 16, nr, nd, 0.0, 1.0, 0.0, 1.0)
    assert F.frc1_info(ok + bytes((nr * 63 + 7) // 8))["record_bits"] == 63


def test_info_truncation_and_trailing_bytes():
    buf = _stream("crop64_t4")
    body = F.frc1_info(buf)["body_bytes"]
    assert len(buf) == 72 + body
    for cut in (0, 71, 72 + body - 1):
        with pytest.raises(F.FracError):
            F.frc1_info(buf[:cut])
    assert F.frc1_info(buf + b"\xff" * 5) == F.frc1_info(buf)
    assert F.last_error() != ""


def test_info_degenerate_field_is_valid():
    # min == max is how the packer stores a field whose values are all equal
    rec, meta = golden("crop64_t4")
    items = encode_items(rec, 8)
    items["contrast"] = 0.25
    info = F.frc1_info(codec.pack_stream(items, 64, 64, 8))
    assert info["contrast_min"] == info["contrast_max"] == 0.25


def test_cpp_layer_compiles(tmp_path):
    src = tmp_path / "frc1.cpp"
    src.write_text(
        '#include "fracenc.hpp"\n'
        "int use(fracenc::Engine& e, const std::vector<uint8_t>& s)\n"
        "{\n"
        "    const fracenc::Frc1Info i = fracenc::frc1_info(s.data(), s.size());\n"
        "    std::vector<uint8_t> plane;\n"
        "    const std::pair<int, double> r = e.decode_frc1(s, plane, 2, 10, 1e-5);\n"
        "    const std::pair<int, double> q = e.decode_frc1(s.data(), s.size(), plane);\n"
        "    return r.first + q.first + (int)i.record_bits + (int)i.body_bytes;\n"
        "}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)])
