"""FRC3, the colour container, on the host (CPU only): frac_pack_frc3's bytes against codec.pack_color_stream,
frac_frc3_info's fields against codec.unpack_color_stream, the size query, and every refusal of the header
comment in include/fracenc.h, one mutation each.  Plane streams are synthetic (frc1_synth / frq1_synth)."""
import ctypes as C
import struct

import numpy as np
import pytest

import fractencode_amd as F
from fractencode_amd import codec
from frc1_synth import synth_stream
from frq1_synth import synth_quadtree_stream

FRAMES = [(32, 32), (37, 27), (96, 64)]
KINDS = {"frc1": (1, 1, 1), "frq1": (2, 2, 2), "mixed": (2, 1, 2), "mixed2": (1, 2, 1)}


def plane_stream(kind: int, W: int, H: int, seed: int) -> bytes:
    if kind == 1:
        return synth_stream(W, H, 4, 8, 4, seed)
    return synth_quadtree_stream(W, H, seed, (8, 4), T=4)


def plane_streams(W: int, H: int, kinds, seed: int = 300) -> list:
    return [plane_stream(k, W if i == 0 else W // 2, H if i == 0 else H // 2, seed + i) for i, k in enumerate(kinds)]


def container(W=37, H=27, kinds=(1, 1, 2)) -> bytes:
    return codec.pack_color_stream(plane_streams(W, H, kinds), W, H)


@pytest.mark.parametrize("W,H", FRAMES)
@pytest.mark.parametrize("kinds", list(KINDS))
def test_pack_frc3_equals_the_host_restatement(W, H, kinds):
    streams = plane_streams(W, H, KINDS[kinds])
    got = F.pack_frc3(streams, W, H)
    want = codec.pack_color_stream(streams, W, H)
    assert got == want
    assert got[:4] == b"FRC3" and len(got) % 8 == 0
    back, h = codec.unpack_color_stream(got)
    assert back == streams
    info = F.frc3_info(got)
    assert info == h
    assert (info["width"], info["height"], info["flags"]) == (W, H, 0)
    assert tuple(info["kind"]) == KINDS[kinds]
    assert info["length"] == [len(s) for s in streams] and info["offset"][0] == 32
    for k in range(3):
        assert got[info["offset"][k]:info["offset"][k] + info["length"][k]] == streams[k]
        assert info["offset"][k] % 8 == 0
    assert info["total_bytes"] == len(got)
    # trailing bytes are ignored
    assert F.frc3_info(got + b"\x01\x02\x03") == info


def test_some_stream_needs_padding():
    # the zero padding is exercised: at least one synthetic stream's length is no multiple of 8
    s = container()
    info = F.frc3_info(s)
    assert any(n % 8 for n in info["length"])


def test_size_query_and_short_capacity():
    W, H = 37, 27
    streams = plane_streams(W, H, (1, 2, 1))
    want = codec.pack_color_stream(streams, W, H)
    bufs = [np.frombuffer(s, np.uint8) for s in streams]
    ptrs = (C.c_void_p * 3)(*[b.ctypes.data for b in bufs])
    lens = (C.c_size_t * 3)(*[len(b) for b in bufs])
    n = C.c_size_t(0)
    assert F.lib().frac_pack_frc3(ptrs, lens, W, H, None, 0, C.byref(n)) == 0
    assert n.value == len(want)
    cap = 100
    out = np.full(cap + 8, 0xEE, np.uint8)
    n = C.c_size_t(0)
    assert F.lib().frac_pack_frc3(ptrs, lens, W, H, out.ctypes.data_as(C.c_void_p), cap, C.byref(n)) == 0
    assert n.value == len(want) and out[:cap].tobytes() == want[:cap] and (out[cap:] == 0xEE).all()


def put_u32(s: bytes, off: int, v: int) -> bytes:
    return s[:off] + struct.pack("<I", v) + s[off + 4:]


def refusals():
    s = container()
    info = codec.unpack_color_stream(s)[1]
    oy, ou, ov = info["offset"]
    ly, lu, lv = info["length"]
    W, H = 37, 27
    pad_at = next(info["offset"][k] + info["length"][k] for k in range(3) if info["length"][k] % 8)
    wrong_u = codec.pack_color_stream(plane_streams(W, H, (1, 1, 2)), W, H)
    # the U section replaced by a stream of another frame size (same container otherwise valid)
    streams = plane_streams(W, H, (1, 1, 2))
    other_u = plane_stream(1, W // 2 + 1, H // 2, 77)
    head = codec.COLOR_HEADER.pack(b"FRC3", 1, 0, W, H, len(streams[0]), len(other_u), len(streams[2]), 0)
    wrong_u = head + b"".join(x + bytes(-len(x) % 8) for x in (streams[0], other_u, streams[2]))
    other_y = plane_stream(1, W, H + 1, 78)
    head = codec.COLOR_HEADER.pack(b"FRC3", 1, 0, W, H, len(other_y), len(streams[1]), len(streams[2]), 0)
    wrong_y = head + b"".join(x + bytes(-len(x) % 8) for x in (other_y, streams[1], streams[2]))
    return {
        "short": s[:31],
        "magic": b"FRC1" + s[4:],
        "version": s[:4] + struct.pack("<H", 2) + s[6:],
        "flags": s[:6] + struct.pack("<H", 1) + s[8:],
        "reserved": put_u32(s, 28, 1),
        "width_1": put_u32(s, 8, 1),
        "height_65536": put_u32(s, 12, 65536),
        "section_past_len": s[:-8],
        "len_v_huge": put_u32(s, 24, 0xFFFFFFF0),
        "padding_byte": s[:pad_at] + b"\x01" + s[pad_at + 1:],
        "inner_magic": s[:ou] + b"FRX1" + s[ou + 4:],
        "inner_header": put_u32(s, oy + 16, 0),            # the Y stream's range_size = 0: frac_frc1_info refuses it
        "inner_frq1_header": s[:ov + 16] + b"\x03" + s[ov + 17:],  # the V stream's max_size = 3
        "inner_truncated": put_u32(s, 16, ly - 1),         # the Y stream one byte short of its records
        "y_size": wrong_y,
        "u_size": wrong_u,
        "header_size_not_streams": put_u32(s, 8, W + 2),   # header 39×27: Y no longer the frame, chroma still 18 wide
    }


REFUSALS = refusals()


def test_the_unmutated_container_is_accepted():
    s = container()
    assert F.frc3_info(s)["total_bytes"] == len(s)


@pytest.mark.parametrize("name", list(REFUSALS))
def test_frc3_info_refuses(name):
    s = REFUSALS[name]
    buf = np.frombuffer(s, np.uint8)
    out = F.FracFrc3Info()
    assert F.lib().frac_frc3_info(buf.ctypes.data, len(buf), C.byref(out)) == -1  # FRAC_E_INVALID
    assert F.last_error()
    with pytest.raises(F.FracError):
        F.frc3_info(s)
    with pytest.raises(ValueError):
        codec.unpack_color_stream(s)


def test_pack_frc3_refuses():
    W, H = 37, 27
    good = plane_streams(W, H, (1, 1, 2))
    F.pack_frc3(good, W, H)
    cases = {
        "width_1": (good, 1, H),
        "height_65536": (good, W, 65536),
        "y_size": ([plane_stream(1, W, H + 1, 78), good[1], good[2]], W, H),
        "u_size": ([good[0], plane_stream(1, W // 2 + 1, H // 2, 77), good[2]], W, H),
        "v_size": ([good[0], good[1], plane_stream(2, W // 2, H // 2 + 1, 79)], W, H),
        "inner_magic": ([good[0], b"FRX1" + good[1][4:], good[2]], W, H),
        "inner_header": ([put_u32(good[0], 16, 0), good[1], good[2]], W, H),
        "inner_truncated": ([good[0][:-1], good[1], good[2]], W, H),
        "empty_stream": ([good[0], b"", good[2]], W, H),
    }
    for name, (streams, w, h) in cases.items():
        with pytest.raises(F.FracError):
            F.pack_frc3(streams, w, h)
        with pytest.raises(ValueError):
            codec.pack_color_stream(streams, w, h)
    with pytest.raises(F.FracError):
        F.pack_frc3(good[:2], W, H)
