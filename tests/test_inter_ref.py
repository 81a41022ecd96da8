"""CPU checks of the inter-frame reference (inter_ref.py) and of the FRCS sequence container (codec.pack_sequence /
unpack_sequence).

The reference is the oracle's decoder on a stacked plane; what makes it the definition of one application is checked
here for every stream the device tests use: the top half stays the reference plane, and two, three and four passes
give the same bottom half."""
import struct

import numpy as np
import pytest

import frc1_synth as S1
import frq1_synth as SQ
import inter_ref as R
from fractencode_amd import codec

FRC1 = [pytest.param(S1.fast_stream, k, id=f"fast{k}") for k in range(5)] + \
       [pytest.param(S1.other_stream, k, id=f"other{k}") for k in range(6)]
FRQ1 = [pytest.param(SQ.case_stream, name, id=name) for name in SQ.CASES]


@pytest.mark.parametrize("scale", [1, 3])
@pytest.mark.parametrize("make,key", FRC1 + FRQ1)
def test_stacked_decode_is_one_application(oracle, make, key, scale):
    rec, W, H, _ = R.stream_records(make(key), scale)
    ref = R.random_plane(W, H, 7)
    two = R.stacked(oracle, rec, W, H, ref, 2)
    np.testing.assert_array_equal(two[:H], ref)
    for passes in (3, 4):
        np.testing.assert_array_equal(R.stacked(oracle, rec, W, H, ref, passes), two)
    # pixels no range with a domain covers keep the reference
    covered = np.zeros((H, W), bool)
    for r in rec[rec["sw"] != 0]:
        covered[int(r["y"]):int(r["y"] + r["h"]), int(r["x"]):int(r["x"] + r["w"])] = True
    np.testing.assert_array_equal(two[H:][~covered], ref[~covered])
    if covered.any():
        assert (two[H:][covered] != ref[covered]).any()


def test_the_pass_reads_the_reference_not_the_plane(oracle):
    # a stream applied to two references that differ inside one domain patch only differs exactly in the ranges
    # that read that patch
    s = SQ.case_stream("96x64")
    rec, W, H, _ = R.stream_records(s)
    a = R.random_plane(W, H, 3)
    b = a.copy()
    d = rec[0]
    box = np.s_[int(d["dy"]):int(d["dy"] + d["sh"]), int(d["dx"]):int(d["dx"] + d["sw"])]
    b[box] ^= 0x80
    pa, pb = R.apply_stream(oracle, s, a), R.apply_stream(oracle, s, b)
    touched = np.zeros((H, W), bool)
    for r in rec:
        if r["dx"] < d["dx"] + d["sw"] and d["dx"] < r["dx"] + r["sw"] and r["dy"] < d["dy"] + d["sh"] and \
                d["dy"] < r["dy"] + r["sh"]:
            touched[int(r["y"]):int(r["y"] + r["h"]), int(r["x"]):int(r["x"] + r["w"])] = True
    assert touched[int(d["y"]), int(d["x"])]
    np.testing.assert_array_equal(pa[~touched], pb[~touched])
    assert (pa[touched] != pb[touched]).any()


# --- FRCS -----------------------------------------------------------------------------------------------

def _frames():
    return [("I", SQ.case_stream("96x64")), ("P", SQ.case_stream("96x64_empty5")),
            ("P", S1.synth_stream(96, 64, 8, 16, 8, 5)), ("I", SQ.case_stream("96x64", contrast_bits=6))]


def test_sequence_round_trip():
    frames = _frames()
    data = codec.pack_sequence(frames, 96, 64)
    assert data[:4] == b"FRCS" and len(data) % 8 == (20 + 8 * len(frames)) % 8
    got, h = codec.unpack_sequence(data)
    assert got == frames
    assert (h["width"], h["height"], h["flags"], h["frames"], h["total_bytes"]) == (96, 64, 0, 4, len(data))
    assert h["length"] == [len(s) for _, s in frames]
    assert h["offset"][0] == 20 + 8 * len(frames)
    for k in range(1, 4):
        assert h["offset"][k] == h["offset"][k - 1] + h["length"][k - 1] + (-h["length"][k - 1] % 8)
    for (_, s), off in zip(frames, h["offset"]):
        assert data[off:off + len(s)] == s
    assert any(len(s) % 8 for _, s in frames)  # some stream is padded
    # an empty sequence and a lone I frame
    assert codec.unpack_sequence(codec.pack_sequence([], 96, 64))[0] == []
    assert codec.unpack_sequence(codec.pack_sequence(frames[:1], 96, 64))[0] == frames[:1]
    # trailing bytes after the last section are not the container's
    assert codec.unpack_sequence(data + b"\x01")[1]["total_bytes"] == len(data)


def test_pack_sequence_refusals():
    frames = _frames()
    with pytest.raises(ValueError, match="first frame"):
        codec.pack_sequence(frames[1:], 96, 64)
    with pytest.raises(ValueError, match="neither I nor P"):
        codec.pack_sequence([frames[0], ("B", frames[1][1])], 96, 64)
    with pytest.raises(ValueError, match="the sequence 96x48"):
        codec.pack_sequence(frames, 96, 48)
    with pytest.raises(ValueError, match="neither an FRC1 nor an FRQ1"):
        codec.pack_sequence([("I", b"FRC3" + bytes(60))], 96, 64)


def _edited(data: bytes, offset: int, value: bytes) -> bytes:
    return data[:offset] + value + data[offset + len(value):]


def test_unpack_sequence_refusals():
    frames = _frames()
    data = codec.pack_sequence(frames, 96, 64)
    _, h = codec.unpack_sequence(data)
    cases = [
        (_edited(data, 0, b"FRCT"), "bad magic or version"),
        (_edited(data, 4, struct.pack("<H", 2)), "bad magic or version"),
        (_edited(data, 6, struct.pack("<H", 1)), "flags are not zero"),
        (_edited(data, 20 + 8 + 2, b"\x01"), "padding byte"),                       # a frame entry's zero bytes
        (_edited(data, 20 + 8 * 2, b"B"), "neither I nor P"),
        (_edited(data, 20, b"P"), "first frame"),
        (data[:-8], "runs past the end"),                                           # the last section cut short
        (data[:20 + 8 * 3], "frame table runs past the end"),
        (data[:12], "truncated header"),
        (_edited(data, 12, struct.pack("<I", 48)), "the sequence 96x48"),           # the streams are 96x64
        (_edited(data, 20 + 8 + 4, struct.pack("<I", h["length"][1] - 4)), "FRQ1: truncated"),  # its own parser
    ]
    k = next(k for k in range(4) if h["length"][k] % 8)
    cases.append((_edited(data, h["offset"][k] + h["length"][k], b"\x01"), "padding byte"))
    for bad, why in cases:
        with pytest.raises(ValueError, match=why):
            codec.unpack_sequence(bad)
    # a frame stream of another frame size, well-formed in itself
    other = codec.pack_sequence([("I", SQ.case_stream("128x64_none"))], 128, 64)
    with pytest.raises(ValueError, match="the sequence 96x64"):
        codec.unpack_sequence(_edited(other, 8, struct.pack("<II", 96, 64)))
