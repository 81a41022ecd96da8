"""Inter-coded frames decoded on the device (frac_decode_inter / frac_decode_inter_device): a stream applied once
to a reference plane.

The checker is inter_ref (the oracle's decoder on a stacked plane, pinned on the CPU by test_inter_ref.py), never
the library's own decoders; every comparison is byte for byte, through the host and the device variant, with
seeded random reference planes.  What the groups reach:

  inter_frc1   R = 128 > tile, R = 1 and 3 (ranges ending inside a lane's dword), W no multiple of 4 (rows end
               inside a dword: byte stores), H < 16, W > 64 and no multiple of 64, T = 8
  inter_frq1   leaves of 2..48 scaled pixels, two leaves inside one dword, boundaries off dword alignment
  inter_apply  ratios 4/3, 1, 2.5 and 4, margins, domain-less records inside a tile, no domain at all, no record
               at all, the stepwise flag
  the planes   ref pitch ≠ plane pitch, odd pitches, a base off dword alignment, pitch == W with W % 4 ≠ 0; the
               bytes between the rows of a strided destination and after its last row keep their sentinel
"""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

import fractencode_amd as F
import frc1_synth as S1
import frq1_synth as SQ
import inter_ref as R
import quadtree_frames as Q
from fractencode_amd import codec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _engine(flags=0):
    return F.Engine(0, 8, flags=flags)


_fast = functools.lru_cache(maxsize=None)(S1.fast_stream)
_other = functools.lru_cache(maxsize=None)(S1.other_stream)
_quad = functools.lru_cache(maxsize=None)(SQ.case_stream)
_REF = {}


def _want(oracle, key, stream, scale, seed=11):
    """(reference plane, the stream applied to it once) by inter_ref, computed once per case."""
    k = (key, scale, seed)
    if k not in _REF:
        _, W, H, _ = R.stream_records(stream, scale)
        ref = R.random_plane(W, H, seed)
        want = R.apply_stream(oracle, stream, ref, scale)
        ref.setflags(write=False)
        want.setflags(write=False)
        _REF[k] = (ref, want)
    return _REF[k]


def _check(oracle, e, key, stream, scale):
    ref, want = _want(oracle, key, stream, scale)
    np.testing.assert_array_equal(e.decode_inter(stream, ref, scale), want)
    d_ref = torch.from_numpy(ref.copy()).to(DEV)
    got = e.decode_inter(stream, d_ref, scale)
    assert got.is_cuda and got.data_ptr() != d_ref.data_ptr()
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    np.testing.assert_array_equal(d_ref.cpu().numpy(), ref)  # the reference is read, not written
    return ref, want


def _is_fast(stream):
    rec, W, H, g = R.stream_records(stream)
    return len(rec) > 0 and W % g == 0 and H % g == 0 and bool((rec["sw"] == 2 * rec["w"]).all())


# --- FRC1 -------------------------------------------------------------------------------------------------

FRC1_FAST = [pytest.param(k, s, id=f"fast{k}-x{s}") for k in (0, 1, 2, 3, 4, 6) for s in S1.FAST_STREAMS[k][7][:2]]
FRC1_FAST.append(pytest.param(0, 16, id="fast0-x16"))  # R = 128: a range larger than the 64×16 tile


@pytest.mark.parametrize("k,scale", FRC1_FAST)
def test_frc1_fast_geometry(oracle, k, scale):
    assert _is_fast(_fast(k))
    _check(oracle, _engine(), ("fast", k), _fast(k), scale)


@pytest.mark.parametrize("k", range(8))
def test_frc1_general_route(oracle, k):
    s = _other(k)
    assert not _is_fast(s)
    for scale in (1, 2):
        ref, want = _check(oracle, _engine(), ("other", k), s, scale)
        if k in (5, 6):  # no domain fits / no range fits: the plane is the reference
            np.testing.assert_array_equal(want, ref)
        else:
            assert (want != ref).any()
    if k == 7:  # margins keep the reference
        W, H, n = S1.OTHER_STREAMS[k][:3]
        ref, want = _want(oracle, ("other", k), s, 1)
        np.testing.assert_array_equal(want[:, W - W % n:], ref[:, W - W % n:])
        np.testing.assert_array_equal(want[H - H % n:], ref[H - H % n:])


# --- FRQ1 -------------------------------------------------------------------------------------------------

FRQ1_FAST = {"96x64", "48x32_to2", "80x48_16_8", "24x40_8", "128x64_all", "128x64_none", "256x128_carry"}


@pytest.mark.parametrize("scale", [1, 3])
@pytest.mark.parametrize("name", list(SQ.CASES))
def test_frq1(oracle, name, scale):
    s = _quad(name)
    assert _is_fast(s) == (name in FRQ1_FAST)
    _check(oracle, _engine(), ("quad", name), s, scale)


# --- the planes' layouts ------------------------------------------------------------------------------------

def _strided(rows, W, pitch, offset, fill):
    """A [rows, W] view at column `offset` of a [rows + 1, pitch] buffer filled with `fill`: (buffer, view)."""
    buf = torch.full((rows + 1, pitch), fill, dtype=torch.uint8, device=DEV)
    return buf, buf[:rows, offset:offset + W]


def _check_layout(e, stream, ref, want, rpitch, roff, ppitch, poff):
    H, W = ref.shape
    rbuf, r = _strided(H, W, rpitch, roff, 0xA5)
    r.copy_(torch.from_numpy(ref.copy()))
    pbuf, p = _strided(H, W, ppitch, poff, 0x5A)
    out = e.decode_inter(stream, r, out=p)
    assert out.data_ptr() == p.data_ptr()
    got = pbuf.cpu().numpy()
    np.testing.assert_array_equal(got[:H, poff:poff + W], want)
    mask = np.ones(got.shape, bool)
    mask[:H, poff:poff + W] = False
    assert (got[mask] == 0x5A).all(), (rpitch, roff, ppitch, poff)  # between the rows and after the last one
    back = rbuf.cpu().numpy()
    np.testing.assert_array_equal(back[:H, roff:roff + W], ref)
    mask = np.ones(back.shape, bool)
    mask[:H, roff:roff + W] = False
    assert (back[mask] == 0xA5).all()


LAYOUTS = [(128, 0, 112, 0),   # ref pitch ≠ plane pitch, both dword-aligned
           (112, 0, 128, 4),   # the plane's base off the buffer's, still dword-aligned
           (101, 0, 103, 0),   # both pitches odd: byte stores
           (128, 0, 112, 1),   # a plane base offset by 1 byte
           (128, 2, 112, 2),   # and by 2
           (105, 3, 112, 0)]   # an odd reference under a dword-aligned plane


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda v: "r%d+%d_p%d+%d" % v)
def test_device_layouts(oracle, layout):
    for key, s in ((("fast", 4), _fast(4)), (("quad", "96x64"), _quad("96x64"))):
        ref, want = _want(oracle, key, s, 1)
        assert ref.shape[1] in (100, 96)
        _check_layout(_engine(), s, ref, want, *layout)


def test_tight_rows_that_end_inside_a_dword(oracle):
    # pitch == W exactly with W % 4 != 0: rows start at every alignment and end inside a lane's dword
    quad = SQ.synth_quadtree_stream(22, 10, 60, sizes=(2,))
    assert _is_fast(quad)
    for key, s in ((("fast", 2), _fast(2)), (("fast", 3), _fast(3)), (("quad22", 0), quad)):
        ref, want = _want(oracle, key, s, 1)
        H, W = ref.shape
        assert W % 4 != 0
        _check_layout(_engine(), s, ref, want, W, 0, W, 0)
        # general route, the same planes: the fill goes row by row too
        _check_layout(_engine(F.FLAG_DECODE_STEPWISE), s, ref, want, W + 5, 1, W + 3, 2)


# --- refusals -------------------------------------------------------------------------------------------------

def _device_call(e, stream, scale, ref, rstride, plane, pstride, plane_bytes):
    buf = np.frombuffer(stream, np.uint8)
    torch.cuda.synchronize()
    rc = F.lib().frac_decode_inter_device(e._ctx, buf.ctypes.data, len(buf), scale,
                                          C.c_void_p(ref.data_ptr() if ref is not None else None), rstride,
                                          C.c_void_p(plane.data_ptr() if plane is not None else None), pstride,
                                          plane_bytes)
    e.sync()
    return rc


def _host_call(e, stream, scale, ref, plane, plane_bytes):
    buf = np.frombuffer(stream, np.uint8)
    return F.lib().frac_decode_inter(e._ctx, buf.ctypes.data, len(buf), scale,
                                     ref.ctypes.data if ref is not None else None,
                                     plane.ctypes.data if plane is not None else None, plane_bytes)


def _bad_index_streams():
    s = _fast(4)
    h = F.frc1_info(s)
    assert h["n_domains"] + 1 < 1 << h["index_bits"]
    bad1 = S1.set_bits(s, 3 * h["record_bits"], h["index_bits"], h["n_domains"] + 1)
    assert F.frc1_info(bad1) == h
    q = _quad("96x64")
    hq = F.frq1_info(q)
    assert hq["n_domains"][1] + 1 < 1 << hq["index_bits"][1]
    _, widths, bit = SQ.record_fields(q, hq, 1, 3)
    badq = SQ.set_stream_bits(q, hq["record_offset"][1], bit, widths[0], hq["n_domains"][1] + 1)
    assert F.frq1_info(badq) == hq
    return [(s, bad1, (36, 100)), (q, badq, (64, 96))]


def test_refusals_leave_the_plane_alone():
    e = _engine()
    for good, bad, (H, W) in _bad_index_streams():
        ref = R.random_plane(W, H, 5)
        d_ref = torch.from_numpy(ref).to(DEV)
        plane = torch.full((2 * H, W), 0x5A, dtype=torch.uint8, device=DEV)
        h_plane = np.full((H, W), 0x5A, np.uint8)
        full = W * (H - 1) + W
        dev = [
            (bad, 1, d_ref, W, plane, W, full, "index out of range"),
            (good, 1, d_ref, W, plane, W, full - 1, "plane_bytes"),
            (good, 1, d_ref, W, plane, W - 1, full, "stride"),
            (good, 1, d_ref, W - 1, plane, W, full, "stride"),
            (good, 0, d_ref, W, plane, W, full, "scale"),
            (good, 17, d_ref, W, plane, W, 17 * 17 * full, "scale"),
            (good, 1, None, W, plane, W, full, "NULL"),
            (good, 1, d_ref, W, None, W, full, "NULL"),
            (good, 1, plane[:H], W, plane[H - 1:], W, full, "overlap"),   # the ref's last row is the plane's first
            (good, 1, plane[1:], W, plane[:H], W, full, "overlap"),
            (good, 1, plane[:H], W, plane[:H], W, full, "overlap"),       # in place
            (good[:-1], 1, d_ref, W, plane, W, full, "truncated|ends inside"),
            (b"FRC3" + good[4:], 1, d_ref, W, plane, W, full, "neither"),
        ]
        for stream, scale, r, rs, p, ps, nbytes, why in dev:
            assert _device_call(e, stream, scale, r, rs, p, ps, nbytes) == -1, why
            assert (plane == 0x5A).all(), why
            assert re.search(why, F.last_error(e._ctx)), (why, F.last_error(e._ctx))
        # adjacent, not overlapping: the plane starts at the byte after the reference's last
        plane[:H].copy_(d_ref)
        assert _device_call(e, good, 1, plane[:H], W, plane[H:], W, full) == 0
        host = [(bad, 1, ref, h_plane, full), (good, 1, ref, h_plane, full - 1), (good, 0, ref, h_plane, full),
                (good, 17, ref, h_plane, 17 * 17 * full), (good, 1, None, h_plane, full)]
        for stream, scale, r, p, nbytes in host:
            assert _host_call(e, stream, scale, r, p, nbytes) == -1
            assert (h_plane == 0x5A).all()
        assert _host_call(e, good, 1, ref, None, full) == -1
        # the wrapper refuses a reference of the wrong shape before the call
        with pytest.raises(F.FracError, match=f"ref must be {H}x{W}"):
            e.decode_inter(good, ref[:-1])
        with pytest.raises(F.FracError, match=f"ref must be {H}x{W}"):
            e.decode_inter(good, d_ref[:, :-1])
        with pytest.raises(F.FracError, match=f"out must be {H}x{W}"):
            e.decode_inter(good, d_ref, out=plane)
        for scale in (0, 17):  # and a scale outside 1..16, for either kind of reference
            for r in (ref, d_ref):
                with pytest.raises(F.FracError, match="scale must be in 1..16"):
                    e.decode_inter(good, r, scale)
        # spans, not pixels: the left and right halves of one wide buffer interleave without sharing a byte
        wide = torch.full((H, 2 * W), 0x5A, dtype=torch.uint8, device=DEV)
        assert _device_call(e, good, 1, wide[:, :W], 2 * W, wide[:, W:], 2 * W, 2 * W * (H - 1) + W) == -1
        assert "overlap" in F.last_error(e._ctx) and (wide == 0x5A).all()


def test_index_equal_to_the_domain_count_keeps_the_reference(oracle):
    s = _fast(4)
    h = F.frc1_info(s)
    none = S1.set_bits(s, 3 * h["record_bits"], h["index_bits"], h["n_domains"])
    ref, want = _check(oracle, _engine(), ("fast4-none3",), none, 1)
    np.testing.assert_array_equal(want[0:4, 12:16], ref[0:4, 12:16])  # record 3's range
    assert not _is_fast(none)


# --- state ---------------------------------------------------------------------------------------------------

def test_decode_inter_is_a_reader(oracle):
    case = Q.BY_NAME["m98x74_16_4"]
    frame = case.planes()[0]
    doms, rngs = F.create_uniform_grid(case.W, case.H, 16, 8), F.create_uniform_grid(case.W, case.H, 8, 8)
    s = _quad("96x64")
    ref, want = _want(oracle, ("quad", "96x64"), s, 1)
    with F.Engine(0, 4) as e:
        np.testing.assert_array_equal(e.decode_inter(s, ref), want)  # no frame needs to be set
        e.set_frame(frame)
        e.set_domains(doms)
        items, _ = e.search(rngs)
        np.testing.assert_array_equal(e.decode_inter(s, ref), want)
        e.decode_inter(s, torch.from_numpy(ref.copy()).to(DEV))
        again, _ = e.fetch()
        assert again.tobytes() == items.tobytes()
        e.quadtree_rate(16, 4)
        before = e.rate_sizes([0.0, 5.0, 50.0])
        np.testing.assert_array_equal(e.decode_inter(_fast(4), _want(oracle, ("fast", 4), _fast(4), 1)[0]),
                                      _want(oracle, ("fast", 4), _fast(4), 1)[1])
        for a, b in zip(before, e.rate_sizes([0.0, 5.0, 50.0])):
            np.testing.assert_array_equal(a, b)


def test_stepwise_flag_gives_the_same_bytes(oracle):
    for key, s, scale in ((("fast", 4), _fast(4), 3), (("quad", "48x32_to2"), _quad("48x32_to2"), 3)):
        assert _is_fast(s)
        _check(oracle, _engine(F.FLAG_DECODE_STEPWISE), key, s, scale)


def test_decode_inter_stream(oracle):
    s = _quad("96x64")
    ref, want = _want(oracle, ("quad", "96x64"), s, 1)
    np.testing.assert_array_equal(F.decode_inter_stream(s, ref), want)
    rec, _ = codec.unpack_quadtree_stream(s)
    assert len(rec) and (want != ref).any()
