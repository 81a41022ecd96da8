"""frac_decode_frc1: FRC1 streams unpacked, validated and decoded on the device, at any integer scale.

Bar: every comparison is against the oracle decoding codec.unpack_stream's records (every coordinate
and size multiplied by the scale); plane, iteration count and rms are identical.  The decode is
fixed-point given identical records, so no tolerance applies.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import fractencode_amd as F
from fractencode_amd import codec
from frc1_synth import oracle_decode_stream as _want, set_bits as _set_bits
from golden_util import plane

pytestmark = pytest.mark.gpu


def _search(p, n, T=4, cls=False, dsize=None, bits=((5, 7),)):
    """GPU search of plane p → (records, [device-packed stream per bits pair])."""
    H, W = p.shape
    dsize = dsize or 2 * n
    doms = F.create_uniform_grid(W, H, dsize, dsize // 2)
    rngs = F.create_uniform_grid(W, H, n, n)
    with F.Engine(0, T, cls) as e:
        e.set_frame(p)
        e.set_domains(F.preclassify(p, doms) if cls else doms)
        out, _ = e.search(F.preclassify(p, rngs) if cls else rngs)
        streams = [e.pack_frc1(*b) for b in bits] if dsize == 2 * n else []
    return out, streams


@functools.lru_cache(maxsize=None)
def _crop64_stream():
    return _search(plane("crop64"), 8)[1][0]


LENNA_BITS = ((5, 7), (7, 11), (9, 16))


@functools.lru_cache(maxsize=None)
def _lenna_streams(T):
    return _search(plane("lenna_y"), 8, T=T, bits=LENNA_BITS if T == 4 else ((5, 7),))[1]


def _same(got, want):
    assert (got[1], got[2]) == (want[1], want[2])
    np.testing.assert_array_equal(got[0], want[0])


def test_unaligned_record_width(oracle):
    # case 1: 64², 49 domains → 6 + 2 + 5 + 7 = 20-bit records
    s = _crop64_stream()
    assert F.frc1_info(s)["record_bits"] == 20
    with F.Engine(0, 4) as e:
        for m in (-1, 0, 1, 3):
            _same(e.decode_frc1(s, max_iter=m), _want(oracle, s, max_iter=m))


@pytest.mark.parametrize("T,k,bits", [(4, 0, 26), (4, 1, 32), (4, 2, 39), (8, 0, 27)])
def test_wider_records(oracle, T, k, bits):
    # case 2: 512², 3969 domains → 12 index bits; 39-bit records straddle three words
    s = _lenna_streams(T)[k]
    assert F.frc1_info(s)["record_bits"] == bits
    with F.Engine(0, T) as e:
        _same(e.decode_frc1(s), _want(oracle, s))


@pytest.mark.parametrize("scale", [2, 3])
def test_scale(oracle, scale):
    # case 3: the 64² stream decoded at 128² and 192²
    s = _crop64_stream()
    with F.Engine(0, 4) as e:
        for m in (-1, 2):
            got = e.decode_frc1(s, scale=scale, max_iter=m)
            assert got[0].shape == (64 * scale, 64 * scale)
            _same(got, _want(oracle, s, scale, max_iter=m))


@pytest.mark.parametrize("scale", [1, 2])
def test_domainless_records(oracle, scale):
    # case 4: the classifier leaves 5 of this frame's 16 ranges without a domain (tests/test_gpu_stream.py);
    # their pixels keep the initial plane's values
    p = np.random.default_rng(0).integers(0, 256, (32, 32), dtype=np.uint8)
    s = _search(p, 8, cls=True)[1][0]
    rec, h = codec.unpack_stream(s)
    assert 0 < int((rec["sw"] == 0).sum()) < len(rec)
    init = np.random.default_rng(1).integers(1, 256, (32 * scale, 32 * scale), dtype=np.uint8)
    with F.Engine(0, 4) as e:
        _same(e.decode_frc1(s, scale=scale, initial=init), _want(oracle, s, scale, initial=init))


@pytest.mark.parametrize("scale", [1, 2])
def test_margins(oracle, scale):
    # case 5: 70×52 is no multiple of the range size: the right and bottom margins are never written
    p = np.random.default_rng(7).integers(0, 256, (52, 70), dtype=np.uint8)
    out, _ = _search(p, 8, bits=())
    s = codec.pack_stream(out, 70, 52, 8)
    init = np.random.default_rng(8).integers(1, 256, (52 * scale, 70 * scale), dtype=np.uint8)
    with F.Engine(0, 4) as e:
        _same(e.decode_frc1(s, scale=scale, initial=init), _want(oracle, s, scale, initial=init))
        _same(e.decode_frc1(s, scale=scale), _want(oracle, s, scale))


def test_ratio_other_than_two(oracle):
    # case 6: 16×16 domains onto 4×4 ranges (the CLI default)
    out, _ = _search(plane("crop64"), 4, dsize=16)
    s = codec.pack_stream(out, 64, 64, 4, domain_size=16)
    with F.Engine(0, 4) as e:
        _same(e.decode_frc1(s), _want(oracle, s))
        _same(e.decode_frc1(s, scale=2, max_iter=3), _want(oracle, s, 2, max_iter=3))


def test_degenerate_quantizer_field(oracle):
    # case 7: a constant frame: every contrast equal and every brightness equal, so the header stores
    # min == max and every record dequantizes to exactly that value
    p = np.full((32, 32), 77, dtype=np.uint8)
    s = _search(p, 8)[1][0]
    h = F.frc1_info(s)
    assert h["contrast_min"] == h["contrast_max"] and h["brightness_min"] == h["brightness_max"]
    with F.Engine(0, 4) as e:
        _same(e.decode_frc1(s), _want(oracle, s))


def test_rejections_leave_the_context_usable(oracle):
    s = _crop64_stream()
    h = F.frc1_info(s)
    want = _want(oracle, s)
    # record 37's index field overwritten by n_domains + 1 (the error unpack_stream raises)
    bad = _set_bits(s, 37 * h["record_bits"], h["index_bits"], h["n_domains"] + 1)
    with pytest.raises(ValueError):
        codec.unpack_stream(bad)
    with F.Engine(0, 4) as e:
        with pytest.raises(F.FracError, match="domain index out of range"):
            e.decode_frc1(bad)
        _same(e.decode_frc1(s), want)
        # a plane one byte short of the output
        buf = np.frombuffer(s, dtype=np.uint8)
        out = np.zeros((64, 64), np.uint8)
        it, rms = C.c_int(), C.c_double()
        rc = F.lib().frac_decode_frc1(e._ctx, buf.ctypes.data, len(buf), 1, -1, 1e-5, out.ctypes.data, out.size - 1,
                                      C.byref(it), C.byref(rms))
        assert rc == -1  # FRAC_E_INVALID
        with pytest.raises(F.FracError):
            e._check(rc)
        assert not out.any()
        _same(e.decode_frc1(s), want)
        for scale in (0, 17):
            with pytest.raises(F.FracError):
                e.decode_frc1(s, scale=scale)
            _same(e.decode_frc1(s), want)
        # a header the host check refuses never reaches the device either
        with pytest.raises(F.FracError):
            e.decode_frc1(s[:-1])
        _same(e.decode_frc1(s), want)


def test_equals_the_item_decoder_at_512():
    s = _lenna_streams(4)[0]
    with F.Engine(0, 4) as e:
        got = e.decode_frc1(s)
        ref = e.decode(codec.unpack_stream(s)[0], 512, 512)
    _same(got, ref)
    # and the stepwise item decoder fed by the device-side expansion of the same stream
    with F.Engine(0, 4, flags=F.FLAG_DECODE_STEPWISE) as e:
        _same(e.decode_frc1(s, max_iter=4), F.Engine(0, 4).decode_frc1(s, max_iter=4))


def test_decode_stream_convenience():
    s = _crop64_stream()
    with F.Engine(0, 4) as e:
        want = e.decode_frc1(s, scale=2, max_iter=5)
    _same(F.decode_stream(s, scale=2, max_iter=5), want)
