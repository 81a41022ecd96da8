"""FRC1 decode and pack, and the item decoder, at small odd geometries.

Records are made on the host (frc1_synth: random items through codec.pack_stream) or by a search of a
small random plane; the checker is the oracle decoding codec.unpack_stream's records, scaled.  Every
comparison is exact: bytes, planes, iteration count and rms.  What each group reaches that the larger
fixtures (word-aligned bodies, square frames, R ∈ {8, 16, 24}) never did:

  frc1dec_records   the last record's window over a partial tail word; all 32 bit offsets; 63- and 64-bit
                    records (the third-dword merge, the record_bits == 64 mask)
  frac_decode_frc1  the tail memset / copy of a body that is no whole number of dwords; a stream without
                    ranges; a stream without domains; the 65535 bound
  frc1dec_step      R = 1, 2, 3, 6, 12, 15 and 128: the range switch inside a lane's dword, tiles of exactly
                    1024 records, a range larger than the tile; widths that are no multiple of 4 or 64;
                    rcols ≠ rrows; T = 8 with a scale
  decode_fused_loop convergence below, at and above the 8-step chunk, and the 300-step run
  frc1dec_expand    domain sides that are not twice the range side, domain-less records, margins
  decode_fused / decode_apply   non-power-of-two range sides (the `%` path), size ratios 1 (the sampler's
                    edge clamp), 1.5, 2.5, 3 and 4, off-lattice domains on non-square planes, mixed sizes
  frc1_minmax / frc1_records / frc1_words   n ∈ {2, 3, 4, 16}, non-square frames, margins, domain counts
                    1, 2^k − 1 and 2^k, 2- and 16-bit fields, the tail clamp, a second frame

The device dequantizer (frc1_value) is checked only through the decoded pixels: a 1-ulp slip in a
contrast or brightness would rarely move a pixel, so these tests do not pin it to the last bit.
"""
import functools

import numpy as np
import pytest

import fractencode_amd as F
from fractencode_amd import codec
from frc1_synth import (FAST_STREAMS, OTHER_STREAMS, fast_stream, oracle_decode_stream, other_stream, set_bits,
                        synth_items, synth_mixed_items, synth_stream)
from golden_util import oracle_records

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _engine(T, flags=0):
    """One context per (transforms, flags) for the whole module: its buffers are reused across streams of
    different sizes, as a long-lived decoder's are."""
    return F.Engine(0, T, flags=flags)


_fast = functools.lru_cache(maxsize=None)(fast_stream)
_other = functools.lru_cache(maxsize=None)(other_stream)


def _initial(shape, seed=9):
    return np.random.default_rng(seed).integers(1, 256, shape, dtype=np.uint8)


def _same(got, want):
    assert (got[1], got[2]) == (want[1], want[2])
    np.testing.assert_array_equal(got[0], want[0])


def _check_stream(oracle, e, s, scale, max_iters=(-1, 5)):
    """decode_frc1 against the oracle: with and without an initial plane, unbounded and bounded."""
    h = codec.read_header(s)
    init = _initial((scale * h["height"], scale * h["width"]))
    for initial in (None, init):
        for m in max_iters:
            _same(e.decode_frc1(s, scale=scale, max_iter=m, initial=initial),
                  oracle_decode_stream(oracle, s, scale, m, initial))


# --- stream decoder: the fast path --------------------------------------------------------------

FAST_CASES = [pytest.param(k, scale, id=f"{c[0]}x{c[1]}-n{c[2]}-{c[6]}bit-x{scale}")
              for k, c in enumerate(FAST_STREAMS) for scale in c[7]]


@pytest.mark.parametrize("k,scale", FAST_CASES)
def test_fast_path_geometries(oracle, k, scale):
    W, H, n, T, cb, bb, record_bits, _ = FAST_STREAMS[k]
    s = _fast(k)
    h = F.frc1_info(s)
    # what sends a stream down frc1dec_step: the grid tiles the frame, domain = 2n, no domain-less record
    assert W % n == 0 and H % n == 0 and h["domain_size"] == 2 * n
    assert (codec.unpack_stream(s)[0]["sw"] == 2 * n).all()
    assert h["record_bits"] == record_bits and h["body_bytes"] == (h["n_ranges"] * record_bits + 7) // 8
    _check_stream(oracle, _engine(T), s, scale)


def test_fast_path_stream_shapes():
    # the properties the cases above are chosen for
    h = F.frc1_info(_fast(0))
    assert (h["n_ranges"], h["n_domains"], h["n_ranges"] * h["record_bits"]) == (15, 8, 270)
    assert h["body_bytes"] == 34  # 8 whole dwords + 2 bytes, the last of them 6 bits
    h = F.frc1_info(_fast(7))
    assert (h["n_domains"], h["index_bits"], h["n_ranges"]) == (4096, 13, 4225)
    assert {(i * 63) % 32 for i in range(h["n_ranges"])} == set(range(32))
    for k in range(len(FAST_STREAMS) - 1):
        h = F.frc1_info(_fast(k))
        bits = h["n_ranges"] * h["record_bits"]
        assert bits % 32 and (bits % 8 or k == 6)  # 208×48: 195 whole bytes, no whole dword


def test_tail_record_is_decoded(oracle):
    # the last record of the 270-bit body lies in the partial tail word: its transform and brightness code
    # rewritten must change the decoded range, on the oracle and on the device alike
    s = _fast(0)
    h = F.frc1_info(s)
    last = h["n_ranges"] - 1
    widths = [h["index_bits"], 2, h["contrast_bits"], h["brightness_bits"]]
    _, t, _, qb = (int(f[last]) for f in codec._unpack_bits(s[codec.HEADER.size:], h["n_ranges"], widths))
    bit = last * h["record_bits"]
    assert bit + h["record_bits"] > 32 * (h["body_bytes"] // 4)  # it reaches into the tail word
    edited = set_bits(s, bit + widths[0], 2, t ^ 1)
    edited = set_bits(edited, bit + widths[0] + 2 + widths[2], widths[3], qb ^ 0x40)
    rec = codec.unpack_stream(s)[0][last]
    box = np.s_[int(rec["y"]):int(rec["y"] + rec["h"]), int(rec["x"]):int(rec["x"] + rec["w"])]
    e = _engine(4)
    for m in (-1, 5):
        a, b = oracle_decode_stream(oracle, s, max_iter=m), oracle_decode_stream(oracle, edited, max_iter=m)
        assert (a[0][box] != b[0][box]).any()
        _same(e.decode_frc1(edited, max_iter=m), b)
        _same(e.decode_frc1(s, max_iter=m), a)


# --- convergence in the 8-step chunked loop -----------------------------------------------------

# (W, H, n, cmax, seed) → the oracle's iteration count at scale 1 and at scale 3.  Step i of the loop is
# the (i + 1)-th; the host looks at the flag after steps 7, 15, …: counts of 5-7 stop inside the first chunk
# with steps enqueued behind them, 8 and 9 just after the first look, 10-12 further on, 300 never.
CONVERGENCE = [
    ((13, 9, 1, 0.6, 1), (6, 7)),
    ((13, 9, 1, 0.8, 5), (8, 300)),
    ((13, 9, 1, 0.95, 1), (8, 12)),
    ((70, 6, 2, 0.6, 2), (6, 9)),
    ((70, 6, 2, 0.8, 3), (300, 11)),
    ((70, 6, 2, 0.95, 5), (8, 12)),
    ((66, 27, 3, 0.6, 1), (7, 10)),
    ((66, 27, 3, 0.8, 3), (10, 300)),
    ((66, 27, 3, 0.95, 5), (9, 12)),
]


@functools.lru_cache(maxsize=None)
def _contractive(W, H, n, cmax, seed):
    return synth_stream(W, H, n, 2 * n, 8, seed, cmax=cmax, brightness=(0.0, 200.0))


@pytest.mark.parametrize("case,counts", CONVERGENCE, ids=[f"{c[0]}x{c[1]}-c{c[3]}" for c, _ in CONVERGENCE])
def test_convergence_counts(oracle, case, counts):
    s = _contractive(*case)
    for scale, count in zip((1, 3), counts):
        want = oracle_decode_stream(oracle, s, scale)
        assert want[1] == count  # the property the case is kept for
        assert (want[2] < 1e-5) == (count < 300)
        _same(_engine(8).decode_frc1(s, scale=scale), want)
        init = _initial(want[0].shape)
        _same(_engine(8).decode_frc1(s, scale=scale, initial=init), oracle_decode_stream(oracle, s, scale, initial=init))


def test_convergence_counts_cover_the_chunk_boundary():
    counts = {c for _, pair in CONVERGENCE for c in pair}
    assert any(c < 8 for c in counts) and counts & {8, 9} and any(9 < c < 300 for c in counts) and 300 in counts


def test_convergence_stepwise(oracle):
    # the same streams through frc1dec_expand and the step-by-step item decoder
    e = _engine(8, F.FLAG_DECODE_STEPWISE)
    for case, counts in (CONVERGENCE[1], CONVERGENCE[6]):
        for scale, count in zip((1, 3), counts):
            want = oracle_decode_stream(oracle, _contractive(*case), scale)
            assert want[1] == count
            _same(e.decode_frc1(_contractive(*case), scale=scale), want)


# --- stream decoder: every other stream ---------------------------------------------------------

OTHER_CASES = [pytest.param(k, scale, id=f"{c[0]}x{c[1]}-n{c[2]}-d{c[3]}-x{scale}")
               for k, c in enumerate(OTHER_STREAMS[:-1]) for scale in (1, 2)]


@pytest.mark.parametrize("k,scale", OTHER_CASES)
def test_other_stream_geometries(oracle, k, scale):
    W, H, n, d, every = OTHER_STREAMS[k]
    s = _other(k)
    rec, h = codec.unpack_stream(s)
    empty = int((rec["sw"] == 0).sum())
    if every:
        # a 64×16 output tile of the scale-1 frame covers ranges of both kinds
        assert 0 < empty < len(rec)
        tile = rec[(rec["x"] < 64) & (rec["y"] < 16)]
        assert 0 < int((tile["sw"] == 0).sum()) < len(tile)
    elif h["n_domains"] == 0:
        assert empty == len(rec) and h["index_bits"] == 1
    else:
        assert empty == 0
    _check_stream(oracle, _engine(8), s, scale)
    _check_stream(oracle, _engine(8, F.FLAG_DECODE_STEPWISE), s, scale, max_iters=(5,))


def test_stream_without_ranges_returns_the_initial_plane(oracle):
    s = _other(6)
    assert len(s) == codec.HEADER.size and F.frc1_info(s)["n_ranges"] == 0
    init = _initial((14, 10))
    got = _engine(8).decode_frc1(s, scale=2, initial=init)
    _same(got, oracle_decode_stream(oracle, s, 2, initial=init))
    np.testing.assert_array_equal(got[0], init)


def test_scale_bound(oracle):
    # 4096×8: refused at scale 16 (65536 columns), accepted at 15 (one 61440×120 plane)
    s = _other(len(OTHER_STREAMS) - 1)
    h = F.frc1_info(s)
    assert (h["n_ranges"], h["n_domains"], h["body_bytes"]) == (512, 0, 1024)
    e = _engine(8)
    with pytest.raises(F.FracError, match="at most 65535"):
        e.decode_frc1(s, scale=16)
    init = _initial((15 * 8, 15 * 4096))
    _same(e.decode_frc1(s, scale=15, initial=init), oracle_decode_stream(oracle, s, 15, initial=init))
    _same(e.decode_frc1(_fast(0)), oracle_decode_stream(oracle, _fast(0)))


# --- device packer ------------------------------------------------------------------------------

def _plane(W, H, seed, patch=False):
    """Uniform noise; `patch`: a ramp with one 12×12 block of noise, so that few categories have a domain."""
    rng = np.random.default_rng(seed)
    if not patch:
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    p = ((2 * x + 3 * y) % 256).astype(np.uint8)
    p[10:22, 30:42] = rng.integers(0, 256, (12, 12), dtype=np.uint8)
    return p


def _load(e, p, n, cls, dsize=None, dstride=None):
    H, W = p.shape
    doms = F.create_uniform_grid(W, H, dsize or 2 * n, dstride or n)
    rngs = F.create_uniform_grid(W, H, n, n)
    e.set_frame(p)
    e.set_domains(F.preclassify(p, doms) if cls else doms)
    return e.search(F.preclassify(p, rngs) if cls else rngs)


# (W, H, n, T, classifier, contrast bits, brightness bits, plane seed); the classifier cases' seeds are
# those whose frame leaves some, not all, ranges without a domain (3 of 48 and 1 of 225)
PACK_CASES = [
    (24, 40, 8, 4, False, 5, 7, 11),    # 8 = 2^3 domains; 270 bits: the tail clamp
    (64, 16, 8, 4, False, 5, 7, 12),    # 7 = 2^3 − 1 domains
    (16, 16, 8, 4, False, 5, 7, 13),    # one domain, four ranges
    (70, 52, 8, 8, True, 5, 7, 5),      # margins; ranges without a domain of their category
    (70, 6, 2, 8, False, 2, 16, 15),
    (66, 27, 3, 4, False, 6, 9, 16),
    (100, 36, 4, 8, True, 16, 2, 18),   # the ramp-and-patch plane
    (208, 48, 16, 4, False, 9, 16, 18),
]


@pytest.mark.parametrize("W,H,n,T,cls,cb,bb,seed", PACK_CASES, ids=[f"{c[0]}x{c[1]}-n{c[2]}" for c in PACK_CASES])
def test_device_packer_geometries(oracle, W, H, n, T, cls, cb, bb, seed):
    p = _plane(W, H, seed, patch=(W, H) == (100, 36))
    with F.Engine(0, T, cls) as e:
        out, st = _load(e, p, n, cls)
        dev = e.pack_frc1(cb, bb)
        if cls:
            assert 0 < st["empty_ranges"] < len(out)
        else:
            assert st["empty_ranges"] == 0
        assert dev == codec.pack_stream(out, W, H, n, transforms=T, use_classifier=cls, contrast_bits=cb,
                                        brightness_bits=bb)
        info, h = F.frc1_info(dev), codec.read_header(dev)
        assert {k: h[k] for k in h if k not in ("magic", "version")} == \
               {k: info[k] for k in info if k not in ("record_bits", "body_bytes")}
        assert info["body_bytes"] == len(dev) - codec.HEADER.size
        init = _initial((H, W))
        for m in (-1, 5):
            _same(e.decode_frc1(dev, max_iter=m, initial=init), oracle_decode_stream(oracle, dev, 1, m, init))


def test_device_packer_domain_counts():
    for k, nd in ((0, 8), (1, 7), (2, 1)):
        W, H, n = PACK_CASES[k][:3]
        assert len(F.create_uniform_grid(W, H, 2 * n, n)) == nd


def test_device_packer_second_frame():
    # the min / max cells are initialised per call: a second frame's stream is a fresh context's
    a, b = _plane(24, 40, 21), (_plane(24, 40, 22) // 4 + 90).astype(np.uint8)  # b: a narrower value range
    with F.Engine(0, 4) as e:
        _load(e, a, 8, False)
        first = e.pack_frc1()
        e.set_frame(b)
        e.run()
        second = e.pack_frc1()
        assert e.pack_frc1() == second
    with F.Engine(0, 4) as e:
        _load(e, b, 8, False)
        fresh = e.pack_frc1()
    assert second == fresh != first
    ha, hb = codec.read_header(first), codec.read_header(fresh)
    assert (ha["brightness_min"], ha["brightness_max"]) != (hb["brightness_min"], hb["brightness_max"])


def test_device_packer_refusals_leave_the_context_usable():
    p = _plane(64, 64, 23)
    with F.Engine(0, 4) as e:
        out, _ = _load(e, p, 8, False)
        want = codec.pack_stream(out, 64, 64, 8)
        for cb, bb in ((1, 7), (17, 7), (5, 1), (5, 17)):
            with pytest.raises(F.FracError, match=r"bits must be in \[2, 16\]"):
                e.pack_frc1(cb, bb)
            assert e.pack_frc1() == want
        # rectangular ranges (the cut domain grid of tests/test_gpu_parity.py)
        e.set_domains(F.create_uniform_grid(64, 56, (16, 8), (8, 4)))
        e.search(F.create_uniform_grid(64, 64, (8, 4), (8, 4)))
        with pytest.raises(F.FracError, match="square items only"):
            e.pack_frc1()
        # domains of side 2n at stride n / 2
        _load(e, p, 8, False, dsize=16, dstride=4)
        with pytest.raises(F.FracError, match="not the domain lattice"):
            e.pack_frc1()
        # a source plane of another size than the target's
        e.set_planes(p, p[:32, :32])
        e.set_domains(F.create_uniform_grid(64, 64, 16, 8))
        e.search(F.create_uniform_grid(32, 32, 8, 8))
        with pytest.raises(F.FracError, match="one size"):
            e.pack_frc1()
        _load(e, p, 8, False)
        assert e.pack_frc1() == want


# --- item decoder -------------------------------------------------------------------------------

# (W, H, n, d): off-lattice domains, T = 8
ITEM_CASES = [
    (72, 40, 8, 8),    # ratio 1: the sampler's edge clamp
    (72, 40, 8, 12),   # ratio 1.5
    (70, 50, 4, 10),   # ratio 2.5; margins: the unfused path
    (66, 27, 3, 9),    # ratio 3, n no power of two
    (65, 35, 5, 20),   # ratio 4, n no power of two
    (78, 42, 6, 12),   # ratio 2, n no power of two
    (67, 45, 2, 4),    # margins
    (67, 45, 1, 2),    # margins, 1×1 ranges
]


@pytest.mark.parametrize("flags", [0, F.FLAG_DECODE_STEPWISE], ids=["default", "stepwise"])
@pytest.mark.parametrize("W,H,n,d", ITEM_CASES, ids=[f"{c[0]}x{c[1]}-n{c[2]}-d{c[3]}" for c in ITEM_CASES])
def test_item_decoder_geometries(oracle, W, H, n, d, flags):
    init = _initial((H, W))
    e = _engine(8, flags)
    for k, (m, cmax, brightness) in enumerate(((-1, 0.6, (0.0, 200.0)), (5, 1.1, (-40.0, 290.0)))):
        items = synth_items(W, H, n, d, 8, 300 + k, lattice=False, cmax=cmax, brightness=brightness)
        assert len(items) == (W // n) * (H // n) and (items["sw"] == d).all()
        want = oracle.decode(oracle_records(items), n, W, H, max_iter=m, initial=init)
        _same(e.decode(items, W, H, max_iter=m, initial=init), want)
        # the margin is never written
        np.testing.assert_array_equal(want[0][:, W // n * n:], init[:, W // n * n:])
        np.testing.assert_array_equal(want[0][H // n * n:], init[H // n * n:])


def test_item_decoder_off_lattice_and_clamped():
    # what the cases above rely on: origins off the (d, d / 2) lattice, and at ratio 1 a source column d − 1
    items = synth_items(72, 40, 8, 12, 8, 300, lattice=False)
    assert (items["dx"] % 6 != 0).any() and (items["dy"] % 6 != 0).any()
    assert (7 * 8) // 8 == 8 - 1  # Frac::copy's sx at the last column of a ratio-1 item: the clamped one


@pytest.mark.parametrize("flags", [0, F.FLAG_DECODE_STEPWISE], ids=["default", "stepwise"])
def test_item_decoder_mixed_sizes(oracle, flags):
    items, sizes = synth_mixed_items(96, 64, 31)
    assert {16, 8, 4} == set(sizes.tolist()) and int((sizes.astype(np.int64) ** 2).sum()) == 96 * 64
    init = _initial((64, 96))
    e = _engine(8, flags)
    for m in (-1, 5):
        _same(e.decode(items, 96, 64, max_iter=m, initial=init),
              oracle.decode_sized(oracle_records(items), sizes, 96, 64, max_iter=m, initial=init))
