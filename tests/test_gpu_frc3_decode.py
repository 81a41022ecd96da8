"""FRC3 colour containers decoded to RGB on the device (frac_decode_frc3 / frac_decode_frc3_device): for every
case the pixels equal the host restatement of yuv2rgb (tests/yuv2rgb_ref.py) applied to the three single-plane
decodes (Engine.decode_frc1 / decode_frq1, whose own tests pin them to the oracle), and the iteration counts
and rms values are the single-plane calls'.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import fractencode_amd as F
import yuv2rgb_ref as R
from fractencode_amd import codec
from frc1_synth import set_bits, synth_stream
from frq1_synth import synth_quadtree_stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    with F.Engine(0) as e:
        yield e


def chroma(W, H):
    return W // 2, H // 2


def frc1_planes(W, H, n, seed, T=4, **kw):
    cw, ch = chroma(W, H)
    return [synth_stream(W, H, n, 2 * n, T, seed, **kw), synth_stream(cw, ch, n, 2 * n, T, seed + 1, **kw),
            synth_stream(cw, ch, n, 2 * n, T, seed + 2, **kw)]


def frq1_planes(W, H, sizes, seed, T=4):
    cw, ch = chroma(W, H)
    return [synth_quadtree_stream(W, H, seed, sizes, T=T), synth_quadtree_stream(cw, ch, seed + 1, sizes, T=T),
            synth_quadtree_stream(cw, ch, seed + 2, sizes, T=T)]


def decode_plane(e, s, scale, **kw):
    return e.decode_frq1(s, scale, **kw) if s[:4] == b"FRQ1" else e.decode_frc1(s, scale, **kw)


def expected(e, planes, scale=1, **kw):
    """(rgb, iterations, rms) from the three single-plane decodes and the host conversion."""
    dec = [decode_plane(e, s, scale, **kw) for s in planes]
    return R.yuv2rgb_ref(dec[0][0], dec[1][0], dec[2][0]), [d[1] for d in dec], [d[2] for d in dec]


def check(e, planes, W, H, scale=1, ref=None, **kw):
    s = F.pack_frc3(planes, W, H)
    want = expected(ref or e, planes, scale, **kw)
    rgb, it, rms = e.decode_frc3(s, scale, **kw)
    assert rgb.shape == (scale * H, scale * W, 3)
    assert it == want[1] and rms == want[2]
    np.testing.assert_array_equal(rgb, want[0])
    return rgb


@pytest.mark.parametrize("n", [8, 4])
def test_32x32(eng, n):
    # n = 8: the 16×16 chroma planes hold one domain
    check(eng, frc1_planes(32, 32, n, 500 + n), 32, 32)


@pytest.mark.parametrize("scale", [1, 2, 3])
def test_odd_frame_at_scales(eng, scale):
    # 37×27, chroma 18×13: at scale 3 a 111-wide frame over 54-wide chroma, 81 rows over 39: the clamp is live
    rgb = check(eng, frc1_planes(37, 27, 4, 510), 37, 27, scale)
    if scale == 3:
        assert rgb.shape == (81, 111, 3) and 2 * 54 < 111 and 2 * 39 < 81


def test_quadtree_planes(eng):
    check(eng, frq1_planes(96, 64, (16, 8, 4), 520), 96, 64)
    check(eng, frq1_planes(96, 64, (16, 8, 4), 520), 96, 64, 2)


def test_mixed_kinds(eng):
    a, b = frc1_planes(96, 64, 8, 530), frq1_planes(96, 64, (16, 8, 4), 533)
    check(eng, [a[0], b[1], a[2]], 96, 64)
    check(eng, [b[0], a[1], b[2]], 96, 64, 2)


def test_chroma_without_ranges_stays_zero(eng):
    # 12×12: the 6×6 chroma planes are smaller than an 8×8 range, their streams are headers only; the planes
    # stay zero, which converts as u = v = 0
    planes = [synth_stream(12, 12, 4, 8, 4, 540), synth_stream(6, 6, 8, 16, 4, 541), synth_stream(6, 6, 8, 16, 4, 542)]
    assert F.frc1_info(planes[1])["n_ranges"] == 0
    rgb = check(eng, planes, 12, 12)
    y = eng.decode_frc1(planes[0])[0]
    np.testing.assert_array_equal(rgb, R.yuv2rgb_ref(y, np.zeros((6, 6), np.uint8), np.zeros((6, 6), np.uint8)))
    check(eng, planes, 12, 12, 3)


@pytest.mark.parametrize("max_iter", [0, 5, -1])
def test_max_iter(eng, max_iter):
    check(eng, frc1_planes(32, 32, 4, 550, cmax=0.7), 32, 32, max_iter=max_iter)
    check(eng, frq1_planes(32, 32, (8, 4), 553), 32, 32, 2, max_iter=max_iter)


def test_rms_eps_reaches_every_plane(eng):
    check(eng, frc1_planes(32, 32, 4, 555, cmax=0.5), 32, 32, rms_eps=50.0)


def test_stepwise_flag(eng):
    # the stepwise decoders through the same path: equal to their own single-plane calls and to the fused form
    planes = frc1_planes(37, 27, 4, 560, cmax=0.7)
    qplanes = frq1_planes(96, 64, (16, 8, 4), 563)
    with F.Engine(0, flags=F.FLAG_DECODE_STEPWISE) as st:
        a = check(st, planes, 37, 27, 2, max_iter=6)
        b = check(st, qplanes, 96, 64, max_iter=6)
    np.testing.assert_array_equal(a, check(eng, planes, 37, 27, 2, max_iter=6))
    np.testing.assert_array_equal(b, check(eng, qplanes, 96, 64, max_iter=6))


def test_one_engine_large_then_small(eng):
    # buffer reuse: the small frame's planes lie in the large frame's buffer at another pitch; no stale rows
    with F.Engine(0) as e:
        check(e, frc1_planes(200, 120, 8, 570, cmax=0.7), 200, 120, 2, ref=eng, max_iter=4)
        check(e, frc1_planes(37, 27, 4, 573, cmax=0.7), 37, 27, ref=eng, max_iter=4)
        check(e, frq1_planes(32, 32, (8, 4), 576), 32, 32, 3, ref=eng, max_iter=4)


@pytest.mark.parametrize("pad", [0, 4, 7])
def test_device_variant_into_padded_rows(eng, pad):
    import torch

    W, H, scale = 37, 27, 2
    planes = frc1_planes(W, H, 4, 580, cmax=0.7)
    s = F.pack_frc3(planes, W, H)
    want = expected(eng, planes, scale)
    big = torch.full((scale * H, 3 * scale * W + pad), 0x5A, dtype=torch.uint8, device="cuda")
    out = big[:, :3 * scale * W].view(scale * H, scale * W, 3) if pad == 0 else \
        big.as_strided((scale * H, scale * W, 3), (3 * scale * W + pad, 3, 1))
    got, it, rms = eng.decode_frc3(s, scale, out=out)
    assert got is out and it == want[1] and rms == want[2]
    host = big.cpu().numpy()
    np.testing.assert_array_equal(host[:, :3 * scale * W].reshape(scale * H, scale * W, 3), want[0])
    assert (host[:, 3 * scale * W:] == 0x5A).all()
    # a fast-path frame the same way
    planes = frc1_planes(32, 32, 4, 583, cmax=0.7)
    out = torch.zeros((32, 32, 3), dtype=torch.uint8, device="cuda")
    got, _, _ = eng.decode_frc3(F.pack_frc3(planes, 32, 32), out=out)
    np.testing.assert_array_equal(got.cpu().numpy(), expected(eng, planes)[0])


def test_out_tensor_checks(eng):
    import torch

    s = F.pack_frc3(frc1_planes(32, 32, 4, 590), 32, 32)
    with pytest.raises(F.FracError):
        eng.decode_frc3(s, out=torch.zeros((32, 31, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(F.FracError):
        eng.decode_frc3(s, out=torch.zeros((32, 32, 3), dtype=torch.int16, device="cuda"))
    with pytest.raises(F.FracError):
        eng.decode_frc3(s, out=torch.zeros((32, 32, 3), dtype=torch.uint8))
    with pytest.raises(F.FracError):  # row stride 0: below the row's bytes
        eng.decode_frc3(s, out=torch.zeros((1, 32, 3), dtype=torch.uint8, device="cuda").expand(32, 32, 3))
    with pytest.raises(F.FracError):  # pixels not packed
        eng.decode_frc3(s, out=torch.zeros((32, 32, 4), dtype=torch.uint8, device="cuda")[:, :, :3])


def raw_decode(e, s, scale, rgb, stride, nbytes):
    buf = np.frombuffer(s, np.uint8)
    it, rms = (C.c_int * 3)(), (C.c_double * 3)()
    return F.lib().frac_decode_frc3(e._ctx, buf.ctypes.data, len(buf), scale, -1, 1e-5, rgb.ctypes.data, stride, nbytes,
                                    it, rms)


def test_rgb_capacity_and_stride(eng):
    W, H, scale = 37, 27, 2
    planes = frc1_planes(W, H, 4, 600, cmax=0.7)
    s = F.pack_frc3(planes, W, H)
    row = 3 * scale * W
    stride = row + 10
    need = stride * (scale * H - 1) + row
    rgb = np.full(need, 0x5A, np.uint8)
    assert raw_decode(eng, s, scale, rgb, stride, need - 1) == -1  # one byte short of the last row
    assert raw_decode(eng, s, scale, rgb, row - 1, need) == -1      # stride below 3·scale·W
    assert (rgb == 0x5A).all()
    assert raw_decode(eng, s, 0, rgb, stride, need) == -1 and raw_decode(eng, s, 17, rgb, stride, need) == -1
    assert raw_decode(eng, s, scale, rgb, stride, need) == 0
    rows = np.concatenate([rgb, np.zeros(10, np.uint8)]).reshape(scale * H, stride)
    np.testing.assert_array_equal(rows[:, :row].reshape(scale * H, scale * W, 3), expected(eng, planes, scale)[0])
    assert (rows[:-1, row:] == 0x5A).all()
    # the container's own checks come first: a mutated header never reaches the device
    assert raw_decode(eng, s[:6] + b"\x01" + s[7:], scale, rgb, stride, need) == -1


@pytest.mark.parametrize("which", [0, 2])
def test_bad_record_index_leaves_rgb_untouched(eng, which):
    W, H = 32, 32
    planes = frc1_planes(W, H, 4, 610, cmax=0.7)
    h = F.frc1_info(planes[which])
    planes[which] = set_bits(planes[which], 5 * h["record_bits"], h["index_bits"], h["n_domains"] + 1)
    with pytest.raises(ValueError):
        codec.unpack_stream(planes[which])
    s = F.pack_frc3(planes, W, H)  # the parsers accept it: the index is checked on the device
    rgb = np.full(3 * W * H, 0x5A, np.uint8)
    assert raw_decode(eng, s, 1, rgb, 3 * W, rgb.size) == -1
    assert "domain index out of range" in F.last_error(eng._ctx)
    assert (rgb == 0x5A).all()
    good = frc1_planes(W, H, 4, 610, cmax=0.7)
    check(eng, good, W, H)  # the context stays usable


def test_decode_leaves_a_runs_results_readable(eng):
    from golden_util import plane

    with F.Engine(0, 4) as e:
        e.set_frame(plane("crop64"))
        e.set_domains(F.create_uniform_grid(64, 64, 16, 8))
        out, _ = e.search(F.create_uniform_grid(64, 64, 8, 8))
        check(e, frc1_planes(37, 27, 4, 620, cmax=0.7), 37, 27, 2, ref=eng)
        again, _ = e.fetch()
        assert again.tobytes() == out.tobytes()
        assert e.pack_frc1()[:4] == b"FRC1"


def test_end_to_end_colour_round_trip(eng):
    from fractencode_amd.color import ColorEncoder

    rng = np.random.default_rng(630)
    W, H = 64, 48
    # a smooth seeded frame (random 8×6 colours, upsampled, plus a little noise): something to encode
    coarse = rng.integers(0, 256, (6, 8, 3)).astype(np.float64)
    rgb = np.clip(np.kron(coarse, np.ones((8, 8, 1))) + rng.normal(0, 6, (H, W, 3)), 0, 255).astype(np.uint8)
    with ColorEncoder(0, 8, 16, 4) as enc:
        enc.load(rgb)
        enc.run()
        enc.sync()
        s = enc.pack_frc3()
        singles = [e.pack_frc1() for e in enc.engines]
        q, stats = enc.encode_quadtree_frc3(8, 4, 10.0)
    assert s == codec.pack_color_stream(singles, W, H)
    info = F.frc3_info(s)
    assert (info["width"], info["height"], info["kind"]) == (W, H, [1, 1, 1])
    for scale in (1, 2):
        got, it, rms = F.decode_color_stream(s, scale)
        want = expected(eng, singles, scale)
        np.testing.assert_array_equal(got, want[0])
        assert it == want[1] and rms == want[2]
    qinfo = F.frc3_info(q)
    assert qinfo["kind"] == [2, 2, 2] and len(stats) == 3 and all("items" in st for st in stats)
    qplanes = codec.unpack_color_stream(q)[0]
    got, it, rms = F.decode_color_stream(q, 2)
    want = expected(eng, qplanes, 2)
    np.testing.assert_array_equal(got, want[0])
    assert it == want[1] and rms == want[2]
