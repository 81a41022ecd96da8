"""frac_inter_error (a stream applied once to the plane the domains lie on, compared on the device with the plane the
ranges lie on) and frac_set_planes_device.

The expected sums are quality_ref.sse of inter_ref's plane (the oracle's decoder on a stacked plane) against the
target plane over quality_ref.covered: exact integers.  One fast and one general FRC1 stream, a quadtree stream on
the fast route, one with margins (the rectangle is smaller than the frame) and a leafless one (no pixel)."""
import functools

import numpy as np
import pytest
import torch

import fractencode_amd as F
import frc1_synth as S1
import frq1_synth as SQ
import inter_ref as R
import quality_ref as QR

pytestmark = pytest.mark.gpu

CASES = {
    "frc1_fast": lambda: S1.fast_stream(4),       # 100×36, n = 4: inter_frc1, W no multiple of 64
    "frc1_general": lambda: S1.other_stream(4),   # 72×40, domain-less records: inter_apply + plane_sse_blocks
    "96x64": lambda: SQ.case_stream("96x64"),     # inter_frq1
    "70x58_margins": lambda: SQ.case_stream("70x58_margins"),
    "15x15_none": lambda: SQ.case_stream("15x15_none"),
}


@functools.lru_cache(maxsize=None)
def _stream(name):
    return CASES[name]()


def _expected(oracle, stream, src, tgt):
    _, W, H, g = R.stream_records(stream)
    cw, ch = QR.covered(W, H, g)
    if cw * ch == 0:
        return 0, 0
    return QR.sse(R.apply_stream(oracle, stream, src), tgt, g)[0], cw * ch


@pytest.mark.parametrize("name", list(CASES))
def test_inter_error(oracle, name):
    s = _stream(name)
    _, W, H, _ = R.stream_records(s)
    src, tgt = R.random_plane(W, H, 21), R.random_plane(W, H, 22)
    with F.Engine(0, 8) as e:
        e.set_planes(src, tgt)
        sse, pixels = _expected(oracle, s, src, tgt)
        got = e.inter_error(s)
        assert (got["sse"], got["pixels"]) == (sse, pixels)
        assert got["psnr"] == F._psnr(sse, pixels)
        if name == "15x15_none":
            assert (sse, pixels) == (0, 0)
        elif name == "70x58_margins":
            assert pixels == 64 * 48 < W * H
        else:
            assert pixels == W * H and sse > 0
        assert e.inter_error(s) == got  # the total is zeroed per call
        # a target that equals the applied plane: a zero sum
        e.set_planes(src, R.apply_stream(oracle, s, src))
        assert e.inter_error(s)["sse"] == 0
        # one plane: the quantized collage error
        e.set_frame(tgt)
        sse1, pixels1 = _expected(oracle, s, tgt, tgt)
        got = e.inter_error(s)
        assert (got["sse"], got["pixels"]) == (sse1, pixels1)
        # NULL outputs
        buf = np.frombuffer(s, np.uint8)
        assert F.lib().frac_inter_error(e._ctx, buf.ctypes.data, len(buf), None, None) == 0


def test_inter_error_state_and_frame_size():
    s = _stream("96x64")
    with F.Engine(0, 8) as e:
        with pytest.raises(F.FracError, match="rc=-3.*no planes set"):
            e.inter_error(s)
        e.set_frame(R.random_plane(100, 36, 1))
        with pytest.raises(F.FracError, match="rc=-1.*stream's frame is 96x64"):
            e.inter_error(s)
        assert e.inter_error(_stream("frc1_fast"))["pixels"] == 3600
        e.set_planes(R.random_plane(96, 64, 1), R.random_plane(100, 36, 2))  # the source fits, the target does not
        with pytest.raises(F.FracError, match="rc=-1.*stream's frame is 96x64"):
            e.inter_error(s)
        with pytest.raises(F.FracError, match="rc=-1"):
            e.inter_error(s[:-1])
        with pytest.raises(F.FracError, match="rc=-1.*neither"):
            e.inter_error(b"FRC3" + s[4:])


def test_inter_error_is_a_reader():
    W, H = 96, 64
    src, tgt = R.random_plane(W, H, 31), R.random_plane(W, H, 32)
    doms, rngs = F.create_uniform_grid(W, H, 16, 8), F.create_uniform_grid(W, H, 8, 8)
    with F.Engine(0, 4) as e:
        e.set_planes(src, tgt)
        e.set_domains(doms)
        items, _ = e.search(rngs)
        stream = e.pack_frc1()
        first = e.inter_error(stream)
        again, _ = e.fetch()
        assert again.tobytes() == items.tobytes()
        assert e.pack_frc1() == stream and e.inter_error(stream) == first


def test_set_planes_device():
    W, H = 64, 48
    src, tgt = R.random_plane(W, H, 41), R.random_plane(W, H, 42)
    doms, rngs = F.create_uniform_grid(W, H, 8, 4), F.create_uniform_grid(W, H, 4, 4)

    def records(e, a, b):
        e.set_planes(a, b)
        e.set_domains(doms)
        return e.search(rngs)[0]

    with F.Engine(0, 4) as e:
        want = records(e, src, tgt)
    sbuf = torch.full((H, 80), 0xA5, dtype=torch.uint8, device="cuda:0")
    tbuf = torch.full((H, 71), 0x5A, dtype=torch.uint8, device="cuda:0")
    d_src, d_tgt = sbuf[:, 3:3 + W], tbuf[:, 7:]
    d_src.copy_(torch.from_numpy(src))
    d_tgt.copy_(torch.from_numpy(tgt))
    with F.Engine(0, 4) as e:
        got = records(e, d_src, d_tgt)
        assert got.tobytes() == want.tobytes()
        assert not np.array_equal(got, records(e, d_tgt, d_src))  # the planes' roles matter
        # a setter: it ends the run's results; a failed check changes nothing
        e.set_planes(d_src, d_tgt)
        with pytest.raises(F.FracError, match="rc=-3"):
            e.fetch()
        e.run()
        assert e.fetch()[0].tobytes() == want.tobytes()
        rc = F.lib().frac_set_planes_device(e._ctx, d_src.data_ptr(), W, H, W - 1, d_tgt.data_ptr(), W, H, 71)
        assert rc == -1
        assert e.fetch()[0].tobytes() == want.tobytes()
        small = torch.zeros((8, 8), dtype=torch.uint8, device="cuda:0")
        with pytest.raises(F.FracError, match="CUDA uint8"):
            e.set_planes(small, np.zeros((8, 8), np.uint8))
        with pytest.raises(F.FracError, match="rows must be contiguous"):
            e.set_planes(small, tbuf.t()[:8, :8])
        assert e._frame_wh == (W, H)  # a refused call leaves the wrapper's frame size too
        # the stream of the device planes' run is measured against them
        stream = e.pack_frc1()
        with F.Engine(0, 4) as h:
            h.set_planes(src, tgt)
            assert e.inter_error(stream) == h.inter_error(stream)
