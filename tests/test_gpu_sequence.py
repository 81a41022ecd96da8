"""The closed loop: SequenceEncoder (I frames iteratively decoded, P frames coded against the previous reconstruction
and applied once) and decode_sequence over its FRCS container.

Four 96×64 frames: a value-noise frame, a brightness-shifted copy, a locally perturbed copy of that, and a second
shift.  With gop = 3 they are I, P, P, I.  What the decoder makes of the container equals, byte for byte, the
encoder's own reconstruction after each push: no drift.  The P frames' planes are also checked against inter_ref
(the oracle's decoder), and their inter_error against the host's sum."""
import functools

import numpy as np
import pytest
import torch

import fractencode_amd as F
import inter_ref as R
import quality_ref as QR
from fractencode_amd import codec
from fractencode_amd.synth import value_noise

pytestmark = pytest.mark.gpu

W, H = 96, 64


def _frames():
    base = value_noise(W, H, 77)
    f1 = np.clip(base.astype(np.int32) + 9, 0, 255).astype(np.uint8)
    f2 = f1.copy()
    f2[16:40, 24:72] = np.random.default_rng(5).integers(0, 256, (24, 48), dtype=np.uint8)
    f3 = np.clip(f2.astype(np.int32) - 14, 0, 255).astype(np.uint8)
    return [base, f1, f2, f3]


@functools.lru_cache(maxsize=None)
def _run():
    """(frames, [(kind, stream)], the reconstruction after each push, the container)."""
    frames = _frames()
    out, recs = [], []
    with F.SequenceEncoder(gop=3, max_size=16, min_size=4) as enc:
        for k, f in enumerate(frames):
            # numpy and device frames alike
            plane = f if k % 2 == 0 else torch.from_numpy(f).to("cuda:0")
            out.append(enc.push(plane))
            recs.append(enc.reconstruction().cpu().numpy().copy())
        data = enc.pack()
    return frames, out, recs, data


def test_kinds_and_container():
    _, out, _, data = _run()
    assert [k for k, _ in out] == ["I", "P", "P", "I"]
    frames, h = codec.unpack_sequence(data)
    assert frames == out and (h["width"], h["height"]) == (W, H)
    for _, s in out:
        assert s[:4] == b"FRQ1" and F.frq1_info(s)["width"] == W


def test_decode_sequence_is_the_encoders_reconstruction(oracle):
    _, out, recs, data = _run()
    planes = F.decode_sequence(data)
    assert len(planes) == 4
    for k in range(4):
        np.testing.assert_array_equal(planes[k], recs[k])
    # and each plane is what the checkers make of its stream
    with F.Engine(0, 4) as e:
        for k, (kind, s) in enumerate(out):
            if kind == "I":
                np.testing.assert_array_equal(e.decode_frq1(s)[0], recs[k])
            else:
                np.testing.assert_array_equal(R.apply_stream(oracle, s, recs[k - 1]), recs[k])
    assert (recs[1] != recs[0]).any() and (recs[2] != recs[1]).any()


def test_p_streams_inter_error_is_the_reconstructions_error():
    frames, out, recs, _ = _run()
    with F.Engine(0, 4) as e:
        for k, (kind, s) in enumerate(out):
            if kind != "P":
                continue
            e.set_planes(recs[k - 1], frames[k])
            got = e.inter_error(s)
            sse, _ = QR.sse(recs[k], frames[k], 16)
            assert (got["sse"], got["pixels"]) == (sse, W * H)


def test_decode_sequence_at_scale_2(oracle):
    _, out, _, data = _run()
    planes = F.decode_sequence(data, scale=2)
    assert [p.shape for p in planes] == [(2 * H, 2 * W)] * 4
    np.testing.assert_array_equal(planes[0], F.decode_stream(out[0][1], scale=2)[0])
    np.testing.assert_array_equal(planes[1], R.apply_stream(oracle, out[1][1], planes[0], 2))
