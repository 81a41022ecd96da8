"""The host restatement of yuv2rgb (tests/yuv2rgb_ref.py), CPU only, against the reference build's goldens
(tools/make_yuv2rgb_golden.py ← ImageIO::yuv2rgb, image/ImageIO.cpp:68-84): all 2^24 (y, u, v) triples, the
Lenna planes, and seeded frames of odd and smallest sizes (rgb_from_yuv_odd.npz), where the restatement's
chroma clamp stands for the reference's read of an edge-replicated plane.
"""
import json

import numpy as np
import pytest

import yuv2rgb_ref as R
from fractencode_amd.synth import sha256
from golden_util import GOLD, plane

ODD = ("67x101", "3x5", "2x2")  # width × height


def digests():
    with open(f"{GOLD}/yuv2rgb.json") as f:
        return json.load(f)


@pytest.mark.parametrize("chunk", range(4))
def test_restatement_all_triples(chunk):
    assert sha256(np.ascontiguousarray(R.all_triples_ref_quarter(chunk))) == digests()["chunks"][chunk]


def test_all_triples_layout_holds_every_triple_once():
    seen = set()
    for c in range(4):
        y, u, v = R.all_triples_planes(c)
        assert y.shape == (4096, 4096) and u.shape == v.shape == (2048, 2048)
        # per 512×512 block one luma and the 256×256 (u, v) ramp
        lum = y[::512, ::512]
        assert (y == np.repeat(np.repeat(lum, 512, 0), 512, 1)).all()
        assert (u[:256, :256] == np.arange(256)[None, :]).all() and (v[:256, :256] == np.arange(256)[:, None]).all()
        assert (u == np.tile(u[:256, :256], (8, 8))).all() and (v == np.tile(v[:256, :256], (8, 8))).all()
        seen.update(int(x) for x in lum.ravel())
    assert seen == set(range(256))


def test_restatement_lenna():
    rgb = R.yuv2rgb_ref(plane("lenna_y"), plane("lenna_u"), plane("lenna_v"))
    assert sha256(rgb) == digests()["lenna"]


@pytest.mark.parametrize("name", ODD)
def test_restatement_odd_and_smallest_frames(name):
    z = np.load(f"{GOLD}/rgb_from_yuv_odd.npz")
    y, u, v, want = (z[f"{k}_{name}"] for k in ("y", "u", "v", "rgb"))
    W, H = (int(s) for s in name.split("x"))
    assert y.shape == (H, W) and u.shape == v.shape == (H // 2, W // 2) and want.shape == (H, W, 3)
    np.testing.assert_array_equal(R.yuv2rgb_ref(y, u, v), want)


def test_fraction_fallback_is_the_same_rounding(monkeypatch):
    y, u, v = R.seeded_planes(16, 12, 5)
    want = R.yuv2rgb_ref(y, u, v)
    monkeypatch.setattr(R, "EXTENDED", False)
    np.testing.assert_array_equal(R.yuv2rgb_ref(y, u, v), want)


def test_fma_contraction_matters():
    # the source text's unfused G differs from the built reference on a few (u, v) pairs per luma value:
    # the restatement (and the kernel pinned to the same digests) must not be the unfused form
    y, u, v = R.all_triples_planes(1)
    q = (slice(0, 256), slice(0, 256))  # block 0: luma 64
    up, vp = u[q].astype(np.float64) - 128.0, v[q].astype(np.float64) - 128.0
    fused = R.convert(64.0, up, vp)
    unfused = R.convert(64.0, up, vp, fused=False)
    assert (fused[..., 1] != unfused[..., 1]).any()
    assert np.abs(fused.astype(int) - unfused.astype(int)).max() == 1


def grey_ramp_rgb() -> np.ndarray:
    g = np.arange(256, dtype=np.uint8)
    return np.repeat(np.repeat(g, 3).reshape(1, 256, 3), 2, 0)


def test_grey_ramp_round_trip_of_the_reference(oracle):
    # rgb2yuv then yuv2rgb on a grey ramp is NOT the identity in the reference: its chroma weights sum to
    # −0.001 (U) and −0.0003 (V), so a grey level's U and V fall just below 128 and truncate to 127 (128 at
    # level 0), and its luma weights give Y = g or g − 1 (test_color.py::test_fma_contraction_matters).
    # The way back then yields (Y − 2, Y + 1, Y − 2) away from the clamps.  The device round trip
    # (test_gpu_yuv2rgb.py) is held to this, the reference's, result and not to the ramp.
    rgb = grey_ramp_rgb()
    y, u, v = oracle.rgb2yuv(rgb)
    assert set(np.unique(u)) <= {127, 128} and set(np.unique(v)) <= {127, 128} and (u[:, 1:] == 127).any()
    back = R.yuv2rgb_ref(y, u, v)
    assert (back != rgb).any()
    assert np.abs(back.astype(int) - rgb.astype(int)).max() <= 3
