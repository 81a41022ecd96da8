"""CPU checks of the colour-quality feature: color_quality_ref.py's restatement of the rules pinned on hand-made
inputs and on the covered rectangles of the shapes test_gpu_color_quality.py runs, and the library's three entry
points at the ABI boundary (no device call)."""
import ctypes as C
import math

import numpy as np

import color_quality_ref as CR
import fractencode_amd as F
from fractencode_amd import codec

SYMBOLS = ("frac_decode_error_frc3", "frac_decode_error_frc3_device", "frac_quadtree_rate_candidates")


def test_covered_rectangle():
    assert CR.covered(96, 64, 16) == (96, 64)
    assert CR.covered(98, 74, 16) == (96, 64)           # Y 96 × 64; chroma 49 × 37 covers 48 × 32, doubled
    assert CR.covered(70, 58, 16) == (64, 32)           # chroma 35 × 29 covers 32 × 16: the chroma grid decides
    assert CR.covered(37, 27, 4) == (32, 24)            # chroma 18 × 13 covers 16 × 12
    assert CR.covered(38, 28, (3, 7, 7)) == (28, 27)    # width from chroma (2 · 14), height from luma: odd
    assert CR.covered(38, 28, (3, 7, 9)) == (28, 18)    # chroma 19 × 14: U decides the width, V the height
    assert CR.covered(12, 12, (4, 8, 8)) == (0, 0)      # chroma 6 × 6 under 8
    assert CR.covered(12, 40, (4, 4, 8)) == (0, 32)     # one side without a range: no pixel
    assert CR.covered(2048, 2048, 16) == (2048, 2048)
    # the chroma cell (x / 2, y / 2) of every covered pixel lies inside the chroma plane
    for W in range(2, 41):
        for g in ((1, 1, 1), (3, 7, 7), (4, 4, 4), (16, 16, 16), (2, 5, 3)):
            rw, _ = CR.covered(W, W, g)
            assert rw <= W and (rw == 0 or (rw - 1) // 2 < W // 2)


def test_channel_sums():
    a = np.zeros((5, 6, 3), np.uint8)
    b = np.zeros((5, 6, 3), np.uint8)
    a[0, 0] = (255, 0, 10)
    b[0, 0] = (0, 3, 250)       # 255², 3², 240² (no uint8 wrap-around)
    a[2, 3, 1] = 7              # G only
    a[4, 0] = a[0, 5] = 200     # outside 4 × 4
    assert CR.channel_sse(a, b, 4, 4) == [255 * 255, 9 + 49, 240 * 240]
    assert CR.channel_sse(a, b, 6, 5) == [255 * 255 + 2 * 200 * 200, 9 + 49 + 2 * 200 * 200,
                                          240 * 240 + 2 * 200 * 200]
    assert CR.channel_sse(a, b, 0, 0) == [0, 0, 0] and CR.channel_sse(a, b, 4, 0) == [0, 0, 0]
    assert CR.channel_sse(a, b, 3, 3) == [255 * 255, 9, 240 * 240]  # an odd rectangle: (2, 3) lies outside
    full = CR.channel_sse(np.full((64, 64, 3), 255, np.uint8), np.zeros((64, 64, 3), np.uint8), 64, 64)
    assert full == [64 * 64 * 255 * 255] * 3


def test_psnr_and_its_bound():
    assert CR.psnr(0, 100) == math.inf
    assert CR.psnr(3 * 100, 100) == 10.0 * math.log10(255.0 ** 2)  # MSE 1 per sample
    assert CR.max_sse_of(20.0, 96 * 64) == int(np.floor(65025.0 * 3 * 96 * 64 / 100.0))
    assert CR.max_sse_of(30.0, 0) == 0
    # the translation is the single-plane one at three samples per pixel
    import quality_ref as QR
    assert CR.max_sse_of(33.0, 1000) == QR.max_sse_of(33.0, 3000)


def test_container_bytes_equal_the_packer():
    assert CR.container_bytes([64, 64, 64]) == 32 + 192
    assert CR.container_bytes([65, 71, 72]) == 32 + 72 + 72 + 72
    assert CR.container_bytes([1, 8, 9]) == 32 + 8 + 8 + 16
    from frq1_synth import synth_quadtree_stream
    from frc1_synth import synth_stream
    planes = [synth_quadtree_stream(98, 74, 1, (8, 4), T=4), synth_stream(49, 37, 4, 8, 4, 2),
              synth_quadtree_stream(49, 37, 3, (16, 8, 4), T=4)]
    assert any(len(p) % 8 for p in planes)  # the padding shows
    assert CR.container_bytes([len(p) for p in planes]) == len(codec.pack_color_stream(planes, 98, 74))


def test_union_of_candidates():
    u = CR.union([[0.0, 1.5, 3.0], [0.0, 1.5, 2.0], [0.0]])
    assert u.dtype == np.float64 and u.tolist() == [0.0, 1.5, 2.0, 3.0]
    near = np.nextafter(1.5, 2.0)
    assert CR.union([[0.0, 1.5], [0.0, near], [0.0]]).tolist() == [0.0, 1.5, near]  # == on the double
    assert CR.union([[0.0], [0.0], [0.0]]).tolist() == [0.0]


def test_size_rule():
    sizes = [900, 700, 500, 300]  # monotone: larger split distances give smaller containers
    assert CR.fit_size(sizes, 900) == 0 and CR.fit_size(sizes, 899) == 1 and CR.fit_size(sizes, 300) == 3
    assert CR.fit_size(sizes, 299) is None
    # not monotone (the padding, or a plane whose size rises): still the least candidate that fits
    sizes = [900, 500, 700, 300]
    assert CR.fit_size(sizes, 600) == 1 and CR.fit_size(sizes, 499) == 3 and CR.fit_size(sizes, 750) == 1
    assert CR.fit_size([], 10) is None


def test_library_exports_the_colour_quality_symbols():
    lib = F.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert getattr(lib, name).restype is C.c_int
    assert lib.frac_abi_version() == 9


def test_a_null_context_is_invalid():
    lib = F.lib()
    buf = (C.c_uint8 * 64)()
    rgb = (C.c_uint8 * 64)()
    assert lib.frac_decode_error_frc3(None, buf, 64, rgb, 12, -1, 1e-5, None, None, None, None) == -1
    assert lib.frac_decode_error_frc3_device(None, buf, 64, rgb, 12, -1, 1e-5, None, None, None, None) == -1
    assert lib.frac_quadtree_rate_candidates(None, None, 0, None) == -1
