"""Host restatement of the device yuv2rgb (fracenc_color.hip ← ImageIO::yuv2rgb, image/ImageIO.cpp:68-84),
and the all-triples layout of tools/make_yuv2rgb_golden.py (data generator, shared by tests).

The built reference contracts every product into its addition:

    R = clamp(fma( 1.402, v', y)),  G = clamp(fma(-0.714, v', fma(-0.344, u', y))),  B = clamp(fma( 1.772, u', y))

with u' = u − 128, v' = v − 128.  In a long double with a 64-bit significand c·k + y is exact for these
operands (a 53-bit constant times an integer of at most 8 bits, plus a value below 2^9 whose last bit is no
finer than the product's), so rounding it to float64 once is the fused result.  Without such a long double
the same rounding is done per distinct operand triple in rational arithmetic.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

L = np.longdouble
EXTENDED = np.finfo(L).nmant >= 63


def _fma(c: float, k: np.ndarray, y: np.ndarray) -> np.ndarray:
    """fl64(c·k + y), one rounding; k integer-valued float64, y float64 (broadcast together)."""
    k, y = np.broadcast_arrays(np.asarray(k, np.float64), np.asarray(y, np.float64))
    if EXTENDED:
        return (L(c) * k.astype(L) + y.astype(L)).astype(np.float64)
    # slow path: each distinct (k, y) pair once, exactly
    pairs, inv = np.unique(np.stack([k.ravel(), y.ravel()], 1), axis=0, return_inverse=True)
    fc = Fraction(c)
    vals = np.array([float(fc * Fraction(float(a)) + Fraction(float(b))) for a, b in pairs], np.float64)
    return vals[inv.reshape(-1)].reshape(k.shape)


def _clamp(x: np.ndarray) -> np.ndarray:
    """ImageIO.cpp:11-13: < 0 → 0, > 255 → 255, otherwise truncate."""
    return np.where(x < 0.0, 0, np.where(x > 255.0, 255, np.trunc(np.clip(x, 0.0, 255.0)))).astype(np.uint8)


def convert(y, up, vp, fused: bool = True) -> np.ndarray:
    """RGB (last axis) of float64 y and u' = u − 128, v' = v − 128, broadcast together.  fused=False is the
    source text's unfused form, which the built reference is not."""
    y, up, vp = (np.asarray(a, np.float64) for a in (y, up, vp))
    if fused:
        r = _fma(1.402, vp, y)
        g = _fma(-0.714, vp, _fma(-0.344, up, y))
        b = _fma(1.772, up, y)
    else:
        r = y + 1.402 * vp
        g = y - 0.344 * up - 0.714 * vp
        b = y + 1.772 * up
    return np.stack([_clamp(r), _clamp(g), _clamp(b)], -1)


def yuv2rgb_ref(y: np.ndarray, u: np.ndarray, v: np.ndarray, fused: bool = True) -> np.ndarray:
    """[H, W, 3] from Y [H, W] and U, V of any equal size (at least 1×1): pixel (x, y) reads chroma cell
    (x/2, y/2) clamped to the chroma planes' last column and row."""
    H, W = y.shape
    ch, cw = u.shape
    assert v.shape == u.shape and ch >= 1 and cw >= 1
    cy = np.minimum(np.arange(H) // 2, ch - 1)[:, None]
    cx = np.minimum(np.arange(W) // 2, cw - 1)[None, :]
    return convert(y.astype(np.float64), u[cy, cx].astype(np.float64) - 128.0, v[cy, cx].astype(np.float64) - 128.0,
                   fused)


# ---- all 2^24 (y, u, v) triples in 4 chunks -------------------------------------------------------
# Chunk c is a 4096×4096 frame of 8×8 blocks; block k (row-major) is a 512×512 Y block of luma 64c + k over
# 256×256 chroma cells with U[j, i] = i and V[j, i] = j.  Every pixel of a 2×2 quad has the same triple, so
# the digests are taken over rgb[::2, ::2].

def all_triples_planes(chunk: int):
    k = np.arange(8)
    luma = (64 * chunk + 8 * k[:, None] + k[None, :]).astype(np.uint8)
    y = np.repeat(np.repeat(luma, 512, 0), 512, 1)
    ramp = np.tile(np.arange(256, dtype=np.uint8), 8)
    u = np.ascontiguousarray(np.broadcast_to(ramp[None, :], (2048, 2048)))
    v = np.ascontiguousarray(np.broadcast_to(ramp[:, None], (2048, 2048)))
    return y, u, v


def all_triples_ref_quarter(chunk: int) -> np.ndarray:
    """yuv2rgb_ref(*all_triples_planes(chunk))[::2, ::2] without converting every pixel four times."""
    y, u, v = all_triples_planes(chunk)
    return convert(y[::2, ::2].astype(np.float64), u.astype(np.float64) - 128.0, v.astype(np.float64) - 128.0)


def seeded_planes(W: int, H: int, seed: int, cw: int | None = None, ch: int | None = None):
    """Random Y [H, W] and U, V [ch, cw] (default H/2 × W/2)."""
    rng = np.random.default_rng(seed)
    cw, ch = W // 2 if cw is None else cw, H // 2 if ch is None else ch
    return (rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8),
            rng.integers(0, 256, (ch, cw), dtype=np.uint8))
