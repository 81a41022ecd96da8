"""numpy restatement of the colour-quality rules (include/fracenc.h, "colour quality", and the rules stated in
fractencode_amd/color.py): the rectangle the three planes' grids cover, the three channel sums over it, the
container size, the union of the planes' candidates and the size rule.  The quality rule is quality_ref.bisect
over the union.  test_color_quality_ref.py pins it on the CPU; test_gpu_color_quality.py compares the engines
with it."""
from __future__ import annotations

import math

import numpy as np

HEADER = 32


def cov(w: int, g: int) -> int:
    """What a grid of g from the origin covers of w."""
    return w - w % g


def covered(W: int, H: int, g) -> tuple[int, int]:
    """(rw, rh): the pixels from the origin of a W × H RGB frame that the grids of all three planes cover;
    g = (g_Y, g_U, g_V), the planes' FRC1 range_size or FRQ1 max_size (an int: the same for all)."""
    gy, gu, gv = (g, g, g) if np.isscalar(g) else g
    rw = min(cov(W, gy), 2 * cov(W // 2, gu), 2 * cov(W // 2, gv))
    rh = min(cov(H, gy), 2 * cov(H // 2, gu), 2 * cov(H // 2, gv))
    return rw, rh


def channel_sse(decoded: np.ndarray, ref: np.ndarray, rw: int, rh: int) -> list[int]:
    """[Σ(R − R_ref)², Σ(G − G_ref)², Σ(B − B_ref)²] of two [H, W, 3] uint8 frames over rw × rh from the origin."""
    assert decoded.shape == ref.shape and decoded.shape[2] == 3
    d = decoded[:rh, :rw].astype(np.int64) - ref[:rh, :rw].astype(np.int64)
    return [int(v) for v in (d * d).sum(axis=(0, 1), dtype=np.int64)]


def psnr(sse: int, pixels: int) -> float:
    """10·log10(255²·3·pixels / sse); inf at sse == 0."""
    return math.inf if sse == 0 else 10.0 * math.log10(255.0 ** 2 * 3 * pixels / sse)


def max_sse_of(min_psnr: float, pixels: int) -> int:
    """ColorEncoder.rate_quality's translation of a PSNR target."""
    return int(math.floor(255.0 ** 2 * 3 * pixels / 10.0 ** (min_psnr / 10.0)))


def container_bytes(plane_bytes) -> int:
    """The FRC3 container of three plane streams of these sizes: the header and each stream padded to 8."""
    assert len(plane_bytes) == 3
    return HEADER + sum((int(n) + 7) // 8 * 8 for n in plane_bytes)


def union(candidates) -> np.ndarray:
    """The sorted distinct union of the planes' candidate lists (== on the double)."""
    return np.unique(np.concatenate([np.asarray(c, np.float64) for c in candidates]))


def fit_size(sizes, max_bytes: int) -> int | None:
    """The size rule over the container sizes of the union in ascending candidate order: the index of the least
    candidate whose container has at most max_bytes, every candidate looked at; None when none fits."""
    for i, s in enumerate(sizes):
        if int(s) <= max_bytes:
            return i
    return None
