"""numpy restatement of the decoded-quality rules (include/fracenc.h, "decoded quality"): the covered
rectangle, the block sums of squared error over it, and the quality fit's bisection over a list of decoded
errors.  test_quality_ref.py pins it on the CPU; test_gpu_quality.py compares the engines with it."""
from __future__ import annotations

import numpy as np


def covered(W: int, H: int, g: int) -> tuple[int, int]:
    """(width, height) of what a g × g grid from the origin covers of a W × H frame."""
    return W - W % g, H - H % g


def sse(decoded: np.ndarray, frame: np.ndarray, g: int) -> tuple[int, np.ndarray]:
    """(total, int64 [H // g, W // g] block sums) of (decoded − frame)² over the covered rectangle."""
    assert decoded.shape == frame.shape
    H, W = frame.shape
    cw, ch = covered(W, H, g)
    d = decoded[:ch, :cw].astype(np.int64) - frame[:ch, :cw].astype(np.int64)
    blocks = (d * d).reshape(ch // g, g, cw // g, g).sum(axis=(1, 3), dtype=np.int64)
    return int(blocks.sum(dtype=np.int64)), blocks


def bisect(E, max_sse: int) -> tuple[int | None, int]:
    """frac_quadtree_rate_quality's rule over the decoded errors E[i] of the candidates in ascending order:
    (the answer's index, or None when the smallest candidate fails; the probes made)."""
    m = len(E)
    assert m >= 1
    probes = 1
    if E[m - 1] <= max_sse:
        return m - 1, probes
    if m > 1:
        probes += 1
    if m == 1 or E[0] > max_sse:
        return None, probes
    lo, hi = 0, m - 1
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        probes += 1
        if E[mid] <= max_sse:
            lo = mid
        else:
            hi = mid
    return lo, probes


def max_sse_of(min_psnr: float, pixels: int) -> int:
    """Engine.rate_quality's translation of a PSNR target."""
    import math

    return int(math.floor(255.0 ** 2 * pixels / 10.0 ** (min_psnr / 10.0)))
