"""Colour frames: main.cpp's --color mode on the device.

The reference loads a PNG, converts it with ImageIO::rgb2yuv (image/ImageIO.cpp:43-58)
and encodes the three planes independently, each with its own grids and classifier
(main.cpp:184-196 → encode_image2, main.cpp:142-180).  Here the RGB frame is uploaded
once, converted on the device (frac_rgb_to_yuv_device), and the Y, U and V searches
are enqueued on three engines that share one HIP stream, so the searches run in turn: the luma
search alone fills the GPU, and letting the small chroma searches overlap it on streams of their
own measured slower (C5: 12.73 vs 12.54 ms per frame for the three searches, 13.32 vs 12.69 ms with
the conversion; profiles/r03/session5/paths.jsonl).  streams="own" keeps one stream per engine.

The way back: pack_frc3 / encode_quadtree_frc3 put the three planes' streams into one FRC3 container
(codec.py), which Engine.decode_frc3 / decode_color_stream decode to RGB on the device.
"""
from __future__ import annotations

import math

import numpy as np

from . import ENGINE_AUTO, Engine, FracError, create_uniform_grid, pack_frc3

PLANES = ("Y", "U", "V")


class ColorEncoder:
    """Three-plane encoder.  load(rgb) → run() → sync() → fetch(), engines reused across frames."""

    def __init__(self, device: int = 0, range_size: int = 8, domain_size: int | None = None, transforms: int = 4,
                 use_classifier: bool = False, rms_threshold: float = 0.0, s_max: float = -1.0,
                 engine: int = ENGINE_AUTO, timing: bool = False, streams: str = "shared"):
        if streams not in ("shared", "own"):
            raise ValueError(f"streams must be 'shared' or 'own', not {streams!r}")
        self.device = device
        self.range_size = range_size
        self.domain_size = domain_size or 2 * range_size
        self.use_classifier = use_classifier
        self.engines = [Engine(device, transforms, use_classifier, rms_threshold, s_max, engine, timing) for _ in PLANES]
        self._stream = None
        if streams == "shared":
            import torch

            self._stream = torch.cuda.Stream(torch.device("cuda", device))
            for e in self.engines:
                e.set_stream(self._stream.cuda_stream)
        self.planes = None
        self.rgb = None
        self.ranges = None

    def close(self) -> None:
        for e in self.engines:
            e.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def load(self, rgb) -> None:
        """rgb: numpy uint8 [H, W, 3] or a CUDA uint8 tensor [H, W, 3]; converted on the device."""
        import torch

        if not (hasattr(rgb, "is_cuda") and rgb.is_cuda):
            rgb = torch.from_numpy(np.ascontiguousarray(rgb, dtype=np.uint8)).to(f"cuda:{self.device}")
        planes = self.engines[0].rgb_to_yuv(rgb)
        self.planes = planes
        self.rgb = rgb  # kept on the device: decode_error compares against it
        self.frame_wh = (int(rgb.shape[1]), int(rgb.shape[0]))
        n, d = self.range_size, self.domain_size
        geom = [tuple(p.shape) for p in planes]
        same = geom == getattr(self, "_geom", None)
        if not same:
            self.ranges = []
        sharded = getattr(self, "_sharded", False)
        self._sharded = False
        for k, (e, p) in enumerate(zip(self.engines, planes)):
            H, W = p.shape
            e.set_frame(p)
            if same:
                if sharded:  # encode_sharded left each engine holding only this rank's shard
                    e.set_ranges(self.ranges[k])
                continue  # a frame of the same geometry keeps the grids (and, classifier off, the prepared state)
            # categories −1: with the classifier on, the engine classifies every item on the
            # device plane (main.cpp:155-162 preclassifies both grids on the same plane)
            doms = create_uniform_grid(W, H, d, d // 2)
            rngs = create_uniform_grid(W, H, n, n)
            e.set_domains(doms)
            e.set_ranges(rngs)
            self.ranges.append(rngs)
        self._geom = geom

    def run(self) -> None:
        """Enqueue the three searches (asynchronous; on the shared stream, or each engine's own)."""
        for e in self.engines:
            e.run()

    def sync(self) -> None:
        for e in self.engines:
            e.sync()

    def fetch(self):
        """[(encode items, stats)] for Y, U, V."""
        return [e.fetch() for e in self.engines]

    def encode_sharded(self, rank: int, world: int, device=None, group=None):
        """C5 over several GPUs (BASELINE configs[4]): after load(), every rank searches its
        contiguous shard of each plane's ranges and the (domain, transform, s, o, rms) tuples are
        all-gathered (fractencode_amd.distributed); returns the full Y, U, V encode_item_t arrays
        on every rank.  `device` = a CUDA device for nccl, None for gloo (host tuples)."""
        from .distributed import encode_sharded

        self._sharded = True  # the next load() of a same-geometry frame restores the full range lists
        out = []
        for e, rngs, p in zip(self.engines, self.ranges, self.planes):
            H, W = p.shape
            doms = create_uniform_grid(W, H, self.domain_size, self.domain_size // 2)
            out.append(encode_sharded(e, rngs, doms, rank, world, device=device, group=group))
        return out

    def pack_frc3(self, contrast_bits: int = 5, brightness_bits: int = 7) -> bytes:
        """After run() and sync(): each engine's pack_frc1 (quantized and packed on the device), the three
        streams in one FRC3 container."""
        if self.planes is None:
            raise FracError("pack_frc3: no frame loaded")
        return pack_frc3([e.pack_frc1(contrast_bits, brightness_bits) for e in self.engines], *self.frame_wh)

    def encode_quadtree_frc3(self, max_size: int = 16, min_size: int = 4, split_distance: float = 10.0,
                             contrast_bits: int = 5, brightness_bits: int = 7, host_pack: bool | None = None):
        """After load(): each engine's encode_quadtree_stream (an FRQ1 stream per plane) in one FRC3 container.
        host_pack: that method's switch between the host and the device packer (None: its default).
        Returns (container bytes, [summed stats dict] for Y, U, V)."""
        if self.planes is None:
            raise FracError("encode_quadtree_frc3: no frame loaded")
        kw = {} if host_pack is None else {"host_pack": host_pack}
        parts = [e.encode_quadtree_stream(max_size, min_size, split_distance, contrast_bits, brightness_bits, **kw)
                 for e in self.engines]
        return pack_frc3([s for s, _ in parts], *self.frame_wh), [st for _, st in parts]

    # ---- colour quality: one split distance steers the three planes -----------------------------------------
    #
    # quadtree_rate() builds a rate state on each engine.  The candidates of a colour frame are the sorted distinct
    # union c[0] < … < c[m − 1] of the three planes' candidates (Engine.rate_candidates, == on the double): between
    # two neighbours no plane's partition changes, so the union lists every container a split distance can give.
    # The container at a split distance t is pack_frc3 of the three engines' rate_stream(t); its size is
    # 32 + Σ_k pad8(size_k), pad8 rounding up to a multiple of 8.
    #   Size rule (rate_fit): the answer is the least candidate of the union whose container has at most max_bytes,
    #   found by evaluating every candidate (one rate_sizes call per plane over the whole union, a minimum on the
    #   host), so it is exact whether or not the size is monotone.  Nothing fits: FracError naming the smallest
    #   container.
    #   Quality rule (rate_quality): frac_quadtree_rate_quality's bisection (include/fracenc.h) over the union,
    #   with E(i) the summed RGB sse of the container at c[i] from decode_error against the RGB frame of load():
    #   probe m − 1, the answer if it meets; else probe 0 (m > 1), FracError if it fails (or m = 1); then lo = 0,
    #   hi = m − 1, while hi − lo > 1 probe mid = lo + (hi − lo) // 2, lo = mid if it meets, else hi = mid; the
    #   answer is lo.  The answer meets the target and the next larger candidate does not (unless it is the
    #   largest); E is not monotone, so it need not be the largest candidate that meets it.  A PSNR target becomes
    #   max_sse = floor(255²·3·pixels / 10^(psnr/10)), pixels the covered rectangle's area.

    def decode_error(self, stream, max_iter: int = -1, rms_eps: float = 1e-5) -> dict:
        """Engine.decode_error_frc3 of an FRC3 container against the RGB frame of load(), which stayed on the
        device."""
        if self.planes is None:
            raise FracError("decode_error: no frame loaded")
        return self.engines[0].decode_error_frc3(stream, self.rgb, max_iter, rms_eps)

    def quadtree_rate(self, max_size: int = 16, min_size: int = 4):
        """After load(): Engine.quadtree_rate on each plane's engine (three frac_quadtree_rate_builds); afterwards
        the rate_* methods below answer for any split distance without a search.  Returns [summed stats dict] for
        Y, U, V."""
        if self.planes is None:
            raise FracError("quadtree_rate: no frame loaded")
        self._rate_geom = (max_size, min_size)
        return [e.quadtree_rate(max_size, min_size) for e in self.engines]

    def rate_candidates(self) -> np.ndarray:
        """The sorted distinct union (float64, == on the double) of the three planes' candidates."""
        return np.unique(np.concatenate([e.rate_candidates() for e in self.engines]))

    def rate_sizes(self, splits, contrast_bits: int = 5, brightness_bits: int = 7):
        """Per split distance in `splits` the size of the container rate_stream would return there:
        (container bytes uint64 [n] = 32 + Σ_k pad8(plane bytes), plane bytes uint64 [n, 3])."""
        t = np.ascontiguousarray(splits, dtype=np.float64).reshape(-1)
        planes = np.stack([e.rate_sizes(t, contrast_bits, brightness_bits)[0] for e in self.engines], axis=1)
        pad8 = (planes + np.uint64(7)) & ~np.uint64(7)
        return np.uint64(32) + pad8.sum(axis=1, dtype=np.uint64), planes

    def rate_stream(self, split: float, contrast_bits: int = 5, brightness_bits: int = 7) -> bytes:
        """The FRC3 container at `split` from the rate states: pack_frc3 of the three engines' rate_stream."""
        return pack_frc3([e.rate_stream(split, contrast_bits, brightness_bits) for e in self.engines], *self.frame_wh)

    def rate_fit(self, max_bytes: int, contrast_bits: int = 5, brightness_bits: int = 7):
        """The size rule: the least candidate of the union whose container has at most max_bytes, every candidate
        evaluated → (split distance, container bytes, [plane bytes]·3).  FracError when nothing fits."""
        cands = self.rate_candidates()
        size, planes = self.rate_sizes(cands, contrast_bits, brightness_bits)
        fits = np.flatnonzero(size <= np.uint64(max_bytes))
        if not len(fits):
            raise FracError(f"rate_fit: no split distance fits {max_bytes} bytes; the smallest container has "
                            f"{int(size.min())} bytes")
        i = int(fits[0])
        return float(cands[i]), int(size[i]), [int(v) for v in planes[i]]

    def rate_errors(self, splits, contrast_bits: int = 5, brightness_bits: int = 7, max_iter: int = -1,
                    rms_eps: float = 1e-5):
        """Per split distance in `splits` decode_error(rate_stream(t)):
        (summed sse uint64 [n], channel sse uint64 [n, 3], container bytes uint64 [n])."""
        t = np.ascontiguousarray(splits, dtype=np.float64).reshape(-1)
        sse, chan, size = np.zeros(len(t), np.uint64), np.zeros((len(t), 3), np.uint64), np.zeros(len(t), np.uint64)
        for i, v in enumerate(t):
            stream = self.rate_stream(float(v), contrast_bits, brightness_bits)
            err = self.decode_error(stream, max_iter, rms_eps)
            sse[i], chan[i], size[i] = err["sse"], err["channel_sse"], len(stream)
        return sse, chan, size

    def _rate_pixels(self) -> int:
        """The area the three level-0 grids of the rate states cover together (0 before quadtree_rate)."""
        W, H = self.frame_wh
        g = getattr(self, "_rate_geom", (0, 0))[0]
        if not g:
            return 0
        return min(W - W % g, 2 * (W // 2 - W // 2 % g)) * min(H - H % g, 2 * (H // 2 - H // 2 % g))

    def _quality_fit(self, max_sse, min_psnr, contrast_bits, brightness_bits, max_iter, rms_eps):
        if (max_sse is None) == (min_psnr is None):
            raise ValueError("rate_quality: exactly one of max_sse and min_psnr")
        if max_sse is None:
            max_sse = int(math.floor(255.0 ** 2 * 3 * self._rate_pixels() / 10.0 ** (min_psnr / 10.0)))
        cands = self.rate_candidates()
        m = len(cands)
        made = 0

        def probe(i):
            nonlocal made
            made += 1
            stream = self.rate_stream(float(cands[i]), contrast_bits, brightness_bits)
            return i, stream, self.decode_error(stream, max_iter, rms_eps)

        best = probe(m - 1)
        if best[2]["sse"] > max_sse:
            first = probe(0) if m > 1 else best
            if first[2]["sse"] > max_sse:
                raise FracError(f"rate_quality: the decoded error at the smallest split distance, "
                                f"{first[2]['sse']}, exceeds {max_sse}")
            lo, hi, best = 0, m - 1, first
            while hi - lo > 1:
                mid = lo + (hi - lo) // 2
                p = probe(mid)
                if p[2]["sse"] <= max_sse:
                    lo, best = mid, p
                else:
                    hi = mid
        i, stream, err = best
        return stream, {"split_distance": float(cands[i]), "bytes": len(stream), "sse": err["sse"],
                        "channel_sse": err["channel_sse"], "pixels": err["pixels"], "psnr": err["psnr"],
                        "probes": made}

    def rate_quality(self, max_sse: int | None = None, min_psnr: float | None = None, contrast_bits: int = 5,
                     brightness_bits: int = 7, max_iter: int = -1, rms_eps: float = 1e-5) -> dict:
        """The quality rule: a candidate of the union whose container's summed RGB sse is within the target, by
        frac_quadtree_rate_quality's bisection with decode_error as the probe.  Exactly one of max_sse and min_psnr;
        min_psnr becomes max_sse = floor(255²·3·pixels / 10^(psnr/10)).  Returns a dict with split_distance, bytes,
        sse, channel_sse, pixels, psnr and probes.  The answer meets the target and the next larger candidate does
        not (unless it is the largest); the decoded error is not monotone in the split distance, so it need not be
        the largest candidate that meets it — rate_errors over rate_candidates answers that.  FracError when the
        smallest split distance fails."""
        return self._quality_fit(max_sse, min_psnr, contrast_bits, brightness_bits, max_iter, rms_eps)[1]

    def encode_quadtree_to_size(self, max_bytes: int, max_size: int = 16, min_size: int = 4, contrast_bits: int = 5,
                                brightness_bits: int = 7):
        """After load(): the FRC3 container of the least split distance at which it has at most max_bytes (the size
        rule): quadtree_rate + rate_fit + rate_stream.  Returns (container, info): info has split_distance, bytes,
        plane_bytes and stats ([summed stats dict] of the three full-tree searches)."""
        stats = self.quadtree_rate(max_size, min_size)
        t, size, planes = self.rate_fit(max_bytes, contrast_bits, brightness_bits)
        stream = self.rate_stream(t, contrast_bits, brightness_bits)
        return stream, {"split_distance": t, "bytes": size, "plane_bytes": planes, "stats": stats}

    def encode_quadtree_to_psnr(self, min_psnr: float, max_size: int = 16, min_size: int = 4,
                                contrast_bits: int = 5, brightness_bits: int = 7, max_iter: int = -1,
                                rms_eps: float = 1e-5):
        """After load(): an FRC3 container whose decoded RGB PSNR against the loaded frame is at least min_psnr (the
        quality rule): quadtree_rate + rate_quality.  Returns (container, info): rate_quality's dict plus stats."""
        stats = self.quadtree_rate(max_size, min_size)
        stream, info = self._quality_fit(None, min_psnr, contrast_bits, brightness_bits, max_iter, rms_eps)
        info["stats"] = stats
        return stream, info

    def host_planes(self):
        return [p.cpu().numpy() for p in self.planes]


def encode_color(rgb, **kw):
    """Convert + encode one RGB frame; returns ([Y, U, V] host planes, [(items, stats)] per plane)."""
    with ColorEncoder(**kw) as enc:
        enc.load(rgb)
        enc.run()
        enc.sync()
        return enc.host_planes(), enc.fetch()
