"""fractencode_amd — MI355X-native range×domain search for fractal block-matching.

Python binding of the C ABI in include/fracenc.h (libfracenc.so, built in-tree by
``__graft_entry__.build()``).  The product path is the HIP library; there is no
CPU fallback: constructing an :class:`Engine` without the library or without a
GPU raises.

The names mirror the reference's engine API for this path
(sebsgit/fractencode encode/EncodingEngine2.hpp, encode/TransformEstimator2.hpp):
  * :func:`create_uniform_grid`  — Frac2::createUniformGrid (image/partition2.hpp:109-135)
  * :func:`preclassify`          — BrightnessBlocksClassifier2::preclassify (Classifier2.cpp:64-68)
  * :class:`Engine`              — an AbstractEncodingEngine2 that encodes a whole batch
                                   of range items per call on one GPU
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# FRAC_LIB: an explicitly built alternative (tools/build_tuning.py's A/B library); the product is libfracenc.so.
# build_info() reports which library was loaded and whether it is a tuning build; bench.py refuses the
# headline with FRAC_LIB set.
PRODUCT_LIB = os.path.join(HERE, "libfracenc.so")
LIB_PATH = os.environ.get("FRAC_LIB") or PRODUCT_LIB

GRID_ITEM = np.dtype([("x", "<u4"), ("y", "<u4"), ("w", "<u4"), ("h", "<u4"), ("category", "<i4")])
ENCODE_ITEM = np.dtype([("x", "<u4"), ("y", "<u4"), ("w", "<u4"), ("h", "<u4"),
                        ("distance", "<f8"), ("contrast", "<f8"), ("brightness", "<f8"),
                        ("transform", "<i4"), ("_pad", "<i4"),
                        ("dx", "<u4"), ("dy", "<u4"), ("sw", "<u4"), ("sh", "<u4")])
# frac_tuple: (domain index, transform, s, o, rms) — the 32-byte record of the multi-GPU gather
TUPLE = np.dtype([("domain", "<u4"), ("transform", "<i4"), ("contrast", "<f8"), ("brightness", "<f8"),
                  ("distance", "<f8")])
# frac_run_timing: per-run device times (frac_timing_history)
RUN_TIMING = np.dtype([("ms_device", "<f8"), ("ms_prep", "<f8"), ("ms_search", "<f8"), ("ms_finish", "<f8")])
NO_DOMAIN = 0xFFFFFFFF
# frac_qt_leaf: a quadtree leaf in 32 bytes (frac_encode_quadtree_leaves, ABI 7)
QT_LEAF = np.dtype([("x", "<u2"), ("y", "<u2"), ("code", "<u4"), ("contrast", "<f8"), ("brightness", "<f8"),
                    ("distance", "<f8")])
QT_NO_DOMAIN = 0xFFFFFF
assert GRID_ITEM.itemsize == 20 and ENCODE_ITEM.itemsize == 64 and TUPLE.itemsize == 32 and QT_LEAF.itemsize == 32


def records_from_leaves(leaves: np.ndarray, width: int) -> np.ndarray:
    """encode_item_t records (ENCODE_ITEM) from 32-byte quadtree leaves (QT_LEAF) of a frame `width`
    pixels wide: the range at (x, y) of size n = 1 << (code >> 28), the winner domain `code & 0xffffff` of
    that level's grid createUniformGrid(W, H, 2n, n) (cols = (W − 2n)/n + 1), transform (code >> 24) & 15;
    QT_NO_DOMAIN is the reference's default record (domain (0, 0), size (0, 0))."""
    code = np.asarray(leaves["code"], np.uint32)
    n = (np.uint32(1) << (code >> np.uint32(28))).astype(np.uint32)
    d = (code & np.uint32(QT_NO_DOMAIN)).astype(np.int64)
    has = d != QT_NO_DOMAIN
    cols = np.where(width >= 2 * n, (np.int64(width) - 2 * n.astype(np.int64)) // n + 1, 1)
    rec = np.zeros(len(leaves), dtype=ENCODE_ITEM)
    rec["x"], rec["y"], rec["w"], rec["h"] = leaves["x"], leaves["y"], n, n
    for k in ("contrast", "brightness", "distance"):
        rec[k] = leaves[k]
    rec["transform"] = ((code >> np.uint32(24)) & np.uint32(15)).astype(np.int32)
    rec["dx"] = np.where(has, (d % cols) * n, 0)
    rec["dy"] = np.where(has, (d // cols) * n, 0)
    rec["sw"] = rec["sh"] = np.where(has, 2 * n, 0)
    return rec

ENGINE_AUTO, ENGINE_VALU, ENGINE_MFMA, ENGINE_SEA = 0, 1, 2, 3
FORM_DOT2, FORM_DIRECT, FORM_FOURIER, FORM_SEA, FORM_SEA_MFMA, FORM_SAMPLED = 0, 1, 2, 3, 4, 5
FORM_NAMES = {FORM_DOT2: "dot2", FORM_DIRECT: "direct", FORM_FOURIER: "fourier", FORM_SEA: "sea",
              FORM_SEA_MFMA: "sea_mfma", FORM_SAMPLED: "sampled"}
FLAG_TIMING = 1
# alternative exact forms (ABI 6; the product build refuses the old FRAC_MFMA_DFT / FRAC_SEA_TILED /
# FRAC_DECODE_UNFUSED environment knobs)
FLAG_DIRECT_FORM, FLAG_SEA_PER_RANGE, FLAG_DECODE_STEPWISE = 2, 4, 8
# ENGINE_AUTO's pruned route (n = 8, T = 4, ratio 2): never / whenever the geometry allows it
FLAG_EXHAUSTIVE, FLAG_PRUNE = 16, 32

# Frac::TransformType (image/transform.h:16-25)
TRANSFORM_NAMES = ("Id", "Rotate_90", "Rotate_180", "Rotate_270", "Flip", "Flip_Rotate_90", "Flip_Rotate_180",
                   "Flip_Rotate_270")


class FracParams(C.Structure):
    _fields_ = [("transforms", C.c_uint32), ("use_classifier", C.c_int32), ("rms_threshold", C.c_double),
                ("s_max", C.c_double), ("engine", C.c_uint32), ("flags", C.c_uint32)]


class FracStats(C.Structure):
    _fields_ = [("rejected_mappings", C.c_uint64), ("total_mappings", C.c_uint64), ("hit_ranges", C.c_uint32),
                ("fallback_ranges", C.c_uint32), ("empty_ranges", C.c_uint32), ("engine", C.c_uint32),
                ("ms_device", C.c_double), ("ms_search", C.c_double), ("ms_prep", C.c_double),
                ("ms_finish", C.c_double), ("search_form", C.c_uint32), ("pad_", C.c_uint32),
                ("matrix_flops", C.c_uint64), ("evaluated_mappings", C.c_uint64)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class FracQuadtreeParams(C.Structure):
    _fields_ = [("max_size", C.c_uint32), ("min_size", C.c_uint32), ("split_distance", C.c_double)]


class FracFrc1Info(C.Structure):
    """struct frac_frc1_info: an FRC1 header's fields, plus record_bits and body_bytes."""
    _fields_ = [(k, C.c_uint32) for k in ("width", "height", "range_size", "domain_size", "domain_stride",
                                         "transforms", "contrast_bits", "brightness_bits", "index_bits",
                                         "record_bits", "n_ranges", "n_domains", "flags")] + \
               [("body_bytes", C.c_uint64)] + \
               [(k, C.c_double) for k in ("contrast_min", "contrast_max", "brightness_min", "brightness_max")]


class FracFrq1Info(C.Structure):
    """struct frac_frq1_info: an FRQ1 header's fields, plus the per-level counts, widths and section offsets."""
    _fields_ = [(k, C.c_uint32) for k in ("width", "height", "max_size", "min_size", "transforms", "contrast_bits",
                                         "brightness_bits", "flags", "n_leaves", "levels")] + \
               [(k, C.c_uint32 * 4) for k in ("nodes", "leaves", "n_domains", "index_bits", "record_bits")] + \
               [(k, C.c_uint64 * 4) for k in ("bitmap_offset", "record_offset")] + \
               [("body_bytes", C.c_uint64)] + \
               [(k, C.c_double) for k in ("contrast_min", "contrast_max", "brightness_min", "brightness_max")]


class FracFrc3Info(C.Structure):
    """struct frac_frc3_info: an FRC3 container's header, plus each plane stream's kind and place."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("flags", C.c_uint32), ("kind", C.c_uint32 * 3),
                ("offset", C.c_uint64 * 3), ("length", C.c_uint64 * 3), ("total_bytes", C.c_uint64)]


KIND_FRC1, KIND_FRQ1 = 1, 2  # frac_frc3_info.kind


class FracError(RuntimeError):
    pass


_lib = None


# The product compile line (__graft_entry__.build): part of the source id, so a change of flags or
# of the ROCm toolchain rebuilds the library and re-keys the PMC measurements like a source change.
# -amdgpu-mfma-vgpr-form: MFMA accumulators in VGPRs (gfx950 has one unified register file), so the
# integer epilogue reads them without v_accvgpr_read copies.
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall",
               "-mllvm", "-amdgpu-mfma-vgpr-form"]
SOURCE_EXTS = (".hip", ".h", ".cuh")


def _rocm_version() -> str:
    try:
        with open("/opt/rocm/.info/version") as f:
            return f.read().strip()
    except OSError:
        return "unknown"


def source_id() -> str:
    """16 hex digits identifying the library's sources (the .hip / .h files of csrc/ and
    include/fracenc.h), its compile flags and the ROCm version: the key under which profiles/ records
    PMC measurements, so a measurement of another build is never reused."""
    import hashlib

    h = hashlib.sha256()
    csrc = os.path.join(HERE, "csrc")
    for name in sorted(os.listdir(csrc)):
        path = os.path.join(csrc, name)
        if not (os.path.isfile(path) and name.endswith(SOURCE_EXTS)):
            continue
        with open(path, "rb") as f:
            h.update(name.encode() + b"\0" + f.read())
    with open(os.path.join(os.path.dirname(HERE), "include", "fracenc.h"), "rb") as f:
        h.update(f.read())
    h.update(("\0".join(HIPCC_FLAGS) + "\0rocm " + _rocm_version()).encode())
    return h.hexdigest()[:16]


def lib() -> C.CDLL:
    """The HIP engine library; raises FracError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FracError(f"{LIB_PATH} not built: run __graft_entry__.build() (no CPU fallback exists)")
        # One HIP runtime per process: PyTorch bundles its own libamdhip64 (soname libamdhip64.so.7,
        # file name libamdhip64.so).  Loaded first, it also serves this library (same soname), so
        # torch streams and device tensors are valid here; loaded second, torch would open a second
        # runtime that finds no device.  Import torch (when installed) before the library.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if LIB_PATH != PRODUCT_LIB:
            import warnings

            warnings.warn(f"fractencode_amd: FRAC_LIB loads {LIB_PATH}, not the product library", stacklevel=2)
        L = C.CDLL(LIB_PATH)
        vp, u32, i32, sz = C.c_void_p, C.c_uint32, C.c_int, C.c_size_t
        sig = {
            "frac_abi_version": (i32, []),
            "frac_device_count": (i32, []),
            "frac_build_id": (C.c_char_p, []),
            "frac_build_flags": (i32, []),
            "frac_create": (vp, [i32, C.POINTER(FracParams)]),
            "frac_destroy": (None, [vp]),
            "frac_last_error": (C.c_char_p, [vp]),
            "frac_set_params": (i32, [vp, C.POINTER(FracParams)]),
            "frac_set_frame": (i32, [vp, vp, u32, u32, u32]),
            "frac_set_planes": (i32, [vp, vp, u32, u32, u32, vp, u32, u32, u32]),
            "frac_set_frame_device": (i32, [vp, vp, u32, u32, u32]),
            "frac_set_frame_device_async": (i32, [vp, vp, u32, u32, u32]),
            "frac_set_frame_async": (i32, [vp, vp, u32, u32, u32]),
            "frac_set_domains": (i32, [vp, vp, sz]),
            "frac_set_ranges": (i32, [vp, vp, sz]),
            "frac_run": (i32, [vp]),
            "frac_fetch": (i32, [vp, vp, C.POINTER(FracStats)]),
            "frac_sync": (i32, [vp]),
            "frac_timing_history": (i32, [vp, vp, sz, C.POINTER(C.c_size_t)]),
            "frac_search": (i32, [vp, vp, sz, vp, C.POINTER(FracStats)]),
            "frac_set_stream": (i32, [vp, vp]),
            "frac_get_stream": (vp, [vp]),
            "frac_device_results": (vp, [vp]),
            "frac_copy_results_device": (i32, [vp, vp]),
            "frac_copy_tuples_device": (i32, [vp, vp]),
            "frac_set_tuple_sink": (i32, [vp, vp]),
            "frac_pack_frc1": (i32, [vp, u32, u32, vp, sz, C.POINTER(C.c_size_t)]),
            "frac_frc1_info": (i32, [vp, sz, C.POINTER(FracFrc1Info)]),
            "frac_decode_frc1": (i32, [vp, vp, sz, u32, i32, C.c_double, vp, sz, C.POINTER(C.c_int),
                                       C.POINTER(C.c_double)]),
            "frac_frq1_info": (i32, [vp, sz, C.POINTER(FracFrq1Info)]),
            "frac_pack_frq1": (i32, [vp, sz, u32, u32, u32, u32, u32, u32, u32, u32, vp, sz, C.POINTER(C.c_size_t)]),
            "frac_decode_frq1": (i32, [vp, vp, sz, u32, i32, C.c_double, vp, sz, C.POINTER(C.c_int),
                                       C.POINTER(C.c_double)]),
            "frac_fetch_tuples": (i32, [vp, vp]),
            "frac_decode": (i32, [vp, vp, sz, u32, u32, i32, C.c_double, vp, C.POINTER(C.c_int),
                                  C.POINTER(C.c_double)]),
            "frac_decode_results": (i32, [vp, u32, u32, i32, C.c_double, vp, C.POINTER(C.c_int),
                                          C.POINTER(C.c_double)]),
            "frac_classify_items": (i32, [vp, vp, sz, i32]),
            "frac_encode_quadtree": (i32, [vp, C.POINTER(FracQuadtreeParams), vp, sz, C.POINTER(sz),
                                           C.POINTER(FracStats)]),
            "frac_encode_quadtree_leaves": (i32, [vp, C.POINTER(FracQuadtreeParams), vp, sz, C.POINTER(sz),
                                                  C.POINTER(FracStats)]),
            "frac_quadtree_rate_build": (i32, [vp, u32, u32, C.POINTER(FracStats)]),
            "frac_quadtree_rate_sizes": (i32, [vp, u32, u32, vp, sz, vp, vp, vp]),
            "frac_quadtree_rate_fit": (i32, [vp, u32, u32, C.c_uint64, C.POINTER(C.c_double),
                                             C.POINTER(C.c_uint64), C.POINTER(u32)]),
            "frac_quadtree_rate_leaves": (i32, [vp, C.c_double, vp, sz, C.POINTER(sz)]),
            "frac_frq1_size": (i32, [u32, u32, u32, u32, u32, u32, u32, C.POINTER(u32), C.POINTER(C.c_uint64)]),
            "frac_quadtree_rate_stream": (i32, [vp, C.c_double, u32, u32, vp, sz, C.POINTER(sz)]),
            "frac_encode_quadtree_stream": (i32, [vp, C.POINTER(FracQuadtreeParams), u32, u32, vp, sz,
                                                  C.POINTER(sz), C.POINTER(FracStats)]),
            "frac_quadtree_rd_sizes": (i32, [vp, u32, u32, vp, sz, vp, vp, vp, vp]),
            "frac_quadtree_rd_fit": (i32, [vp, u32, u32, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                           C.POINTER(u32), C.POINTER(C.c_uint64)]),
            "frac_quadtree_rd_leaves": (i32, [vp, u32, u32, C.c_uint64, vp, sz, C.POINTER(sz)]),
            "frac_quadtree_rd_stream": (i32, [vp, C.c_uint64, u32, u32, vp, sz, C.POINTER(sz)]),
            "frac_decode_error": (i32, [vp, vp, sz, i32, C.c_double, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), vp,
                                        sz, C.POINTER(sz), C.POINTER(C.c_int), C.POINTER(C.c_double)]),
            "frac_quadtree_rate_errors": (i32, [vp, u32, u32, vp, sz, i32, C.c_double, vp, vp, vp]),
            "frac_quadtree_rate_quality": (i32, [vp, u32, u32, C.c_uint64, i32, C.c_double, C.POINTER(C.c_double),
                                                 C.POINTER(C.c_uint64), C.POINTER(u32), C.POINTER(C.c_uint64),
                                                 C.POINTER(u32)]),
            "frac_rgb_to_yuv_device": (i32, [vp, vp, u32, u32, u32, vp, u32, vp, u32, vp, u32]),
            "frac_rgb_to_yuv": (i32, [vp, vp, u32, u32, u32, vp, vp, vp]),
            "frac_yuv_to_rgb_device": (i32, [vp, vp, u32, u32, u32, vp, u32, vp, u32, vp, u32]),
            "frac_yuv_to_rgb": (i32, [vp, vp, vp, vp, u32, u32, vp, u32]),
            "frac_frc3_info": (i32, [vp, sz, C.POINTER(FracFrc3Info)]),
            "frac_pack_frc3": (i32, [C.POINTER(vp), C.POINTER(sz), u32, u32, vp, sz, C.POINTER(C.c_size_t)]),
            "frac_decode_frc3": (i32, [vp, vp, sz, u32, i32, C.c_double, vp, u32, sz, C.POINTER(C.c_int),
                                       C.POINTER(C.c_double)]),
            "frac_decode_frc3_device": (i32, [vp, vp, sz, u32, i32, C.c_double, vp, u32, sz, C.POINTER(C.c_int),
                                              C.POINTER(C.c_double)]),
            "frac_decode_error_frc3": (i32, [vp, vp, sz, vp, u32, i32, C.c_double, C.POINTER(C.c_uint64),
                                             C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_double)]),
            "frac_decode_error_frc3_device": (i32, [vp, vp, sz, vp, u32, i32, C.c_double, C.POINTER(C.c_uint64),
                                                    C.POINTER(C.c_uint64), C.POINTER(C.c_int),
                                                    C.POINTER(C.c_double)]),
            "frac_quadtree_rate_candidates": (i32, [vp, vp, sz, C.POINTER(sz)]),
            "frac_decode_inter": (i32, [vp, vp, sz, u32, vp, vp, sz]),
            "frac_decode_inter_device": (i32, [vp, vp, sz, u32, vp, u32, vp, u32, sz]),
            "frac_inter_error": (i32, [vp, vp, sz, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
            "frac_set_planes_device": (i32, [vp, vp, u32, u32, u32, vp, u32, u32, u32]),
            "frac_uniform_grid": (sz, [u32, u32, u32, u32, vp, sz]),
            "frac_uniform_grid2": (sz, [u32, u32, u32, u32, u32, u32, vp, sz]),
            "frac_classify": (i32, [vp, u32, u32, u32, vp, sz]),
            "frac_transform_index": (i32, [u32, u32, u32]),
            "frac_hit_limit": (C.c_int64, [C.c_double, u32]),
            "frac_debug_sort_chunk": (u32, []),
            "frac_debug_resolve_group": (u32, []),
            "frac_debug_sort_pairs": (i32, [vp, vp, u32, vp, vp, u32, u32, vp, vp, vp, vp]),
            "frac_debug_bucket_tile": (u32, []),
            "frac_debug_bucket_self_tiles": (u32, []),
            "frac_debug_bucket_keys": (i32, [vp, vp, u32, vp, u32, i32, vp, vp]),
            "frac_debug_bucket_sort": (i32, [vp, u32, u32, vp, u32, u32, vp, vp, vp, vp]),
            "frac_debug_frame_twin_bytes": (C.c_uint64, [vp]),
            "frac_debug_frame_copy_stream": (i32, [vp]),
        }
        for name, (res, args) in sig.items():
            if os.environ.get("FRAC_LIB") and not hasattr(L, name):
                continue  # an A/B library built from older sources lacks the newer entry points
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


BUILD_TUNING = 1


def build_info() -> dict:
    """The loaded library: its path, the source id compiled into it (frac_build_id), whether it is
    a -DFRAC_TUNING build, and whether that id is the id of the sources next to it."""
    L = lib()
    bid = L.frac_build_id().decode()
    return {"lib": os.path.relpath(LIB_PATH, os.path.dirname(HERE)), "build_id": bid,
            "tuning": bool(L.frac_build_flags() & BUILD_TUNING), "matches_sources": bid == source_id()}


def last_error(ctx=None) -> str:
    msg = lib().frac_last_error(ctx)
    return msg.decode() if msg else ""


# ---- test hooks (outside the ABI contract) ------------------------------------------

TP_SORT_CHUNK = 2048  # items per workgroup of the tiled SEA form's sort (frac_debug_sort_chunk)


def debug_sort_pairs(keys, vals, keys_b, vals_b, bits: int):
    """Test hook: the tiled SEA form's stable sort of (key, value) uint32 pairs on the current device, two
    sides through the same launches (either may be empty), on the low `bits` key bits.  Returns
    (keys, vals, keys_b, vals_b) sorted, equal keys in input order."""
    L = lib()
    if L.frac_debug_sort_chunk() != TP_SORT_CHUNK:
        raise FracError("TP_SORT_CHUNK differs from the library's frac_debug_sort_chunk()")
    ins = [np.ascontiguousarray(a, dtype=np.uint32) for a in (keys, vals, keys_b, vals_b)]
    if ins[0].shape != ins[1].shape or ins[2].shape != ins[3].shape or ins[0].ndim != 1 or ins[2].ndim != 1:
        raise ValueError("keys and values must be one-dimensional and of equal length per side")
    outs = [np.empty_like(a) for a in ins]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None  # noqa: E731
    rc = L.frac_debug_sort_pairs(ptr(ins[0]), ptr(ins[1]), ins[0].size, ptr(ins[2]), ptr(ins[3]), ins[2].size,
                                 bits, *[ptr(a) for a in outs])
    if rc != 0:
        raise FracError(f"frac_debug_sort_pairs: {last_error()} (code {rc})")
    return tuple(outs)


def debug_frame_upload(engine) -> dict:
    """What the engine's context holds for overlapped frame uploads: twin_bytes, the capacity of its second
    plane buffers (frac_debug_frame_twin_bytes), and copy_stream, whether its copy stream exists
    (frac_debug_frame_copy_stream)."""
    L = lib()
    return {"twin_bytes": int(L.frac_debug_frame_twin_bytes(engine._ctx)),
            "copy_stream": bool(L.frac_debug_frame_copy_stream(engine._ctx))}


BK_TILE = 1024        # items per workgroup of the classifier bucket sort (frac_debug_bucket_tile)
BK_SELF_TILES = 512   # the most tiles of a sort without the scan launch (frac_debug_bucket_self_tiles)
BK_KEYS = 8           # keys 0..7: categories -1..5 and the padding key
KEYS_AUTO, KEYS_ROWS, KEYS_PAIR, KEYS_BLOCK_SUMS = 0, 1, 2, 3  # frac_debug_bucket_keys' path


def debug_bucket_keys(engine, doms, rngs, path: int = KEYS_AUTO):
    """Test hook: the classifier bucket keys (category + 1) of two GRID_ITEM arrays by the key kernels a
    classified run uses, the domains on the engine's source plane and the ranges on its target plane.  path:
    KEYS_AUTO the run's own choice, KEYS_ROWS the row kernels grid by grid, KEYS_PAIR the paired launch,
    KEYS_BLOCK_SUMS the planes' block sums.  Returns (dom_keys, rng_keys); FracError where the hook refuses."""
    doms = np.ascontiguousarray(doms, dtype=GRID_ITEM)
    rngs = np.ascontiguousarray(rngs, dtype=GRID_ITEM)
    kd, kr = np.full(len(doms), 0xFFFFFFFF, np.uint32), np.full(len(rngs), 0xFFFFFFFF, np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None  # noqa: E731
    rc = lib().frac_debug_bucket_keys(engine._ctx, ptr(doms), len(doms), ptr(rngs), len(rngs), path, ptr(kd), ptr(kr))
    if rc != 0:
        raise FracError(f"frac_debug_bucket_keys: {last_error(engine._ctx)} (code {rc})")
    return kd, kr


def debug_bucket_sort(keys_a, keys_b, dn_a: int | None = None, dn_b: int | None = None):
    """Test hook: the stable bucket sort of two uint32 key arrays (keys 0..7, either may be empty) through the
    same launches.  dn_*: a count the kernels read on the device (the first min(dn, n) keys are sorted), None
    for none.  Returns (order_a, first_a, order_b, first_b): the sorted indices, 0xffffffff where the sort
    wrote nothing, and the BK_KEYS + 1 bucket starts."""
    L = lib()
    if L.frac_debug_bucket_tile() != BK_TILE or L.frac_debug_bucket_self_tiles() != BK_SELF_TILES:
        raise FracError("BK_TILE / BK_SELF_TILES differ from the library's")
    ka, kb = (np.ascontiguousarray(a, dtype=np.uint32) for a in (keys_a, keys_b))
    if ka.ndim != 1 or kb.ndim != 1:
        raise ValueError("keys must be one-dimensional")
    oa, ob = np.zeros(ka.size, np.uint32), np.zeros(kb.size, np.uint32)
    fa, fb = np.zeros(BK_KEYS + 1, np.uint32), np.zeros(BK_KEYS + 1, np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None  # noqa: E731
    none = 0xFFFFFFFF
    rc = L.frac_debug_bucket_sort(ptr(ka), ka.size, none if dn_a is None else dn_a, ptr(kb), kb.size,
                                  none if dn_b is None else dn_b, ptr(oa), ptr(fa), ptr(ob), ptr(fb))
    if rc != 0:
        raise FracError(f"frac_debug_bucket_sort: {last_error()} (code {rc})")
    return oa, fa, ob, fb


# ---- host helpers ----------------------------------------------------------------

def create_uniform_grid(width: int, height: int, item_size, item_offset) -> np.ndarray:
    """Frac2::createUniformGrid (image/partition2.hpp:109-135): row-major items, x fastest
    (categories -1).  item_size / item_offset: an int, or (x, y) like the reference's Size32u."""
    sw, sh = (item_size, item_size) if np.isscalar(item_size) else item_size
    ox, oy = (item_offset, item_offset) if np.isscalar(item_offset) else item_offset
    n = lib().frac_uniform_grid2(width, height, sw, sh, ox, oy, None, 0)
    out = np.zeros(n, dtype=GRID_ITEM)
    if n:
        lib().frac_uniform_grid2(width, height, sw, sh, ox, oy, out.ctypes.data, n)
    return out


def preclassify(plane: np.ndarray, items: np.ndarray) -> np.ndarray:
    """Categories of BrightnessBlocksClassifier2 computed on `plane` (returns a copy)."""
    plane = np.ascontiguousarray(plane, dtype=np.uint8)
    items = np.ascontiguousarray(items, dtype=GRID_ITEM).copy()
    rc = lib().frac_classify(plane.ctypes.data, plane.shape[1], plane.shape[0], plane.shape[1], items.ctypes.data,
                             len(items))
    if rc != 0:
        raise FracError(last_error())
    return items


def frc1_info(stream) -> dict:
    """An FRC1 stream's header, validated against the stream's length on the host (frac_frc1_info): the
    keys of codec.read_header without magic and version, plus record_bits and body_bytes.  Raises
    FracError on a stream frac_decode_frc1 would refuse by its header."""
    buf = np.frombuffer(stream, dtype=np.uint8)
    out = FracFrc1Info()
    if lib().frac_frc1_info(buf.ctypes.data if len(buf) else None, len(buf), C.byref(out)) != 0:
        raise FracError(last_error())
    return {k: getattr(out, k) for k, _ in FracFrc1Info._fields_}


def frq1_info(stream) -> dict:
    """An FRQ1 stream's header and layout, validated against the stream's length on the host
    (frac_frq1_info): the keys of codec.unpack_quadtree_stream's header dict without magic and version.
    Raises FracError on a stream frac_decode_frq1 would refuse by its header or sections."""
    buf = np.frombuffer(stream, dtype=np.uint8)
    out = FracFrq1Info()
    if lib().frac_frq1_info(buf.ctypes.data if len(buf) else None, len(buf), C.byref(out)) != 0:
        raise FracError(last_error())
    return {k: (list(getattr(out, k)) if hasattr(getattr(out, k), "__len__") else getattr(out, k))
            for k, _ in FracFrq1Info._fields_}


def pack_frq1(leaves: np.ndarray, width: int, height: int, max_size: int, min_size: int, transforms: int = 4,
              use_classifier: bool = False, contrast_bits: int = 5, brightness_bits: int = 7) -> bytes:
    """QT_LEAF leaves (encode_quadtree(leaves=True), its order) of a width×height frame as an FRQ1 stream
    (codec.py layout), quantized and packed on the host in one pass (frac_pack_frq1)."""
    leaves = np.ascontiguousarray(leaves, dtype=QT_LEAF)
    args = (leaves.ctypes.data if len(leaves) else None, len(leaves), width, height, max_size, min_size, transforms,
            1 if use_classifier else 0, contrast_bits, brightness_bits)
    n = C.c_size_t(0)
    if lib().frac_pack_frq1(*args, None, 0, C.byref(n)) != 0:
        raise FracError(last_error())
    buf = np.empty(n.value, dtype=np.uint8)
    if lib().frac_pack_frq1(*args, buf.ctypes.data_as(C.c_void_p), n.value, C.byref(n)) != 0:
        raise FracError(last_error())
    return buf.tobytes()


def frq1_size(width: int, height: int, max_size: int, min_size: int, splits, transforms: int = 4,
              contrast_bits: int = 5, brightness_bits: int = 7) -> int:
    """The size in bytes of the FRQ1 stream of a partition of a width×height frame that splits splits[k] nodes
    of level k (sides max_size >> k; one count per level but the last), on the host (frac_frq1_size): the header,
    per level a bitmap over its nodes (all but the last) and its leaves' records, each padded to a dword."""
    s = (C.c_uint32 * 3)(*([int(v) for v in splits] + [0, 0, 0])[:3])
    n = C.c_uint64(0)
    if lib().frac_frq1_size(width, height, max_size, min_size, transforms, contrast_bits, brightness_bits, s,
                            C.byref(n)) != 0:
        raise FracError(last_error())
    return n.value


def frc3_info(stream) -> dict:
    """An FRC3 colour container's header and plane streams, validated on the host (frac_frc3_info): width,
    height, flags, per plane kind (KIND_FRC1 / KIND_FRQ1), offset and length, and total_bytes — the keys of
    codec.unpack_color_stream's header dict.  Raises FracError on a container frac_decode_frc3 would refuse by
    its header or by a plane stream's."""
    buf = np.frombuffer(stream, dtype=np.uint8)
    out = FracFrc3Info()
    if lib().frac_frc3_info(buf.ctypes.data if len(buf) else None, len(buf), C.byref(out)) != 0:
        raise FracError(last_error())
    return {k: (list(getattr(out, k)) if hasattr(getattr(out, k), "__len__") else getattr(out, k))
            for k, _ in FracFrc3Info._fields_}


def pack_frc3(streams, width: int, height: int) -> bytes:
    """The Y, U and V plane streams (FRC1 or FRQ1, kinds may be mixed) of a width × height RGB frame as one FRC3
    container (codec.py layout; frac_pack_frc3)."""
    if len(streams) != 3:
        raise FracError("pack_frc3: three plane streams (Y, U, V)")
    bufs = [np.frombuffer(s, dtype=np.uint8) for s in streams]
    ptrs = (C.c_void_p * 3)(*[b.ctypes.data if len(b) else None for b in bufs])
    lens = (C.c_size_t * 3)(*[len(b) for b in bufs])
    n = C.c_size_t(0)
    if lib().frac_pack_frc3(ptrs, lens, width, height, None, 0, C.byref(n)) != 0:
        raise FracError(last_error())
    out = np.empty(n.value, dtype=np.uint8)
    if lib().frac_pack_frc3(ptrs, lens, width, height, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)) != 0:
        raise FracError(last_error())
    return out.tobytes()


def _device_rows(t, width_bytes: int, what: str) -> int:
    """The row stride in bytes of a CUDA uint8 tensor whose rows hold width_bytes contiguous bytes; FracError for
    a negative or too small one (ctypes would wrap it into a huge uint32)."""
    stride = int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), width_bytes)
    if stride < width_bytes or stride > 0xFFFFFFFF:
        raise FracError(f"{what}: row stride {t.stride(0)} is negative or below the row's {width_bytes} bytes")
    return stride


def _stream_frame(stream) -> tuple[int, int]:
    """(width, height) of an FRC1 or FRQ1 stream, told apart by its magic (frac_frc1_info / frac_frq1_info)."""
    h = frq1_info(stream) if bytes(memoryview(stream)[:4]) == b"FRQ1" else frc1_info(stream)
    return h["width"], h["height"]


def transform_index(n: int, t: int, pix: int) -> int:
    return lib().frac_transform_index(n, t, pix)


def hit_limit(rms_threshold: float, n: int) -> int:
    return lib().frac_hit_limit(rms_threshold, n)


# ---- engine ---------------------------------------------------------------------

def _psnr(sse: int, pixels: int) -> float:
    """10·log10(255²·pixels / sse); inf at sse == 0."""
    return math.inf if sse == 0 else 10.0 * math.log10(255.0 ** 2 * pixels / sse)


class Engine:
    """One search context on one GPU (an AbstractEncodingEngine2 that takes batches).

    Parameters mirror encode_parameters_t / TransformMatcher: ``transforms`` 4 (the
    reference's TransformMatcher::match) or 8, ``use_classifier``, ``rms_threshold``,
    ``s_max``.
    """

    def __init__(self, device: int = 0, transforms: int = 4, use_classifier: bool = False,
                 rms_threshold: float = 0.0, s_max: float = -1.0, engine: int = ENGINE_AUTO, timing: bool = False,
                 flags: int = 0):
        """flags: FLAG_DIRECT_FORM / FLAG_SEA_PER_RANGE / FLAG_DECODE_STEPWISE select an alternative
        exact form (the same records from other kernels: cross-checks); FLAG_EXHAUSTIVE / FLAG_PRUNE keep
        ENGINE_AUTO off / put it on its pruned route (n = 8, T = 4) whatever the run's size."""
        self._p = FracParams(transforms, int(use_classifier), rms_threshold, s_max, engine,
                             (FLAG_TIMING if timing else 0) | flags)
        self._ctx = lib().frac_create(device, C.byref(self._p))
        if not self._ctx:
            raise FracError("frac_create failed: " + last_error())
        self._nr = 0
        self._keep = []
        self._frame_wh = (0, 0)

    def close(self) -> None:
        if getattr(self, "_ctx", None):
            lib().frac_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise FracError(f"rc={rc}: {last_error(self._ctx)}")

    def set_params(self, transforms=None, use_classifier=None, rms_threshold=None, s_max=None, engine=None,
                   flags=None):
        """Change the given parameters of a prepared context (frac_set_params); the next run() re-prepares.  Like
        every setter it ends the last run's results: until the next run() the readers raise FracError."""
        if transforms is not None:
            self._p.transforms = transforms
        if use_classifier is not None:
            self._p.use_classifier = int(use_classifier)
        if rms_threshold is not None:
            self._p.rms_threshold = rms_threshold
        if s_max is not None:
            self._p.s_max = s_max
        if engine is not None:
            self._p.engine = engine
        if flags is not None:
            self._p.flags = (self._p.flags & FLAG_TIMING) | flags
        self._check(lib().frac_set_params(self._ctx, C.byref(self._p)))

    def set_frame(self, plane) -> None:
        """Source == target plane (Encoder2).  numpy uint8 [H, W] or a CUDA torch tensor.  A host plane has been
        consumed when the call returns; after a frame of the same size its upload overlaps what is left of the
        previous run() (frac_set_frame)."""
        self._frame_wh = (int(plane.shape[1]), int(plane.shape[0]))
        if hasattr(plane, "is_cuda") and plane.is_cuda:
            import torch

            if plane.dtype != torch.uint8 or plane.dim() != 2:
                raise FracError("set_frame: a device plane must be a 2-D uint8 tensor")
            if plane.stride(1) != 1 or plane.stride(0) < plane.shape[1]:
                raise FracError("set_frame: device plane rows must be contiguous (stride(1) == 1, "
                                "stride(0) >= width)")
            # the library copies on its own stream: work still pending on torch's current stream
            # (e.g. the kernel producing this plane) must land first
            torch.cuda.current_stream(plane.device).synchronize()
            self._check(lib().frac_set_frame_device(self._ctx, C.c_void_p(plane.data_ptr()), plane.shape[1],
                                                    plane.shape[0], plane.stride(0)))
            return
        plane = np.ascontiguousarray(plane, dtype=np.uint8)
        self._check(lib().frac_set_frame(self._ctx, plane.ctypes.data, plane.shape[1], plane.shape[0],
                                         plane.shape[1]))

    def set_frame_device_async(self, plane) -> None:
        """ABI 9: a CUDA uint8 [H, W] plane copied on this engine's stream without waiting (frame streaming).
        The caller orders the plane's producer before this engine's stream (e.g. an event the stream waits on)
        and keeps the plane unchanged until the stream has passed the copy."""
        if not (hasattr(plane, "is_cuda") and plane.is_cuda) or plane.dim() != 2 or plane.stride(1) != 1:
            raise FracError("set_frame_device_async: a 2-D CUDA uint8 plane with contiguous rows")
        self._frame_wh = (int(plane.shape[1]), int(plane.shape[0]))
        self._check(lib().frac_set_frame_device_async(self._ctx, C.c_void_p(plane.data_ptr()), plane.shape[1],
                                                      plane.shape[0], plane.stride(0)))

    def set_frame_async(self, plane) -> None:
        """ABI 9: frame streaming from host memory — a uint8 [H, W] plane (a pinned torch tensor or a numpy view
        of one, for an asynchronous copy) uploaded on the context's copy stream while the runs already enqueued
        search the previous frame; the next run() searches this one.  The plane must stay unchanged until the
        upload is done (a later sync() / fetch(), or an event on this engine's stream)."""
        if hasattr(plane, "is_cuda"):
            if plane.is_cuda:
                raise FracError("set_frame_async: a host plane (set_frame_device_async takes device planes)")
            plane = plane.numpy()
        if plane.dtype != np.uint8 or plane.ndim != 2 or plane.strides[1] != 1:
            raise FracError("set_frame_async: a 2-D uint8 host plane with contiguous rows")
        self._frame_wh = (int(plane.shape[1]), int(plane.shape[0]))
        self._keep_async = plane  # the memory stays referenced while the upload may run
        self._check(lib().frac_set_frame_async(self._ctx, C.c_void_p(plane.ctypes.data), plane.shape[1],
                                               plane.shape[0], plane.strides[0]))

    def set_planes(self, source, target) -> None:
        """Domains on `source`, ranges on `target` (frac_set_planes): two numpy uint8 [H, W] planes, or two CUDA
        uint8 tensors (rows may be strided), copied device to device (frac_set_planes_device)."""
        if any(hasattr(p, "is_cuda") and p.is_cuda for p in (source, target)):
            import torch

            for p in (source, target):
                if not (hasattr(p, "is_cuda") and p.is_cuda) or p.dtype != torch.uint8 or p.dim() != 2:
                    raise FracError("set_planes: device planes must both be 2-D CUDA uint8 tensors")
                if p.stride(1) != 1 and p.shape[1] > 1:
                    raise FracError("set_planes: device plane rows must be contiguous (stride(1) == 1)")
            ss = _device_rows(source, int(source.shape[1]), "set_planes")
            ts = _device_rows(target, int(target.shape[1]), "set_planes")
            # the library copies on its own stream: work still pending on torch's current stream lands first
            torch.cuda.current_stream(source.device).synchronize()
            self._check(lib().frac_set_planes_device(self._ctx, C.c_void_p(source.data_ptr()), source.shape[1],
                                                     source.shape[0], ss, C.c_void_p(target.data_ptr()),
                                                     target.shape[1], target.shape[0], ts))
            self._frame_wh = (int(source.shape[1]), int(source.shape[0]))  # a refused call leaves it as it was
            return
        self._frame_wh = (int(source.shape[1]), int(source.shape[0]))
        s = np.ascontiguousarray(source, dtype=np.uint8)
        t = np.ascontiguousarray(target, dtype=np.uint8)
        self._check(lib().frac_set_planes(self._ctx, s.ctypes.data, s.shape[1], s.shape[0], s.shape[1], t.ctypes.data,
                                          t.shape[1], t.shape[0], t.shape[1]))

    def set_domains(self, items: np.ndarray) -> None:
        items = np.ascontiguousarray(items, dtype=GRID_ITEM)
        self._check(lib().frac_set_domains(self._ctx, items.ctypes.data if len(items) else None, len(items)))

    def set_ranges(self, items: np.ndarray) -> None:
        items = np.ascontiguousarray(items, dtype=GRID_ITEM)
        self._check(lib().frac_set_ranges(self._ctx, items.ctypes.data if len(items) else None, len(items)))
        self._nr = len(items)

    def run(self) -> None:
        self._check(lib().frac_run(self._ctx))

    def sync(self) -> None:
        self._check(lib().frac_sync(self._ctx))

    def fetch(self):
        out = np.zeros(self._nr, dtype=ENCODE_ITEM)
        st = FracStats()
        self._check(lib().frac_fetch(self._ctx, out.ctypes.data if self._nr else None, C.byref(st)))
        return out, st.as_dict()

    def timing_history(self) -> np.ndarray:
        """Device times (ms: device, prep, search, finish) of every run since the previous call
        (engine created with timing=True); waits for the stream."""
        n = C.c_size_t(0)
        self._check(lib().frac_timing_history(self._ctx, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=RUN_TIMING)
        self._check(lib().frac_timing_history(self._ctx, out.ctypes.data if n.value else None, n.value, C.byref(n)))
        return out[: n.value]

    def search(self, ranges: np.ndarray):
        """set_ranges + run + fetch → (encode items in range order, stats dict)."""
        self.set_ranges(ranges)
        self.run()
        return self.fetch()

    def set_stream(self, stream_handle: int | None) -> None:
        self._check(lib().frac_set_stream(self._ctx, C.c_void_p(stream_handle) if stream_handle else None))

    def stream_handle(self) -> int:
        """The hipStream_t this context enqueues on (frac_get_stream), as an integer."""
        return lib().frac_get_stream(self._ctx) or 0

    def copy_results_device(self, dst_ptr: int) -> None:
        """Async D2D copy of the last run's results (64 B each) to a device buffer."""
        self._check(lib().frac_copy_results_device(self._ctx, C.c_void_p(dst_ptr)))

    def copy_tuples_device(self, dst_ptr: int) -> None:
        """Async pack of the last run's 32-byte (domain, transform, s, o, rms) tuples into a device buffer."""
        self._check(lib().frac_copy_tuples_device(self._ctx, C.c_void_p(dst_ptr)))

    def set_tuple_sink(self, dst_ptr: int | None) -> None:
        """Every later run also writes its 32-byte tuples to dst_ptr (device memory, or pinned host memory
        the device can write: they then cross PCIe while the resolve writes them); None clears it (ABI 8)."""
        self._check(lib().frac_set_tuple_sink(self._ctx, C.c_void_p(dst_ptr) if dst_ptr else None))

    def pack_frc1(self, contrast_bits: int = 5, brightness_bits: int = 7) -> bytes:
        """The last run's results as an FRC1 stream (codec.py layout), quantized and packed on the
        device (frac_pack_frc1)."""
        n = C.c_size_t(0)
        self._check(lib().frac_pack_frc1(self._ctx, contrast_bits, brightness_bits, None, 0, C.byref(n)))
        buf = np.empty(n.value, dtype=np.uint8)
        self._check(lib().frac_pack_frc1(self._ctx, contrast_bits, brightness_bits, buf.ctypes.data_as(C.c_void_p),
                                         n.value, C.byref(n)))
        return buf.tobytes()

    def fetch_tuples(self, out: np.ndarray | None = None) -> np.ndarray:
        """The last run's tuples (TUPLE records) on the host; `out` (TUPLE array of the range count,
        e.g. a view of pinned memory) is filled in place when given."""
        n = self._nr
        if out is None:
            out = np.zeros(n, dtype=TUPLE)
        elif out.dtype != TUPLE or len(out) != n or not out.flags.c_contiguous:
            raise FracError("fetch_tuples: out must be a contiguous TUPLE array of the range count")
        if n:
            self._check(lib().frac_fetch_tuples(self._ctx, out.ctypes.data_as(C.c_void_p)))
        return out

    def decode(self, items: np.ndarray | None, width: int, height: int, max_iter: int = -1, rms_eps: float = 1e-5,
               initial: np.ndarray | None = None):
        """Decoder2::decode on the GPU. items=None decodes the last run's results on the device.
        Returns (plane, iterations, rms)."""
        plane = np.zeros((height, width), np.uint8) if initial is None else np.ascontiguousarray(initial, np.uint8).copy()
        it = C.c_int()
        rms = C.c_double()
        if items is None:
            self._check(lib().frac_decode_results(self._ctx, width, height, max_iter, rms_eps, plane.ctypes.data,
                                                  C.byref(it), C.byref(rms)))
        else:
            items = np.ascontiguousarray(items, dtype=ENCODE_ITEM)
            self._check(lib().frac_decode(self._ctx, items.ctypes.data if len(items) else None, len(items), width,
                                          height, max_iter, rms_eps, plane.ctypes.data, C.byref(it), C.byref(rms)))
        return plane, it.value, rms.value

    def decode_frc1(self, stream, scale: int = 1, max_iter: int = -1, rms_eps: float = 1e-5,
                    initial: np.ndarray | None = None):
        """Decoder2::decode of an FRC1 stream on the GPU (frac_decode_frc1): unpacked, validated and decoded
        on the device, every coordinate and size multiplied by `scale` (1..16).  `initial` as in decode(),
        sized scale·H × scale·W.  Returns (plane, iterations, rms)."""
        h = frc1_info(stream)
        k = scale if 1 <= scale <= 16 else 0  # the library refuses the scale; no plane is sized by it
        W, H = k * h["width"], k * h["height"]
        plane = np.zeros((H, W), np.uint8) if initial is None else np.ascontiguousarray(initial, np.uint8).copy()
        if plane.shape != (H, W):
            raise FracError(f"decode_frc1: initial must be {H}x{W}")
        buf = np.frombuffer(stream, dtype=np.uint8)
        it = C.c_int()
        rms = C.c_double()
        self._check(lib().frac_decode_frc1(self._ctx, buf.ctypes.data, len(buf), scale, max_iter, rms_eps,
                                           plane.ctypes.data, plane.size, C.byref(it), C.byref(rms)))
        return plane, it.value, rms.value

    def decode_frq1(self, stream, scale: int = 1, max_iter: int = -1, rms_eps: float = 1e-5,
                    initial: np.ndarray | None = None):
        """Decoder2::decode of an FRQ1 quadtree stream on the GPU (frac_decode_frq1): laid out, validated and
        decoded on the device, every coordinate and size multiplied by `scale` (1..16).  `initial` as in
        decode(), sized scale·H × scale·W.  Returns (plane, iterations, rms)."""
        h = frq1_info(stream)
        k = scale if 1 <= scale <= 16 else 0  # the library refuses the scale; no plane is sized by it
        W, H = k * h["width"], k * h["height"]
        plane = np.zeros((H, W), np.uint8) if initial is None else np.ascontiguousarray(initial, np.uint8).copy()
        if plane.shape != (H, W):
            raise FracError(f"decode_frq1: initial must be {H}x{W}")
        buf = np.frombuffer(stream, dtype=np.uint8)
        it = C.c_int()
        rms = C.c_double()
        self._check(lib().frac_decode_frq1(self._ctx, buf.ctypes.data, len(buf), scale, max_iter, rms_eps,
                                           plane.ctypes.data, plane.size, C.byref(it), C.byref(rms)))
        return plane, it.value, rms.value

    def decode_inter(self, stream, ref, scale: int = 1, out=None):
        """An FRC1 or FRQ1 stream applied once to the reference plane `ref` (frac_decode_inter): the plane is a copy
        of `ref` in which every record or leaf with a domain has written its range from its domain patch in `ref`,
        every coordinate and size multiplied by `scale`.  One pass: no iterations, no rms.  `ref` is scale·H ×
        scale·W: a numpy uint8 array (the host call; a numpy plane is returned), or a CUDA uint8 tensor, read in
        place (frac_decode_inter_device; rows may be strided); the pixels then go into `out`, a CUDA uint8 tensor
        of that shape that does not overlap `ref` (rows may be strided; the bytes between them stay), or into a new
        tensor.  Returns the plane."""
        if not 1 <= scale <= 16:
            raise FracError("decode_inter: scale must be in 1..16")
        W, H = _stream_frame(stream)
        W, H = scale * W, scale * H
        buf = np.frombuffer(stream, dtype=np.uint8)
        if hasattr(ref, "is_cuda") and ref.is_cuda:
            import torch

            if out is None:
                out = torch.empty((H, W), dtype=torch.uint8, device=ref.device)
            for name, t in (("ref", ref), ("out", out)):
                if not (hasattr(t, "is_cuda") and t.is_cuda) or t.dtype != torch.uint8 or t.dim() != 2:
                    raise FracError(f"decode_inter: {name} must be a 2-D CUDA uint8 tensor")
                if tuple(t.shape) != (H, W):
                    raise FracError(f"decode_inter: {name} must be {H}x{W}")
                if t.stride(1) != 1 and t.shape[1] > 1:
                    raise FracError(f"decode_inter: {name} rows must be contiguous (stride(1) == 1)")
            rs, ps = _device_rows(ref, W, "decode_inter"), _device_rows(out, W, "decode_inter")
            torch.cuda.current_stream(ref.device).synchronize()  # pending work on ref and out lands first
            self._check(lib().frac_decode_inter_device(self._ctx, buf.ctypes.data, len(buf), scale,
                                                       C.c_void_p(ref.data_ptr()), rs, C.c_void_p(out.data_ptr()), ps,
                                                       ps * (H - 1) + W))
            self.sync()
            return out
        if out is not None:
            raise FracError("decode_inter: out goes with a CUDA ref")
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        if ref.shape != (H, W):
            raise FracError(f"decode_inter: ref must be {H}x{W}")
        plane = np.zeros((H, W), np.uint8)
        self._check(lib().frac_decode_inter(self._ctx, buf.ctypes.data, len(buf), scale, ref.ctypes.data,
                                            plane.ctypes.data, plane.size))
        return plane

    def inter_error(self, stream) -> dict:
        """The error of an FRC1 or FRQ1 stream applied once, at scale 1, to the plane the domains lie on, against
        the plane the ranges lie on (frac_inter_error): after set_planes(source, target) the exact decoded error of
        an inter-coded frame, after set_frame the quantized collage error of an ordinary stream.  Over
        decode_error's covered rectangle; nothing crosses PCIe.  Returns a dict with sse, pixels and psnr."""
        buf = np.frombuffer(stream, dtype=np.uint8)
        sse, pixels = C.c_uint64(0), C.c_uint64(0)
        self._check(lib().frac_inter_error(self._ctx, buf.ctypes.data if len(buf) else None, len(buf), C.byref(sse),
                                           C.byref(pixels)))
        return {"sse": sse.value, "pixels": pixels.value, "psnr": _psnr(sse.value, pixels.value)}

    def _frq1_buffer(self, max_size: int, min_size: int, contrast_bits: int, brightness_bits: int):
        """A byte buffer kept across calls that holds any FRQ1 stream of this frame at these sizes and widths: every
        node split (frq1_size) plus a dword of padding per section; 64 bytes where the library will refuse the
        arguments anyway."""
        W, H = self._frame_wh
        try:
            n0 = (W // max_size) * (H // max_size) if min(W, H) >= max_size > 0 else 0
            cap = frq1_size(W, H, max_size, min_size, [n0, 4 * n0, 16 * n0], self._p.transforms, contrast_bits,
                            brightness_bits) + 32
        except FracError:
            cap = 64
        buf = getattr(self, "_frq1_buf", None)
        if buf is None or len(buf) < cap:
            buf = self._frq1_buf = np.empty(cap, dtype=np.uint8)
        return buf

    def encode_quadtree_stream(self, max_size: int = 16, min_size: int = 4, split_distance: float = 10.0,
                               contrast_bits: int = 5, brightness_bits: int = 7, host_pack: bool = True):
        """The quadtree partition of the frame set on this engine as an FRQ1 stream with the engine's transforms
        and classifier flag.  host_pack=True: encode_quadtree(leaves=True) and pack_frq1 on the host.
        host_pack=False: laid out, quantized and packed on the device (frac_encode_quadtree_stream: the leaves
        never cross PCIe), the same bytes.  The host route is the default because the device route's 2.5 ms gain
        was not outside the run-to-run spread of a frame whose search takes 0.5 s.
        Returns (bytes, summed stats dict)."""
        if host_pack:
            leaves, st = self.encode_quadtree(max_size, min_size, split_distance, leaves=True)
            W, H = self._frame_wh
            return pack_frq1(leaves, W, H, max_size, min_size, self._p.transforms, bool(self._p.use_classifier),
                             contrast_bits, brightness_bits), st
        qp = FracQuadtreeParams(max_size, min_size, split_distance)
        buf = self._frq1_buffer(max_size, min_size, contrast_bits, brightness_bits)
        n, st = C.c_size_t(0), FracStats()
        self._check(lib().frac_encode_quadtree_stream(self._ctx, C.byref(qp), contrast_bits, brightness_bits,
                                                      buf.ctypes.data, len(buf), C.byref(n), C.byref(st)))
        if n.value > len(buf):
            raise FracError(f"encode_quadtree_stream: a stream of {n.value} bytes above its bound {len(buf)}")
        stream = buf[: n.value].tobytes()
        d = st.as_dict()
        d["items"] = int.from_bytes(stream[24:28], "little")  # the header's n_leaves
        return stream, d

    def encode_quadtree(self, max_size: int = 16, min_size: int = 4, split_distance: float = 10.0, out=None,
                        allow_short: bool = False, leaves: bool = False):
        """Quadtree partition of the frame set on this engine (frac_encode_quadtree): ranges of
        max_size split into quadrants while their best distance exceeds split_distance, down to
        min_size.  Returns (encode items of mixed sizes, summed stats dict).  With `out` (an
        ENCODE_ITEM array of at least (W/min_size)·(H/min_size) items, e.g. pinned host memory)
        the items are written there and a view of it is returned, without a copy; pinned host memory is
        written by the device directly (no copy command).  allow_short: `out` may be shorter — the items
        past it are counted (the stats) but not written, and the returned view is cut to `out`.
        leaves=True: 32-byte QT_LEAF items instead (frac_encode_quadtree_leaves; records_from_leaves rebuilds
        the records), half the bytes across PCIe."""
        qp = FracQuadtreeParams(max_size, min_size, split_distance)
        n = C.c_size_t(0)
        st = FracStats()
        W, H = self._frame_wh
        cap = max((W // min_size) * (H // min_size), 1)
        dt = QT_LEAF if leaves else ENCODE_ITEM
        if out is not None:
            if out.dtype != dt or not out.flags.c_contiguous or (len(out) < cap and not allow_short):
                raise ValueError(f"out must be a contiguous {'QT_LEAF' if leaves else 'ENCODE_ITEM'} array of at "
                                 f"least {cap} items")
            buf = out
            cap = len(out)
        else:
            # one pass with a worst-case capacity (every range at min_size), in a buffer kept across
            # calls: a fresh one costs a page fault per 4 KiB on first touch
            attr = "_qt_leaf_buf" if leaves else "_qt_buf"
            buf = getattr(self, attr, None)
            if buf is None or len(buf) < cap:
                buf = np.empty(cap, dtype=dt)
                setattr(self, attr, buf)
        fn = lib().frac_encode_quadtree_leaves if leaves else lib().frac_encode_quadtree
        self._check(fn(self._ctx, C.byref(qp), buf.ctypes.data, cap, C.byref(n), C.byref(st)))
        d = st.as_dict()
        d["items"] = n.value
        return (buf[: min(n.value, cap)] if out is not None else buf[: n.value].copy()), d

    def quadtree_rate(self, max_size: int = 16, min_size: int = 4) -> dict:
        """Search the full quadtree of the frame set on this engine once (frac_quadtree_rate_build): every node
        of every level, whatever a split distance would reach.  Afterwards rate_sizes, rate_fit and rate_leaves
        answer for any split distance without a search, until the next setter, run() or encode_quadtree().
        Returns the summed stats dict."""
        st = FracStats()
        self._check(lib().frac_quadtree_rate_build(self._ctx, max_size, min_size, C.byref(st)))
        self._rate_sizes = (max_size, min_size)
        return st.as_dict()

    def rate_sizes(self, splits, contrast_bits: int = 5, brightness_bits: int = 7):
        """Per split distance in `splits` (any doubles) what encode_quadtree_stream would return there:
        (bytes uint64 [n], leaves uint32 [n], per-level split counts uint32 [n, 4])."""
        t = np.ascontiguousarray(splits, dtype=np.float64).reshape(-1)
        n = len(t)
        size, leaves, s = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros((n, 4), np.uint32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if n else None  # noqa: E731
        self._check(lib().frac_quadtree_rate_sizes(self._ctx, contrast_bits, brightness_bits, ptr(t), n, ptr(size),
                                                   ptr(leaves), ptr(s)))
        return size, leaves, s

    def rate_fit(self, max_bytes: int, contrast_bits: int = 5, brightness_bits: int = 7):
        """The smallest split distance whose FRQ1 stream has at most max_bytes (exact: the minimum over every
        candidate of the full tree) → (split distance, bytes, leaves).  FracError when nothing fits."""
        t, size, leaves = C.c_double(0.0), C.c_uint64(0), C.c_uint32(0)
        self._check(lib().frac_quadtree_rate_fit(self._ctx, contrast_bits, brightness_bits, max_bytes, C.byref(t),
                                                 C.byref(size), C.byref(leaves)))
        return t.value, size.value, leaves.value

    def rate_leaves(self, split: float, out=None, allow_short: bool = False) -> np.ndarray:
        """The QT_LEAF leaves of the partition at `split`, as encode_quadtree(leaves=True) returns them, from the
        rate state (no search).  `out`: a contiguous QT_LEAF array (e.g. pinned host memory, which the device
        writes directly) of at least (W/min_size)·(H/min_size) items, or shorter with allow_short (the leaves
        past it are counted but not written); a view of it is returned."""
        W, H = self._frame_wh
        m = getattr(self, "_rate_sizes", (0, 0))[1]  # no build yet: the library refuses the call
        cap = max((W // m) * (H // m), 1) if m else 1
        if out is not None:
            if out.dtype != QT_LEAF or not out.flags.c_contiguous or (len(out) < cap and not allow_short):
                raise ValueError(f"out must be a contiguous QT_LEAF array of at least {cap} items")
            buf, cap = out, len(out)
        else:
            buf = np.empty(cap, dtype=QT_LEAF)
        n = C.c_size_t(0)
        self._check(lib().frac_quadtree_rate_leaves(self._ctx, split, buf.ctypes.data, cap, C.byref(n)))
        return buf[: min(n.value, cap)]

    def rate_stream(self, split: float, contrast_bits: int = 5, brightness_bits: int = 7) -> bytes:
        """The FRQ1 stream of the partition at `split` from the rate state (frac_quadtree_rate_stream): the bytes
        pack_frq1 makes of rate_leaves(split), laid out, quantized and packed on the device — no search, and no
        leaf crosses PCIe."""
        mx, mn = getattr(self, "_rate_sizes", (0, 0))  # no build yet: the library refuses the call
        buf = self._frq1_buffer(mx, mn, contrast_bits, brightness_bits)
        n = C.c_size_t(0)
        self._check(lib().frac_quadtree_rate_stream(self._ctx, split, contrast_bits, brightness_bits, buf.ctypes.data,
                                                    len(buf), C.byref(n)))
        if n.value > len(buf):
            raise FracError(f"rate_stream: a stream of {n.value} bytes above its bound {len(buf)}")
        return buf[: n.value].tobytes()

    def rd_sizes(self, lambdas, contrast_bits: int = 5, brightness_bits: int = 7):
        """Per multiplier in `lambdas` (integers in [0, 2^32]) the rate–distortion-pruned partition of the rate
        state's tree (frac_quadtree_rd_sizes; include/fracenc.h states the rule), every multiplier in one pass:
        (bytes uint64 [n], leaves uint32 [n], per-level split counts uint32 [n, 4], distortion uint64 [n] —
        16 × the leaves' summed squared error)."""
        lam = np.ascontiguousarray(lambdas, dtype=np.uint64).reshape(-1)
        n = len(lam)
        size, leaves, s = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros((n, 4), np.uint32)
        dist = np.zeros(n, np.uint64)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if n else None  # noqa: E731
        self._check(lib().frac_quadtree_rd_sizes(self._ctx, contrast_bits, brightness_bits, ptr(lam), n, ptr(size),
                                                 ptr(leaves), ptr(s), ptr(dist)))
        return size, leaves, s, dist

    def rd_fit(self, max_bytes: int, contrast_bits: int = 5, brightness_bits: int = 7):
        """A multiplier whose pruned partition's FRQ1 stream has at most max_bytes while the multiplier below it
        does not fit (or 0) → (lambda, bytes, leaves, distortion).  FracError when nothing fits."""
        lam, size, leaves, dist = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
        self._check(lib().frac_quadtree_rd_fit(self._ctx, contrast_bits, brightness_bits, max_bytes, C.byref(lam),
                                               C.byref(size), C.byref(leaves), C.byref(dist)))
        return lam.value, size.value, leaves.value, dist.value

    def rd_leaves(self, lam: int, contrast_bits: int = 5, brightness_bits: int = 7, out=None,
                  allow_short: bool = False) -> np.ndarray:
        """The QT_LEAF leaves of the pruned partition at multiplier `lam`, in canonical order, from the rate state
        (no search).  `out` and allow_short as in rate_leaves."""
        W, H = self._frame_wh
        m = getattr(self, "_rate_sizes", (0, 0))[1]  # no build yet: the library refuses the call
        cap = max((W // m) * (H // m), 1) if m else 1
        if out is not None:
            if out.dtype != QT_LEAF or not out.flags.c_contiguous or (len(out) < cap and not allow_short):
                raise ValueError(f"out must be a contiguous QT_LEAF array of at least {cap} items")
            buf, cap = out, len(out)
        else:
            buf = np.empty(cap, dtype=QT_LEAF)
        n = C.c_size_t(0)
        self._check(lib().frac_quadtree_rd_leaves(self._ctx, contrast_bits, brightness_bits, lam, buf.ctypes.data, cap,
                                                  C.byref(n)))
        return buf[: min(n.value, cap)]

    def rd_stream(self, lam: int, contrast_bits: int = 5, brightness_bits: int = 7) -> bytes:
        """The FRQ1 stream of the pruned partition at multiplier `lam` (frac_quadtree_rd_stream): the bytes
        pack_frq1 makes of rd_leaves(lam), packed on the device like rate_stream."""
        mx, mn = getattr(self, "_rate_sizes", (0, 0))  # no build yet: the library refuses the call
        buf = self._frq1_buffer(mx, mn, contrast_bits, brightness_bits)
        n = C.c_size_t(0)
        self._check(lib().frac_quadtree_rd_stream(self._ctx, lam, contrast_bits, brightness_bits, buf.ctypes.data,
                                                  len(buf), C.byref(n)))
        if n.value > len(buf):
            raise FracError(f"rd_stream: a stream of {n.value} bytes above its bound {len(buf)}")
        return buf[: n.value].tobytes()

    def encode_quadtree_to_size(self, max_bytes: int, max_size: int = 16, min_size: int = 4,
                                contrast_bits: int = 5, brightness_bits: int = 7, host_pack: bool = False,
                                rd: bool = False):
        """The best quadtree partition of the frame set on this engine whose FRQ1 stream has at most max_bytes:
        quadtree_rate + rate_fit + rate_stream (host_pack=True: rate_leaves + pack_frq1 on the host, the same
        bytes).  Returns (bytes, info): info has the stats of the full-tree search plus split_distance (the
        smallest that fits), bytes and items.  rd=True: the rate–distortion-pruned partition instead of a split
        distance's (quadtree_rate + rd_fit + rd_stream, or rd_leaves + pack_frq1 with host_pack); info then has
        `lambda` and `distortion` in place of split_distance."""
        info = self.quadtree_rate(max_size, min_size)
        if rd:
            lam, size, n, dist = self.rd_fit(max_bytes, contrast_bits, brightness_bits)
            if host_pack:
                W, H = self._frame_wh
                stream = pack_frq1(self.rd_leaves(lam, contrast_bits, brightness_bits), W, H, max_size, min_size,
                                   self._p.transforms, bool(self._p.use_classifier), contrast_bits, brightness_bits)
            else:
                stream = self.rd_stream(lam, contrast_bits, brightness_bits)
            info.update({"lambda": lam, "distortion": dist, "bytes": size, "items": n})
            return stream, info
        t, size, n = self.rate_fit(max_bytes, contrast_bits, brightness_bits)
        if host_pack:
            leaves = self.rate_leaves(t)
            W, H = self._frame_wh
            stream = pack_frq1(leaves, W, H, max_size, min_size, self._p.transforms, bool(self._p.use_classifier),
                               contrast_bits, brightness_bits)
        else:
            stream = self.rate_stream(t, contrast_bits, brightness_bits)
        info.update(split_distance=t, bytes=size, items=n)
        return stream, info

    def decode_error(self, stream, max_iter: int = -1, rms_eps: float = 1e-5, blocks: bool = False) -> dict:
        """The decoded error of an FRC1 or FRQ1 stream against the frame set on this engine (frac_decode_error):
        decoded at scale 1 on the device and compared there with the plane the ranges lie on, over the rectangle the
        g × g grid covers (g: the FRC1 range size or the FRQ1 max_size); no plane crosses PCIe.  Returns a dict
        with sse, pixels, psnr (10·log10(255²·pixels / sse), inf at sse == 0), iterations and rms; with `blocks`
        also block_sse, the uint64 [H // g, W // g] sums of the g × g blocks."""
        buf = np.frombuffer(stream, dtype=np.uint8)
        sse, pixels, nb = C.c_uint64(0), C.c_uint64(0), C.c_size_t(0)
        it, rms = C.c_int(0), C.c_double(0.0)
        bmap = None
        if blocks:
            h = frq1_info(stream) if bytes(buf[:4]) == b"FRQ1" else frc1_info(stream)
            g = h["max_size"] if "max_size" in h else h["range_size"]
            bmap = np.zeros((h["height"] // g, h["width"] // g) if g else (0, 0), np.uint64)
        self._check(lib().frac_decode_error(self._ctx, buf.ctypes.data, len(buf), max_iter, rms_eps, C.byref(sse),
                                            C.byref(pixels), bmap.ctypes.data if blocks and bmap.size else None,
                                            bmap.size if blocks else 0, C.byref(nb), C.byref(it), C.byref(rms)))
        out = {"sse": sse.value, "pixels": pixels.value, "psnr": _psnr(sse.value, pixels.value),
               "iterations": it.value, "rms": rms.value}
        if blocks:
            if nb.value != bmap.size:
                raise FracError(f"decode_error: {nb.value} blocks, {bmap.size} expected")
            out["block_sse"] = bmap
        return out

    def rate_errors(self, splits, contrast_bits: int = 5, brightness_bits: int = 7, max_iter: int = -1,
                    rms_eps: float = 1e-5):
        """Per split distance in `splits` the decoded error of the rate state's stream there
        (frac_quadtree_rate_errors): decode_error(rate_stream(t)) without a plane or a leaf crossing PCIe.
        Returns (sse uint64 [n], bytes uint64 [n], iterations int32 [n])."""
        t = np.ascontiguousarray(splits, dtype=np.float64).reshape(-1)
        n = len(t)
        sse, size, it = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if n else None  # noqa: E731
        self._check(lib().frac_quadtree_rate_errors(self._ctx, contrast_bits, brightness_bits, ptr(t), n, max_iter,
                                                    rms_eps, ptr(sse), ptr(size), ptr(it)))
        return sse, size, it

    def _rate_pixels(self) -> int:
        """The area the rate state's level-0 grid covers (0 before a build)."""
        W, H = self._frame_wh
        g = getattr(self, "_rate_sizes", (0, 0))[0]
        return (W - W % g) * (H - H % g) if g else 0

    def rate_quality(self, max_sse: int | None = None, min_psnr: float | None = None, contrast_bits: int = 5,
                     brightness_bits: int = 7, max_iter: int = -1, rms_eps: float = 1e-5):
        """A split distance of the rate state whose decoded error is within the target, by the bisection
        include/fracenc.h states for frac_quadtree_rate_quality → (split distance, bytes, leaves, sse, probes).
        Exactly one of max_sse and min_psnr is given; min_psnr becomes max_sse = floor(255²·pixels / 10^(psnr/10)).
        The answer meets the target and the next larger candidate does not (unless it is the largest); the decoded
        error is not monotone in the split distance, so it need not be the largest candidate that meets it —
        rate_errors over the candidates answers that.  FracError when the smallest split distance fails."""
        if (max_sse is None) == (min_psnr is None):
            raise ValueError("rate_quality: exactly one of max_sse and min_psnr")
        if max_sse is None:
            max_sse = int(math.floor(255.0 ** 2 * self._rate_pixels() / 10.0 ** (min_psnr / 10.0)))
        t, size, leaves, sse, probes = C.c_double(0.0), C.c_uint64(0), C.c_uint32(0), C.c_uint64(0), C.c_uint32(0)
        self._check(lib().frac_quadtree_rate_quality(self._ctx, contrast_bits, brightness_bits, int(max_sse), max_iter,
                                                     rms_eps, C.byref(t), C.byref(size), C.byref(leaves),
                                                     C.byref(sse), C.byref(probes)))
        return t.value, size.value, leaves.value, sse.value, probes.value

    def encode_quadtree_to_psnr(self, min_psnr: float, max_size: int = 16, min_size: int = 4,
                                contrast_bits: int = 5, brightness_bits: int = 7, max_iter: int = -1,
                                rms_eps: float = 1e-5):
        """A quadtree partition of the frame set on this engine whose decoded PSNR is at least min_psnr:
        quadtree_rate + rate_quality + rate_stream.  Returns (bytes, info): info has the stats of the full-tree
        search plus split_distance, bytes, items, sse, pixels, psnr and probes."""
        info = self.quadtree_rate(max_size, min_size)
        t, size, n, sse, probes = self.rate_quality(None, min_psnr, contrast_bits, brightness_bits, max_iter, rms_eps)
        stream = self.rate_stream(t, contrast_bits, brightness_bits)
        pixels = self._rate_pixels()
        info.update(split_distance=t, bytes=size, items=n, sse=sse, pixels=pixels, psnr=_psnr(sse, pixels),
                    probes=probes)
        return stream, info

    def classify(self, items: np.ndarray, target_plane: bool = False) -> np.ndarray:
        """BrightnessBlocksClassifier2 categories of `items` computed on the device plane set by
        set_frame / set_planes (returns a copy with the categories filled in)."""
        items = np.ascontiguousarray(items, dtype=GRID_ITEM).copy()
        self._check(lib().frac_classify_items(self._ctx, items.ctypes.data if len(items) else None, len(items),
                                              int(target_plane)))
        return items

    def rgb_to_yuv(self, rgb):
        """ImageIO::rgb2yuv on the device (image/ImageIO.cpp:43-58).

        rgb: numpy uint8 [H, W, 3] → numpy (Y [H, W], U [H/2, W/2], V [H/2, W/2]); or a CUDA
        uint8 tensor [H, W, 3] (rows may be strided) → CUDA tensors, enqueued on this
        engine's stream and synchronised before returning."""
        if hasattr(rgb, "is_cuda") and rgb.is_cuda:
            import torch

            assert rgb.dtype == torch.uint8 and rgb.dim() == 3 and rgb.shape[2] == 3
            assert rgb.stride(2) == 1 and rgb.stride(1) == 3, "pixels must be packed RGB"
            H, W = rgb.shape[0], rgb.shape[1]
            y = torch.empty((H, W), dtype=torch.uint8, device=rgb.device)
            u = torch.empty((H // 2, W // 2), dtype=torch.uint8, device=rgb.device)
            v = torch.empty_like(u)
            torch.cuda.current_stream(rgb.device).synchronize()  # rgb must be ready before our stream reads it
            self._check(lib().frac_rgb_to_yuv_device(self._ctx, C.c_void_p(rgb.data_ptr()), W, H, rgb.stride(0),
                                                     C.c_void_p(y.data_ptr()), W, C.c_void_p(u.data_ptr()),
                                                     max(W // 2, 1), C.c_void_p(v.data_ptr()), max(W // 2, 1)))
            self.sync()
            return y, u, v
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        assert rgb.ndim == 3 and rgb.shape[2] == 3
        H, W = rgb.shape[:2]
        y = np.zeros((H, W), np.uint8)
        u = np.zeros((H // 2, W // 2), np.uint8)
        v = np.zeros((H // 2, W // 2), np.uint8)
        self._check(lib().frac_rgb_to_yuv(self._ctx, rgb.ctypes.data, W, H, 3 * W, y.ctypes.data, u.ctypes.data,
                                          v.ctypes.data))
        return y, u, v

    def yuv_to_rgb(self, y, u, v):
        """ImageIO::yuv2rgb on the device (image/ImageIO.cpp:68-84), the inverse of rgb_to_yuv's layout.

        y [H, W], u and v [H/2, W/2] (H, W >= 2): numpy uint8 → numpy [H, W, 3]; or CUDA uint8 tensors (rows
        may be strided) → a CUDA tensor, enqueued on this engine's stream and synchronised before returning."""
        if all(hasattr(p, "is_cuda") and p.is_cuda for p in (y, u, v)):
            import torch

            for p, name in ((y, "y"), (u, "u"), (v, "v")):
                if p.dtype != torch.uint8 or p.dim() != 2 or (p.shape[1] > 1 and p.stride(1) != 1):
                    raise FracError(f"yuv_to_rgb: {name} must be a 2-D uint8 tensor with contiguous rows")
            H, W = int(y.shape[0]), int(y.shape[1])
            if tuple(u.shape) != (H // 2, W // 2) or tuple(v.shape) != (H // 2, W // 2):
                raise FracError(f"yuv_to_rgb: u and v must be {H // 2}x{W // 2}")
            strides = [_device_rows(p, int(p.shape[1]), "yuv_to_rgb") for p in (y, u, v)]
            rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=y.device)
            torch.cuda.current_stream(y.device).synchronize()  # the planes must be ready before our stream reads them
            self._check(lib().frac_yuv_to_rgb_device(self._ctx, C.c_void_p(y.data_ptr()), W, H, strides[0],
                                                     C.c_void_p(u.data_ptr()), strides[1], C.c_void_p(v.data_ptr()),
                                                     strides[2], C.c_void_p(rgb.data_ptr()), 3 * W))
            self.sync()
            return rgb
        if any(hasattr(p, "is_cuda") for p in (y, u, v)):
            raise FracError("yuv_to_rgb: three numpy arrays or three CUDA tensors")
        y, u, v = (np.ascontiguousarray(p, dtype=np.uint8) for p in (y, u, v))
        if y.ndim != 2 or u.shape != (y.shape[0] // 2, y.shape[1] // 2) or v.shape != u.shape:
            raise FracError("yuv_to_rgb: y must be [H, W], u and v [H/2, W/2]")
        H, W = y.shape
        rgb = np.zeros((H, W, 3), np.uint8)
        self._check(lib().frac_yuv_to_rgb(self._ctx, y.ctypes.data, u.ctypes.data, v.ctypes.data, W, H,
                                          rgb.ctypes.data, 3 * W))
        return rgb

    def decode_frc3(self, stream, scale: int = 1, max_iter: int = -1, rms_eps: float = 1e-5, out=None):
        """An FRC3 colour container to RGB on the GPU (frac_decode_frc3): each plane stream decoded as decode_frc1
        / decode_frq1 at `scale` from a zero plane, the planes converted on the device, only the RGB copied out.
        Returns (rgb [scale·H, scale·W, 3], [iterations]·3, [rms]·3).  `out`: a CUDA uint8 tensor of that shape
        (rows may be strided) receives the pixels on the device (frac_decode_frc3_device) and is returned."""
        h = frc3_info(stream)
        k = scale if 1 <= scale <= 16 else 0  # the library refuses the scale; nothing is sized by it
        W, H = k * h["width"], k * h["height"]
        buf = np.frombuffer(stream, dtype=np.uint8)
        it = (C.c_int * 3)()
        rms = (C.c_double * 3)()
        if out is not None:
            import torch

            if not (hasattr(out, "is_cuda") and out.is_cuda) or out.dtype != torch.uint8 or out.dim() != 3:
                raise FracError("decode_frc3: out must be a CUDA uint8 tensor [H, W, 3]")
            if tuple(out.shape) != (H, W, 3) or out.stride(2) != 1 or out.stride(1) != 3:
                raise FracError(f"decode_frc3: out must be {H}x{W}x3 with packed pixels")
            stride = _device_rows(out, 3 * W, "decode_frc3")
            torch.cuda.current_stream(out.device).synchronize()  # pending work on `out` lands first
            self._check(lib().frac_decode_frc3_device(self._ctx, buf.ctypes.data, len(buf), scale, max_iter, rms_eps,
                                                      C.c_void_p(out.data_ptr()), stride,
                                                      stride * max(H - 1, 0) + 3 * W, it, rms))
            self.sync()
            return out, list(it), list(rms)
        rgb = np.zeros((H, W, 3), np.uint8)
        self._check(lib().frac_decode_frc3(self._ctx, buf.ctypes.data, len(buf), scale, max_iter, rms_eps,
                                           rgb.ctypes.data, 3 * W, rgb.size, it, rms))
        return rgb, list(it), list(rms)

    def decode_error_frc3(self, stream, rgb, max_iter: int = -1, rms_eps: float = 1e-5) -> dict:
        """The decoded RGB error of an FRC3 colour container against `rgb` (frac_decode_error_frc3): the three plane
        streams decoded at scale 1 on the device as decode_frc3 decodes them, converted and compared there pixel by
        pixel, over the rectangle all three planes' g × g grids cover (include/fracenc.h states it); no RGB plane is
        written and nothing decoded crosses PCIe.  No frame needs to be set on this engine.
        rgb: a numpy uint8 [H, W, 3] array (uploaded), or a CUDA uint8 tensor [H, W, 3] with packed pixels (rows may
        be strided; read in place on this engine's stream: frac_decode_error_frc3_device).
        Returns a dict with sse (the sum of the three channels), channel_sse [R, G, B], pixels, psnr
        (10·log10(255²·3·pixels / sse), inf at sse == 0), iterations and rms (lists of three, Y, U, V)."""
        buf = np.frombuffer(stream, dtype=np.uint8)
        sse, pixels = (C.c_uint64 * 3)(), C.c_uint64(0)
        it, rms = (C.c_int * 3)(), (C.c_double * 3)()
        ptr = buf.ctypes.data if len(buf) else None
        if hasattr(rgb, "is_cuda"):
            import torch

            if not rgb.is_cuda or rgb.dtype != torch.uint8 or rgb.dim() != 3 or rgb.shape[2] != 3:
                raise FracError("decode_error_frc3: rgb must be a numpy array or a CUDA uint8 tensor [H, W, 3]")
            if rgb.stride(2) != 1 or rgb.stride(1) != 3:
                raise FracError("decode_error_frc3: rgb must have packed pixels")
            stride = _device_rows(rgb, 3 * int(rgb.shape[1]), "decode_error_frc3")
            shape = (int(rgb.shape[0]), int(rgb.shape[1]))
            torch.cuda.current_stream(rgb.device).synchronize()  # rgb must be ready before our stream reads it
            fn, ref = lib().frac_decode_error_frc3_device, C.c_void_p(rgb.data_ptr())
        else:
            rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
            if rgb.ndim != 3 or rgb.shape[2] != 3:
                raise FracError("decode_error_frc3: rgb must be [H, W, 3]")
            stride, shape = 3 * rgb.shape[1], rgb.shape[:2]
            fn, ref = lib().frac_decode_error_frc3, rgb.ctypes.data
        # the library reads the container's frame from rgb, so rgb must have that frame's shape (a container the
        # parser refuses is left to the call itself to refuse)
        h = FracFrc3Info()
        if lib().frac_frc3_info(ptr, len(buf), C.byref(h)) == 0 and tuple(shape) != (h.height, h.width):
            raise FracError(f"decode_error_frc3: rgb is {shape[1]}x{shape[0]}, the container's frame "
                            f"{h.width}x{h.height}")
        self._check(fn(self._ctx, ptr, len(buf), ref, stride, max_iter, rms_eps, sse, C.byref(pixels), it, rms))
        total = sum(sse)
        return {"sse": total, "channel_sse": list(sse), "pixels": pixels.value,
                "psnr": _psnr(total, 3 * pixels.value), "iterations": list(it), "rms": list(rms)}

    def rate_candidates(self) -> np.ndarray:
        """The rate state's candidates {0.0} ∪ {e(v)} as a float64 array, ascending and distinct
        (frac_quadtree_rate_candidates): the list rate_quality bisects."""
        n = C.c_size_t(0)
        self._check(lib().frac_quadtree_rate_candidates(self._ctx, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.float64)
        self._check(lib().frac_quadtree_rate_candidates(self._ctx, out.ctypes.data, len(out), C.byref(n)))
        if n.value != len(out):
            raise FracError(f"rate_candidates: {n.value} candidates, {len(out)} expected")
        return out

    def device_results_ptr(self) -> int:
        """The device address of the last run's records; 0 when none are readable (no run yet, or a setter
        called since the last one)."""
        return lib().frac_device_results(self._ctx) or 0


def encode(plane: np.ndarray, range_size: int = 4, domain_size: int = 16, transforms: int = 4,
           use_classifier: bool = True, rms_threshold: float = 0.0, s_max: float = -1.0, device: int = 0,
           engine: int = ENGINE_AUTO):
    """Encoder2's search half for one plane, with grids built like main.cpp:142-162 and the CLI's
    defaults (encode/encode_parameters.h:6-13): 16×16 domains at offset 16 / latticeSize 2, 4×4
    ranges, the classifier on, rms threshold 0, sMax −1."""
    plane = np.ascontiguousarray(plane, dtype=np.uint8)
    H, W = plane.shape
    dsz = domain_size
    doms = create_uniform_grid(W, H, dsz, dsz // 2)
    rngs = create_uniform_grid(W, H, range_size, range_size)
    if use_classifier:
        doms = preclassify(plane, doms)
        rngs = preclassify(plane, rngs)
    with Engine(device, transforms, use_classifier, rms_threshold, s_max, engine) as e:
        e.set_frame(plane)
        e.set_domains(doms)
        return e.search(rngs)


def decode_stream(stream, scale: int = 1, device: int = 0, **kw):
    """One call from a stream to pixels, beside encode(): Engine.decode_frc1, or Engine.decode_frq1 for a stream
    whose magic is FRQ1, on a context of its own (kw: max_iter, rms_eps, initial).  Returns (plane, iterations,
    rms)."""
    with Engine(device) as e:
        if bytes(memoryview(stream)[:4]) == b"FRQ1":
            return e.decode_frq1(stream, scale, **kw)
        return e.decode_frc1(stream, scale, **kw)


def decode_color_stream(stream, scale: int = 1, device: int = 0, **kw):
    """One call from an FRC3 colour container to RGB pixels, beside decode_stream: Engine.decode_frc3 on a context
    of its own (kw: max_iter, rms_eps, out).  Returns (rgb, [iterations]·3, [rms]·3)."""
    with Engine(device) as e:
        return e.decode_frc3(stream, scale, **kw)


def color_stream_error(stream, rgb, device: int = 0, **kw):
    """One call from an FRC3 colour container and an RGB frame to the decoded RGB error, beside
    decode_color_stream: Engine.decode_error_frc3 on a context of its own (kw: max_iter, rms_eps).  Returns its
    dict."""
    with Engine(device) as e:
        return e.decode_error_frc3(stream, rgb, **kw)


def decode_inter_stream(stream, ref, scale: int = 1, device: int = 0):
    """One call from an inter-coded stream and its reference plane to pixels, beside decode_stream:
    Engine.decode_inter on a context of its own.  Returns the plane."""
    with Engine(device) as e:
        return e.decode_inter(stream, ref, scale)


class SequenceEncoder:
    """A closed-loop encoder of a sequence of planes of one size: every `gop`-th frame, starting with the first, is
    an I frame (an ordinary quadtree stream, decoded iteratively), every other one a P frame whose domains lie on
    the previous frame's reconstruction, which the decoder has too: frame k is coded against what frame k − 1
    decodes to, so the error does not drift.

    An I frame is set_frame, encode_quadtree_stream and decode_frq1; its reconstruction is uploaded into a device
    tensor: one plane crosses PCIe per I frame, down and up again (the iterative decoders have no device output).
    A P frame stays on the device: set_planes(reconstruction, frame), encode_quadtree_stream(host_pack=False),
    decode_inter(stream, reconstruction, out=spare), and the two reconstruction tensors swap.  A numpy frame is
    uploaded first."""

    def __init__(self, device: int = 0, transforms: int = 4, max_size: int = 16, min_size: int = 4,
                 split_distance: float = 10.0, gop: int = 8, contrast_bits: int = 5, brightness_bits: int = 7,
                 use_classifier: bool = False):
        if gop < 1:
            raise FracError("SequenceEncoder: gop must be at least 1")
        self._e = Engine(device, transforms, use_classifier)
        self._device = device
        self._qt = (max_size, min_size, split_distance, contrast_bits, brightness_bits)
        self._gop = gop
        self._frames = []
        self._wh = None
        self._rec = self._spare = None

    def close(self) -> None:
        self._e.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def push(self, plane):
        """The next frame (numpy uint8 [H, W] or a CUDA uint8 tensor) → (kind, stream), kind "I" or "P"."""
        import torch

        wh = (int(plane.shape[1]), int(plane.shape[0]))
        if self._wh is None:
            self._wh = wh
            dev = torch.device("cuda", self._device)
            self._rec = torch.empty((wh[1], wh[0]), dtype=torch.uint8, device=dev)
            self._spare = torch.empty_like(self._rec)
        elif wh != self._wh:
            raise FracError(f"SequenceEncoder: a frame of {wh[0]}x{wh[1]} in a sequence of {self._wh[0]}x{self._wh[1]}")
        e = self._e
        if len(self._frames) % self._gop == 0:
            kind = "I"
            e.set_frame(plane)
            stream, _ = e.encode_quadtree_stream(*self._qt)
            rec, _, _ = e.decode_frq1(stream)
            self._rec.copy_(torch.from_numpy(rec))
        else:
            kind = "P"
            if not (hasattr(plane, "is_cuda") and plane.is_cuda):
                plane = torch.from_numpy(np.ascontiguousarray(plane, dtype=np.uint8)).to(self._rec.device)
            e.set_planes(self._rec, plane)
            stream, _ = e.encode_quadtree_stream(*self._qt, host_pack=False)
            e.decode_inter(stream, self._rec, out=self._spare)
            self._rec, self._spare = self._spare, self._rec
        self._frames.append((kind, stream))
        return kind, stream

    def reconstruction(self):
        """What a decoder makes of the frames pushed so far: the last frame's plane, a CUDA uint8 tensor that the
        next push() overwrites or retires (clone it to keep it)."""
        if not self._frames:
            raise FracError("SequenceEncoder: no frame pushed")
        return self._rec

    def pack(self) -> bytes:
        """The frames pushed so far as one FRCS container (codec.pack_sequence)."""
        from . import codec

        if self._wh is None:
            raise FracError("SequenceEncoder: no frame pushed")
        return codec.pack_sequence(self._frames, *self._wh)


def decode_sequence(data, scale: int = 1, device: int = 0):
    """An FRCS container (codec.unpack_sequence) to its planes, a list of numpy uint8 [scale·H, scale·W] arrays:
    I frames through decode_frq1 / decode_frc1, P frames through decode_inter against the previous output, which
    stays on the device between frames."""
    import torch

    from . import codec

    frames, _ = codec.unpack_sequence(data)
    planes, prev = [], None
    with Engine(device) as e:
        for kind, stream in frames:
            if kind == "I":
                fn = e.decode_frq1 if stream[:4] == b"FRQ1" else e.decode_frc1
                plane = fn(stream, scale)[0]
                prev = torch.from_numpy(plane).to(torch.device("cuda", device))
            else:
                prev = e.decode_inter(stream, prev, scale)
                plane = prev.cpu().numpy()
            planes.append(plane)
    return planes
