/*
 * fracenc.h — C ABI of the MI355X-native range×domain search engine.
 *
 * This is the drop-in boundary for the reference's hot path
 *   Frac2::AbstractEncodingEngine2 / CpuEncodingEngine2 → TransformEstimator2::estimate
 *   → TransformMatcher::match (sebsgit/fractencode encode/EncodingEngine2.hpp:50-112,
 *   encode/TransformEstimator2.hpp:29-48, encode/transformmatcher.h:38-111).
 * A caller owns the planes and grids; a context owns every device buffer.
 * No torch or HIP types cross this boundary: plain pointers, sizes and status ints.
 *
 * Semantics (identical to the reference on the same inputs):
 *  - domains are visited in the order given (the reference's createUniformGrid
 *    order), ties in distance go to the earliest domain and, inside a domain,
 *    to the later transform; the first candidate with distance <= rms_threshold
 *    wins (early exit); distance is the reference's unfitted fp32 error;
 *  - contrast / brightness follow TransformMatcher::match_generic bit-for-bit;
 *  - geometry: n x n ranges (n >= 2; Size32u rectangles too) and S x S domains with S > n, the pairs
 *    the reference CLI accepts (main.cpp:99); S = 2n is the decimate-then-permute path, any other
 *    pair — the CLI default 16 -> 4 (match_16to4) included — samples as RootMeanSquare does; range
 *    sides above 256 run every candidate in the reference's fp32 arithmetic (slower, same records);
 *  - results are returned in the order the ranges were given.
 * All entry points return 0 on success and a negative FRAC_E* code on error;
 * frac_last_error() gives the message.  Not thread-safe per context.
 */
#ifndef FRACENC_H
#define FRACENC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FRAC_ABI_VERSION 9

/* error codes */
#define FRAC_OK 0
#define FRAC_E_INVALID (-1)     /* bad argument / geometry the engine does not support   */
#define FRAC_E_DEVICE (-2)      /* HIP runtime error                                     */
#define FRAC_E_STATE (-3)       /* call order (e.g. run before planes/grids are set)     */
#define FRAC_E_NOMEM (-4)       /* device or host allocation failed                      */

/* engines (frac_params.engine) */
#define FRAC_ENGINE_AUTO 0      /* fastest engine that supports the geometry.  n = 8, T = 4, ratio 2 on a  */
                                /* large enough run: the MFMA search pruned by the exact elimination bound  */
                                /* (the tiled SEA form's windows), falling back to the exhaustive Fourier   */
                                /* search in the same run when the windows are not small; same records      */
#define FRAC_ENGINE_VALU 1      /* v_dot2_u32_u16 scalar-broadcast search                */
#define FRAC_ENGINE_MFMA 2      /* f16 MFMA search with an exact integer epilogue        */
#define FRAC_ENGINE_SEA 3       /* successive elimination: exact per-candidate bound skips   */
                                /* domains that cannot win; same result, data-dependent cost */

/* flags (frac_params.flags) */
#define FRAC_FLAG_TIMING 1u     /* record per-kernel device time with HIP events         */
/* Alternative exact forms (same records, other kernels; for cross-checks, ABI 6).  They replace
 * the FRAC_MFMA_DFT / FRAC_SEA_TILED / FRAC_DECODE_UNFUSED environment knobs of ABI 5, which a
 * product build now refuses (FRAC_E_INVALID) like every other A/B knob. */
#define FRAC_FLAG_DIRECT_FORM 2u    /* MFMA engine, ratio-2 n = 8 and 16: the direct form (T GEMMs of K = n²)  */
                                    /* instead of the rotation-group Fourier form                               */
#define FRAC_FLAG_SEA_PER_RANGE 4u  /* SEA engine, n = 8, T = 4: the per-range form instead of the tiled one   */
#define FRAC_FLAG_DECODE_STEPWISE 8u /* decoder: one apply + one rms launch per iteration (no fused loop)       */
/* FRAC_ENGINE_AUTO's pruned route (n = 8, T = 4, ratio 2; added after ABI 9 without changing FRAC_ABI_VERSION:
 * an older library refuses them as unknown flag bits).  Neither changes a record; an explicit engine ignores both. */
#define FRAC_FLAG_EXHAUSTIVE 16u    /* AUTO never prunes: a run time that does not depend on the frame's content */
#define FRAC_FLAG_PRUNE 32u         /* AUTO prunes whenever the geometry allows it, however small the run        */
                                    /* (FRAC_FLAG_EXHAUSTIVE wins when both are set)                             */

/* == Frac2::UniformGridItem (image/partition2.hpp:93-99): GridItemBase{origin, size}
 *    + GridItemData{bb_classifierBin}; 20 bytes. category -1 = not classified
 *    (recomputed on the item's own plane, as Classifier2::compare does). */
typedef struct frac_grid_item {
    uint32_t x, y, w, h;
    int32_t category;
} frac_grid_item;

/* Search parameters; the Frac::encode_parameters_t fields that reach the search
 * (encode/encode_parameters.h:5-14, encode/Encoder2.hpp:36). */
typedef struct frac_params {
    uint32_t transforms;    /* 4 = TransformMatcher::match's Id,R90,R180,R270; 8 = all of image/transform.h */
    int32_t use_classifier; /* 0 = DummyClassifier, 1 = BrightnessBlocksClassifier2 gating           */
    double rms_threshold;   /* TransformMatcher rmsThreshold (early-exit distance), default 0.0       */
    double s_max;           /* TransformMatcher sMax (|contrast| clamp when > 0), default -1.0         */
    uint32_t engine;        /* FRAC_ENGINE_*                                                           */
    uint32_t flags;         /* FRAC_FLAG_*                                                             */
} frac_params;

/* == Frac::transform_score_t (encode/datatypes.h:8-13), 32 bytes */
typedef struct frac_score {
    double distance;
    double contrast;
    double brightness;
    int32_t transform; /* Frac::TransformType */
    int32_t _pad;
} frac_score;

/* == Frac::item_match_t (encode/datatypes.h:14-19), 48 bytes */
typedef struct frac_match {
    frac_score score;
    uint32_t x, y;   /* winning domain origin */
    uint32_t sw, sh; /* winning domain size (sourceItemSize); 0,0 when no domain was eligible */
} frac_match;

/* == Frac::encode_item_t (encode/datatypes.h:20-23), 64 bytes */
typedef struct frac_encode_item {
    uint32_t x, y, w, h; /* range */
    frac_match match;
} frac_encode_item;

typedef struct frac_stats {
    uint64_t rejected_mappings; /* == TransformEstimator2::rejectedMappings() for this search   */
    uint64_t total_mappings;    /* nd * nr (Encoder2::encode_stats_t::totalMappings)              */
    uint32_t hit_ranges;        /* ranges decided by the rms threshold                           */
    uint32_t fallback_ranges;   /* ranges re-run in fp32 emulation (min error >= 2^24/16)        */
    uint32_t empty_ranges;      /* ranges with no eligible domain (default record)               */
    uint32_t engine;            /* engine that ran                                               */
    double ms_device;           /* device time of the last run (FRAC_FLAG_TIMING), else 0        */
    double ms_search;           /* device time of the search kernel alone                        */
    double ms_prep;             /* domain pool / operand build                                   */
    double ms_finish;           /* winner fit + fallback                                         */
    uint32_t search_form;       /* FRAC_FORM_*: how the search kernel computed the candidates     */
    uint32_t pad_;
    uint64_t matrix_flops;      /* MFMA flops the search issued (0 for the VALU engine)          */
    uint64_t evaluated_mappings; /* (range, domain) pairs whose error was computed: every eligible */
                                 /* pair for the exhaustive engines, the bound's survivors (SEA)   */
} frac_stats;

/* frac_stats.search_form */
#define FRAC_FORM_DOT2 0    /* VALU engine: packed-u16 v_dot2 per (range, transform, domain)       */
#define FRAC_FORM_DIRECT 1  /* MFMA engine: one f16 GEMM per transform (n²·T MACs per pair)        */
#define FRAC_FORM_FOURIER 2 /* MFMA engine, n = 8, T = 4: rotation-group Fourier form (96 MACs)    */
#define FRAC_FORM_SEA 3     /* SEA engine: bound-pruned exact evaluation (v_dot2)                */
#define FRAC_FORM_SEA_MFMA 4 /* SEA engine, and AUTO's pruned route (engine = MFMA), n = 8, T = 4: the bound */
                             /* per tile pair, Fourier MFMA search over the surviving windows              */
#define FRAC_FORM_SAMPLED 5 /* range sizes outside {2,4,8,16}: per range an exact integer scan of the */
                            /* pool rows, one per (domain, transform), sampled as RootMeanSquare does  */

typedef struct frac_ctx frac_ctx;

int frac_abi_version(void);
/* The 16-hex-digit id of the sources this library was built from (compiled in by the build:
 * a hash of csrc/ and this header), "unknown" for a build that did not pass one. */
const char* frac_build_id(void);
/* FRAC_BUILD_* bits of this library build. */
#define FRAC_BUILD_TUNING 1 /* -DFRAC_TUNING: ablation variants (wrong results by design) compiled in */
int frac_build_flags(void);
/* The number of HIP devices this process sees (ABI 7), or a negative FRAC_E_DEVICE: a caller without
 * the HIP runtime (the reference's EncodingEngineCore2) registers one engine per device with it
 * (Multi-GPU). */
int frac_device_count(void);
/* NULL on failure (message via frac_last_error(NULL)). */
frac_ctx* frac_create(int device, const frac_params* params);
void frac_destroy(frac_ctx* ctx);
const char* frac_last_error(const frac_ctx* ctx);
/* When results are readable.  A context is meant to live long: frame after frame, with parameters, grids and
 * planes changed between runs.  The results of a run are readable from that frac_run until the next call of
 * a setter — frac_set_params, frac_set_domains, frac_set_ranges, frac_set_frame, frac_set_planes,
 * frac_set_frame_device, frac_set_frame_device_async, frac_set_frame_async — or of frac_encode_quadtree /
 * frac_encode_quadtree_leaves / frac_encode_quadtree_stream / frac_quadtree_rate_build (which search lists of
 * their own).  From such a call to
 * the next frac_run every reader — frac_fetch, frac_fetch_tuples, frac_copy_tuples_device,
 * frac_copy_results_device, frac_pack_frc1, frac_decode_results — returns FRAC_E_STATE, and
 * frac_device_results returns NULL: the old winners are never paired with the new parameters, domain list,
 * ranges or planes.  A setter that fails its own argument checks changes nothing.  frac_set_stream,
 * frac_set_tuple_sink, frac_sync, frac_classify_items, frac_decode,
 * frac_decode_frc1, frac_decode_frq1, frac_decode_frc3, frac_decode_frc3_device and the colour conversions
 * (frac_rgb_to_yuv, frac_rgb_to_yuv_device, frac_yuv_to_rgb, frac_yuv_to_rgb_device) leave the results readable.
 * The rate state of frac_quadtree_rate_build has the same life, from that call: it is readable
 * (frac_quadtree_rate_sizes, frac_quadtree_rate_fit, frac_quadtree_rate_leaves, frac_quadtree_rate_stream, and the
 * rate–distortion readers frac_quadtree_rd_sizes, frac_quadtree_rd_fit, frac_quadtree_rd_leaves,
 * frac_quadtree_rd_stream) until
 * the next setter above, frac_run, frac_encode_quadtree / frac_encode_quadtree_leaves /
 * frac_encode_quadtree_stream or frac_quadtree_rate_build, after which its readers return FRAC_E_STATE; the calls that leave a run's results readable leave it readable too, and so do
 * its own readers. */
int frac_set_params(frac_ctx* ctx, const frac_params* params);

/* Planes are uint8, row-major with the given stride (bytes). Copied to the device.
 * frac_set_frame: source == target (what Encoder2 does, encode/Encoder2.hpp:36).
 * frac_set_planes: distinct source (domain) and target (range) planes, as
 * TransformEstimator2's constructor allows (encode/TransformEstimator2.hpp:15-21).
 * Every plane setter below ends the last run's results until the next frac_run.
 * Both calls block: on return the caller's planes have been consumed and may be overwritten or freed.  They do
 * not wait for the runs already enqueued.  The first planes of a geometry go into the context's plane buffers on
 * its stream.  Planes that follow others of the same geometry (sizes, and whether a distinct target is given)
 * are uploaded on a copy stream of the context's own into a second buffer per plane, while the kernels of the
 * previous frac_run still run; the context's stream waits for the upload and the buffers swap, so in a loop of
 * frac_set_frame; frac_run the upload of frame k+1 overlaps what is left of frame k's run.  A context that is
 * given one frame only allocates no second buffer and creates no stream. */
int frac_set_frame(frac_ctx* ctx, const uint8_t* plane, uint32_t w, uint32_t h, uint32_t stride);
int frac_set_planes(frac_ctx* ctx, const uint8_t* src, uint32_t sw, uint32_t sh, uint32_t sstride,
                    const uint8_t* tgt, uint32_t tw, uint32_t th, uint32_t tstride);
/* Planes already in device memory (e.g. a torch tensor in HBM): copied device-to-device. */
int frac_set_frame_device(frac_ctx* ctx, const void* d_plane, uint32_t w, uint32_t h, uint32_t stride);
/* ABI 9: the same copy enqueued on the context's stream without waiting for it, so a caller can stream
 * frames: upload frame k+1 on a stream of its own while frame k searches, make the context's stream wait
 * for that upload (an event), then call this and frac_run.  d_plane must stay unchanged until the
 * context's stream has passed the copy (an event recorded on it after this call).  The first frame of a
 * geometry, or any frame with the classifier on, re-prepares on the host in the next frac_run. */
int frac_set_frame_device_async(frac_ctx* ctx, const void* d_plane, uint32_t w, uint32_t h, uint32_t stride);
/* ABI 9: frame streaming from host memory: frac_set_frame without the host's wait for the upload.  The plane
 * (pinned host memory for an asynchronous copy) is uploaded as frac_set_frame uploads it: after a frame of the
 * same geometry on the context's own copy stream into the second plane buffer while the runs already enqueued
 * still read the current one; the context's stream waits for the upload and the buffers swap.  frac_run right
 * after it searches the new frame, so frame k+1 crosses PCIe while frame k searches.  The host plane must stay unchanged
 * until the upload is done: until a later frac_sync / frac_fetch, or an event recorded on the context's stream
 * after this call. */
int frac_set_frame_async(frac_ctx* ctx, const uint8_t* plane, uint32_t w, uint32_t h, uint32_t stride);

/* The domain pool (TransformEstimator2's sourceGrid) and the range list.  Either call, like
 * frac_set_params and the plane setters, ends the last run's results until the next frac_run. */
int frac_set_domains(frac_ctx* ctx, const frac_grid_item* domains, size_t nd);
int frac_set_ranges(frac_ctx* ctx, const frac_grid_item* ranges, size_t nr);

/* Launch the whole search for the current planes/grids on the context's stream
 * (asynchronous).  frac_fetch waits for it and copies results/stats to the host.
 * On FRAC_ENGINE_AUTO's pruned route (and on FRAC_ENGINE_SEA's tiled form) frac_run blocks the host once,
 * mid-run: it waits for the window sizes (one 32-byte copy) before it sizes and launches the search over
 * them, or the exhaustive search when they exceed the budget.  The rest of the run is asynchronous as ever. */
int frac_run(frac_ctx* ctx);
int frac_fetch(frac_ctx* ctx, frac_encode_item* out, frac_stats* stats);
int frac_sync(frac_ctx* ctx);

/* Per-run device times (FRAC_FLAG_TIMING): the ms_device / ms_prep / ms_search / ms_finish of
 * every frac_run since the previous call that passed `out` (at most the last 256 runs), oldest
 * first, from HIP events recorded on the context's stream around each phase.  Waits for the
 * stream.  *n_out = the run count; writes min(count, cap) entries (out may be NULL to query).
 * Lets a benchmark time the search kernel of exactly the runs of its timed region. */
typedef struct frac_run_timing {
    double ms_device, ms_prep, ms_search, ms_finish;
} frac_run_timing;
int frac_timing_history(frac_ctx* ctx, frac_run_timing* out, size_t cap, size_t* n_out);

/* One-shot: set_ranges + run + fetch (the shape of AbstractEncodingEngine2::encode
 * applied to a batch of range items). */
int frac_search(frac_ctx* ctx, const frac_grid_item* ranges, size_t nr, frac_encode_item* out, frac_stats* stats);

/* Use an external hipStream_t (passed as void*); NULL restores the context's own.  Work the context
 * enqueued on its previous stream comes before anything it enqueues on the new one (an event). */
int frac_set_stream(frac_ctx* ctx, void* hip_stream);
void* frac_get_stream(frac_ctx* ctx);
/* Device pointer to the nr frac_encode_item results of the last run (valid until the next setter call,
 * frac_run or destroy; see "When results are readable"); used for device-side gathers (RCCL).  NULL when
 * no results are readable: before the first frac_run, and between a setter call and the next frac_run. */
const frac_encode_item* frac_device_results(frac_ctx* ctx);
/* Asynchronous device-to-device copy of the last run's nr results into d_dst
 * (ordered on the context's stream). */
int frac_copy_results_device(frac_ctx* ctx, void* d_dst);

/* The winner of one range as north_star's multi-GPU gather names it — (domain, transform,
 * s, o, rms) — in 32 bytes instead of the 64-byte encode_item_t: the range geometry is
 * known to every rank and the domain's origin and size follow from its index.
 * domain = index into the list given to frac_set_domains; FRAC_NO_DOMAIN when no domain
 * was eligible (the default record of encode/datatypes.h:8-26). */
#define FRAC_NO_DOMAIN 0xffffffffu
typedef struct frac_tuple {
    uint32_t domain;
    int32_t transform;
    double contrast, brightness, distance;
} frac_tuple;
/* Asynchronous: pack the last run's nr tuples into d_dst (device memory, 32·nr bytes) on
 * the context's stream. */
int frac_copy_tuples_device(frac_ctx* ctx, void* d_dst);
/* Synchronous: the last run's nr tuples into host memory. */
int frac_fetch_tuples(frac_ctx* ctx, frac_tuple* out);
/* ABI 8: every later frac_run also writes its nr tuples into dst (32·nr bytes; device memory, or pinned host
 * memory the device can write — then they cross PCIe while the run's resolve kernels write them, with no
 * separate pack or copy), ordered on the context's stream: complete once that stream's work is.  The records
 * (frac_fetch, …) are unchanged.  NULL clears it.  The quadtree entry points ignore it. */
int frac_set_tuple_sink(frac_ctx* ctx, void* dst);

/* Decoder2::decode (encode/Encoder2.hpp:67-99) on the device.  `plane` (w×h, row
 * stride w) holds the decoder's initial target (main.cpp:171-173 zero-fills it) and
 * receives the decoded image; the source starts filled with 100.  Items must not
 * overlap; items without a domain (size 0) are skipped.  max_iter < 0 means 300.
 * Writes the iteration count and the final rms exactly as Decoder2 reports them. */
int frac_decode(frac_ctx* ctx, const frac_encode_item* items, size_t n, uint32_t w, uint32_t h, int max_iter,
                double rms_eps, uint8_t* plane, int* iterations, double* rms);
/* The same for the last frac_run's results, which stay on the device. */
int frac_decode_results(frac_ctx* ctx, uint32_t w, uint32_t h, int max_iter, double rms_eps, uint8_t* plane,
                        int* iterations, double* rms);

/* ---- quadtree partition (C4 config; the reference parses --quadtree but never builds one,
 * main.cpp:75-76, so the partition rule is this library's, parity pinned per level) ----
 * Level sizes max_size, max_size/2, ..., min_size (each 2, 4, 8 or 16).  Level-0 ranges are
 * createUniformGrid(W, H, max_size, max_size); every level searches domains
 * createUniformGrid(W, H, 2n, n) of the frame set on ctx (classifier and threshold as in the
 * ctx params; -1 categories are computed on the device).  A range whose best distance exceeds
 * split_distance and whose size exceeds min_size is replaced by its four quadrants (top-left,
 * top-right, bottom-left, bottom-right) at the next level; every other range is emitted.
 * Output order: by level, then in search order (children follow their parent's order).
 * Returns FRAC_OK and the item count in *n_out; writes min(count, cap) items (out may be NULL
 * to query the count — the search still runs).  stats (optional) sums the levels. */
typedef struct frac_quadtree_params {
    uint32_t max_size;
    uint32_t min_size;
    double split_distance;
} frac_quadtree_params;
int frac_encode_quadtree(frac_ctx* ctx, const frac_quadtree_params* qp, frac_encode_item* out, size_t cap,
                         size_t* n_out, frac_stats* stats);
/* The same partition with each leaf in 32 bytes instead of encode_item_t's 64 (ABI 7): what the frame's
 * geometry does not already determine.  A leaf of level size n at (x, y) won domain `code & 0xffffff` of
 * that level's grid createUniformGrid(W, H, 2n, n) — origin ((d % cols)·n, (d / cols)·n) with
 * cols = (W − 2n)/n + 1, size 2n — under transform (code >> 24) & 15; n = 1 << (code >> 28).
 * FRAC_QT_NO_DOMAIN: no eligible domain (the reference's default record: domain (0, 0), size (0, 0)).
 * The doubles are the record's own, bit for bit.  Frames up to 65535 pixels a side whose finest level
 * has fewer than 2^24 − 1 domains.  Into the caller's pinned host memory the device writes them directly,
 * half the PCIe bytes of the 64-byte records. */
#define FRAC_QT_NO_DOMAIN 0xffffffu
typedef struct frac_qt_leaf {
    uint16_t x, y;  /* range origin */
    uint32_t code;  /* domain index (bits 0..23) | transform (24..27) | log2 n (28..31) */
    double contrast, brightness, distance;
} frac_qt_leaf;
int frac_encode_quadtree_leaves(frac_ctx* ctx, const frac_quadtree_params* qp, frac_qt_leaf* out, size_t cap,
                                size_t* n_out, frac_stats* stats);

/* ---- classifier pre-pass on the device (BrightnessBlocksClassifier2::preclassify,
 * encode/Classifier2.cpp:55-68, as main.cpp:155-162 runs it at grid build) ----
 * Writes the category (0..5 or -1) of each item, computed on the context's source plane
 * (target_plane = 0) or target plane (1) already on the device.  frac_run does the same
 * internally for any item whose stored category is -1 when use_classifier is set. */
int frac_classify_items(frac_ctx* ctx, frac_grid_item* items, size_t n, int target_plane);

/* ---- frame loader: colour conversion (ImageIO::rgb2yuv, image/ImageIO.cpp:43-58) ----
 * Packed RGB (w×h, rgb_stride bytes per row) → Y (w×h) and U, V (w/2 × h/2, the odd
 * pixel of each 2×2 quad), bit-exact with the built reference (FMA-contracted weights).
 * Replaces the conversion inside ImageIO::loadImage (ImageIO.cpp:60-66); the PNG decode
 * itself stays on the host.  _device: all pointers are device pointers, the work is
 * enqueued on the ctx stream (call frac_sync before reading).  The host variant uploads,
 * converts on the device and downloads. */
int frac_rgb_to_yuv_device(frac_ctx* ctx, const void* d_rgb, uint32_t w, uint32_t h, uint32_t rgb_stride, void* d_y,
                           uint32_t y_stride, void* d_u, uint32_t u_stride, void* d_v, uint32_t v_stride);
int frac_rgb_to_yuv(frac_ctx* ctx, const uint8_t* rgb, uint32_t w, uint32_t h, uint32_t rgb_stride, uint8_t* y,
                    uint8_t* u, uint8_t* v);

/* ---- frame saver: the conversion back (ImageIO::yuv2rgb, image/ImageIO.cpp:68-84, used by saveImage<3>) ----
 * These two symbols were added after ABI 9 without changing FRAC_ABI_VERSION: probe for them by name
 * (dlsym) when the library may be older.
 *
 * Y (w×h) and U, V (w/2 × h/2) → packed RGB, bit-exact with the built reference, which contracts every
 * product into its addition: with u' = u − 128, v' = v − 128, R = clamp(fma(1.402, v', y)),
 * G = clamp(fma(−0.714, v', fma(−0.344, u', y))), B = clamp(fma(1.772, u', y)).  Pixel (x, y) reads chroma
 * cell (x/2, y/2), clamped to the chroma plane's last column and row: for an odd w or h the reference reads
 * one cell past the plane (its stride padding), which is undefined here.  w and h at least 2 (a smaller frame
 * has no chroma plane: FRAC_E_INVALID, nothing launched).  Every stride is in bytes; rgb_stride too, as
 * frac_rgb_to_yuv's (the reference's own parameter counts pixels).  _device: all pointers are device
 * pointers, the work is enqueued on the ctx stream and not synchronised (call frac_sync before reading).
 * The host variant takes tight planes (strides w and w/2), uploads, converts and downloads. */
int frac_yuv_to_rgb_device(frac_ctx* ctx, const void* d_y, uint32_t w, uint32_t h, uint32_t y_stride,
                           const void* d_u, uint32_t u_stride, const void* d_v, uint32_t v_stride, void* d_rgb,
                           uint32_t rgb_stride);
int frac_yuv_to_rgb(frac_ctx* ctx, const uint8_t* y, const uint8_t* u, const uint8_t* v, uint32_t w, uint32_t h,
                    uint8_t* rgb, uint32_t rgb_stride);

/* ---- FRC1 quantized stream, packed on the device --------------------------
 * The reference has no file format; encode_data_statistics (main.cpp:106-140) builds
 * Frac::Quantizerd over the frame's (contrast, brightness) range with 5 / 7 bits
 * (main.cpp:120-121).  FRC1 (fractencode_amd/codec.py documents the layout) stores per
 * range (domain index, transform, q_contrast, q_brightness) bit-packed after a 72-byte
 * header.  This packs the last run's results into it: min/max reductions, Quantizer codes
 * (encode/Quantizer.hpp:7-45, FP64 as the reference) and the bit packing all run on the
 * device; only the finished stream is copied out.  Requires the ranges to be the
 * createUniformGrid(range_size, range_size) lattice in row-major order and the domains the
 * createUniformGrid(2·range_size, range_size) lattice (the CLI's grids, main.cpp:147-152).
 * contrast_bits, brightness_bits in [2, 16].  *n_out = stream size; writes min(cap, size)
 * bytes (out may be NULL to query the size). */
#define FRAC_FRC1_HEADER_BYTES 72
int frac_pack_frc1(frac_ctx* ctx, uint32_t contrast_bits, uint32_t brightness_bits, uint8_t* out, size_t cap,
                   size_t* n_out);

/* ---- FRC1 streams decoded on the device, at any integer scale ---------------
 * These two symbols were added after ABI 9 without changing FRAC_ABI_VERSION: probe for them by
 * name (dlsym) when the library may be older.
 *
 * The header's fields plus what follows from them.  The type is named by its struct tag (the
 * function below has the same name, which C keeps apart from tags and C++ resolves to the function). */
struct frac_frc1_info {
    uint32_t width, height, range_size, domain_size, domain_stride;
    uint32_t transforms, contrast_bits, brightness_bits, index_bits, record_bits;
    uint32_t n_ranges, n_domains, flags;
    uint64_t body_bytes;                 /* ceil(n_ranges * record_bits / 8) */
    double contrast_min, contrast_max, brightness_min, brightness_max;
};
/* Host only, no device and no ctx: parse and validate an FRC1 header against the stream length
 * (message via frac_last_error(NULL)).  FRAC_E_INVALID for: len < 72, wrong magic or version; a zero
 * width, height or range size; domain_size < 2 or odd, domain_stride != domain_size / 2; transforms
 * outside 1..8; contrast_bits or brightness_bits outside [2, 24]; index_bits != max(1, bitlen(n_domains));
 * record_bits > 64; n_ranges / n_domains other than frac_uniform_grid's counts for (range_size,
 * range_size) / (domain_size, domain_stride); len < 72 + body_bytes; a non-finite min or max.  Trailing
 * bytes are ignored. */
int frac_frc1_info(const uint8_t* stream, size_t len, struct frac_frc1_info* out);
/* Decoder2::decode of the stream's records with every coordinate and size multiplied by `scale`
 * (1..16, scale·W and scale·H at most 65535): the result of frac_decode on the stream's dequantized
 * records (Quantizer::value, a degenerate field dequantizes to its min) so scaled.
 * plane: (scale·W) × (scale·H), row stride scale·W, in/out exactly as frac_decode's plane; plane_bytes
 * is its capacity.  A record whose index equals n_domains has no domain and its range is left
 * untouched; an index above n_domains fails the call (FRAC_E_INVALID) before any plane is touched. */
int frac_decode_frc1(frac_ctx* ctx, const uint8_t* stream, size_t len, uint32_t scale, int max_iter,
                     double rms_eps, uint8_t* plane, size_t plane_bytes, int* iterations, double* rms);

/* ---- FRQ1: the quadtree's leaves as a stream, packed on the host, decoded on the device ----
 * These three symbols were added after ABI 9 without changing FRAC_ABI_VERSION: probe for them by
 * name (dlsym) when the library may be older.
 *
 * FRQ1 (fractencode_amd/codec.py documents the layout) holds, after a 64-byte header, per level of the
 * quadtree a split bitmap over the level's nodes (all but the last level) and the level's leaves as
 * (domain index, transform, q_contrast, q_brightness) records, bit-packed as FRC1's, in the order
 * frac_encode_quadtree emits them.  One quantizer pair covers the stream.
 *
 * The header's fields plus what a walk over the bitmaps derives; levels k = 0 .. levels − 1 have the sides
 * max_size >> k, entries past `levels` are 0.  Offsets are bytes from the start of the stream. */
#define FRAC_FRQ1_HEADER_BYTES 64
struct frac_frq1_info {
    uint32_t width, height, max_size, min_size;
    uint32_t transforms, contrast_bits, brightness_bits, flags;
    uint32_t n_leaves, levels;
    uint32_t nodes[4], leaves[4];     /* N_k, M_k = N_k − (split nodes) */
    uint32_t n_domains[4];            /* frac_uniform_grid(2·n_k, n_k) counts */
    uint32_t index_bits[4], record_bits[4];
    uint64_t bitmap_offset[4], record_offset[4];
    uint64_t body_bytes;
    double contrast_min, contrast_max, brightness_min, brightness_max;
};
/* Host only, no device and no ctx: parse an FRQ1 stream, walk its split bitmaps (popcounts) to find every
 * section, and validate it against the stream length (message via frac_last_error(NULL)).  FRAC_E_INVALID
 * for: len < 64; wrong magic or version; a zero width or height, or a side above 65535; max_size or
 * min_size outside {2, 4, 8, 16}, min_size > max_size; transforms outside 1..8; contrast_bits or
 * brightness_bits outside [2, 24]; a non-zero reserved byte or word; a level's record wider than 64 bits;
 * a stream that ends inside a bitmap or record section; a set padding bit in a bitmap; n_leaves other than
 * the levels' leaf count; a non-finite min or max.  Trailing bytes are ignored. */
int frac_frq1_info(const uint8_t* stream, size_t len, struct frac_frq1_info* out);
/* Host only, no ctx: n leaves of frac_encode_quadtree_leaves (its output order) of a width×height frame
 * encoded with (max_size, min_size) as an FRQ1 stream.  The leaves are on the host already and the pack is
 * one pass over them, so it runs there, in FP64 (Quantizer::quantized, encode/Quantizer.hpp:7-45).
 * stream_flags goes into the header's flags (bit 0: the classifier was on).  *n_out = stream size; writes
 * min(cap, size) bytes (out may be NULL to query the size).  FRAC_E_INVALID (message via
 * frac_last_error(NULL)) for: contrast_bits or brightness_bits outside [2, 16]; sizes or sides as
 * frac_frq1_info refuses them; transforms outside 1..8; a leaf that is not the next leaf of the canonical
 * order (a size code outside the levels, a position that is no node of its level, a leaf out of order,
 * missing or surplus); a domain index that is neither below its level's domain count nor
 * FRAC_QT_NO_DOMAIN; a transform >= transforms; a non-finite contrast or brightness. */
int frac_pack_frq1(const frac_qt_leaf* leaves, size_t n, uint32_t width, uint32_t height, uint32_t max_size,
                   uint32_t min_size, uint32_t transforms, uint32_t stream_flags, uint32_t contrast_bits,
                   uint32_t brightness_bits, uint8_t* out, size_t cap, size_t* n_out);
/* Decoder2::decode of the stream's leaves with every coordinate and size multiplied by `scale`: the result
 * of frac_decode on the stream's dequantized records so scaled.  scale, plane, plane_bytes, max_iter,
 * rms_eps, iterations and rms exactly as frac_decode_frc1's.  A leaf whose index equals its level's domain
 * count has no domain and its range is left untouched; an index above it fails the call (FRAC_E_INVALID)
 * before any plane is touched.  The layout (ranks of the split bits by a prefix sum, leaf origins, the
 * records' bit windows) is computed on the device; only the body is uploaded.  Streams with a level of
 * 2^24 or more domains are refused (as frac_qt_leaf cannot name them). */
int frac_decode_frq1(frac_ctx* ctx, const uint8_t* stream, size_t len, uint32_t scale, int max_iter,
                     double rms_eps, uint8_t* plane, size_t plane_bytes, int* iterations, double* rms);

/* ---- quadtree rate sweep: every split distance's FRQ1 size from one search ----
 * These five symbols were added after ABI 9 without changing FRAC_ABI_VERSION: probe for them by name
 * (dlsym) when the library may be older.
 *
 * The partition frac_encode_quadtree makes at ANY split distance is a function of the distances of the full
 * tree: level 0 is createUniformGrid(W, H, max_size, max_size) in row-major order, level k + 1 holds, for each
 * node of level k in order, its quadrants top-left, top-right, bottom-left, bottom-right (N_k = 4^k · N_0), and
 * the nodes a split distance reaches are a sub-sequence of it in FRQ1's canonical order.  With d(v) the distance
 * of node v's record (the search frac_encode_quadtree runs for that node at that level) and the split key
 * e(v) = min(d(v), e(parent(v))) (e = d at level 0), node v of a level above min_size is reached and split
 * under split distance t exactly when e(v) > t — the comparison frac_encode_quadtree makes, in double.  So
 * S_k(t) = #{v of level k : e(v) > t} gives the node counts N_{k+1}(t) = 4 · S_k(t), the leaf counts
 * M_k = N_k(t) − S_k(t) and the stream's size (frac_frq1_size).  The candidates are {0.0} ∪ {e(v)}: between two
 * neighbouring candidates nothing changes.
 *
 * frac_quadtree_rate_build searches the full tree of the frame set on ctx once, level by level on the device
 * (any engine; arguments, frame limits and statistics as frac_encode_quadtree_leaves'), and keeps every node's
 * leaf and the sorted keys in the context.  Like frac_encode_quadtree it ends the last run's results and consumes
 * the range list.  The rate state stays readable until the next setter (see "When results are readable"),
 * frac_run, frac_encode_quadtree / frac_encode_quadtree_leaves or frac_quadtree_rate_build; without one the three
 * readers below return FRAC_E_STATE.  The readers search nothing, leave the state and each other's answers
 * alone and ignore the tuple sink.  A frame without level-0 ranges builds an empty state: 64 bytes, no leaves,
 * fit 0.0.
 *  - _sizes: for n thresholds (any doubles: negative, +inf) the stream's bytes with these quantizer widths
 *    (each in [2, 16]), its leaf count (leaves, may be NULL) and the per-level split counts S_k (splits [n][4],
 *    may be NULL; 0 from the last level on).
 *  - _fit: the least candidate whose stream has at most max_bytes — the exact smallest split distance that fits,
 *    the minimum over the fitting candidates whether or not the size is monotone — with its size and leaf count
 *    (each pointer may be NULL).  FRAC_E_INVALID when no candidate fits; the message names the smallest size.
 *  - _leaves: the partition at split distance `split` exactly as frac_encode_quadtree_leaves returns it (order,
 *    every field), without a search.  *n_out = the leaf count; writes min(count, cap) leaves (out may be NULL to
 *    query the count).  out: host memory, or device memory, or pinned host memory the device writes directly. */
int frac_quadtree_rate_build(frac_ctx* ctx, uint32_t max_size, uint32_t min_size, frac_stats* stats);
int frac_quadtree_rate_sizes(frac_ctx* ctx, uint32_t contrast_bits, uint32_t brightness_bits, const double* split,
                             size_t n, uint64_t* bytes, uint32_t* leaves, uint32_t* splits);
int frac_quadtree_rate_fit(frac_ctx* ctx, uint32_t contrast_bits, uint32_t brightness_bits, uint64_t max_bytes,
                           double* split, uint64_t* bytes, uint32_t* leaves);
int frac_quadtree_rate_leaves(frac_ctx* ctx, double split, frac_qt_leaf* out, size_t cap, size_t* n_out);
/* Host only, no ctx (message via frac_last_error(NULL)): the size of the FRQ1 stream of a partition of a
 * width×height frame that splits splits[k] nodes of level k (k < levels − 1; later entries are not read, splits
 * may be NULL for a single level): 64 + Σ_k [k < levels − 1: 4·ceil(N_k/32)] + 4·ceil(M_k·record_bits_k/32).
 * FRAC_E_INVALID for sizes, sides, transforms or bits as frac_pack_frq1 refuses them, and for a splits[k] above
 * its level's node count. */
int frac_frq1_size(uint32_t width, uint32_t height, uint32_t max_size, uint32_t min_size, uint32_t transforms,
                   uint32_t contrast_bits, uint32_t brightness_bits, const uint32_t splits[3], uint64_t* bytes);

/* ---- FRQ1 packed on the device: from the rate state, or from a search, the leaves never on the host ----
 * These two symbols were added after ABI 9 without changing FRAC_ABI_VERSION: probe for them by name
 * (dlsym) when the library may be older.
 *
 * Both return, byte for byte, what frac_pack_frq1 makes of the same leaves with the same widths (each in
 * [2, 16], else FRAC_E_INVALID): one quantizer pair over every leaf, the domain-less ones included; a degenerate
 * field coded as 0 with min == max in the header; index == the level's domain count for FRAC_QT_NO_DOMAIN; no
 * bitmap bytes for a level without nodes; every section zero-padded to a dword; 64 bytes for a frame without
 * level-0 ranges.  The split bitmaps, the sections' offsets (at counts only the device knows), the quantizer
 * bounds, the codes and the bit-packing are computed on the device; the host receives the section table and the
 * four bounds, writes the header, and copies exactly the body's bytes.  The header's transforms and flag bit 0
 * (classifier) are the context's (the rate state's for the first call).  out is host memory, pageable or pinned;
 * *n_out = the stream's size; min(cap, size) bytes are written (out may be NULL to query the size; the second
 * call still searches).  A non-finite minimum or maximum fails the call with FRAC_E_INVALID, as
 * frac_pack_frq1's check of every leaf does.  (Where a field's extreme is a zero that occurs with both signs, the
 * header carries −0.0 as the minimum and +0.0 as the maximum, where the host packer keeps the first it met;
 * the codes are the same.)
 *  - frac_quadtree_rate_stream: the stream of the rate state's partition at `split`, i.e. of
 *    frac_quadtree_rate_leaves(split).  A rate reader: FRAC_E_STATE without a readable rate state; it searches
 *    nothing, leaves the state, the other readers' answers and a run's readable results alone, and ignores the
 *    tuple sink.
 *  - frac_encode_quadtree_stream: frac_encode_quadtree_leaves and frac_pack_frq1 in one call, with that call's
 *    arguments, frame limits and statistics; it ends the last run's results and the rate state and consumes the
 *    range list. */
int frac_quadtree_rate_stream(frac_ctx* ctx, double split, uint32_t contrast_bits, uint32_t brightness_bits,
                              uint8_t* out, size_t cap, size_t* n_out);
int frac_encode_quadtree_stream(frac_ctx* ctx, const frac_quadtree_params* qp, uint32_t contrast_bits,
                                uint32_t brightness_bits, uint8_t* out, size_t cap, size_t* n_out,
                                frac_stats* stats);

/* ---- rate–distortion-optimal partitions from the rate state ----
 * These four symbols were added after ABI 9 without changing FRAC_ABI_VERSION: probe for them by name
 * (dlsym) when the library may be older.
 *
 * A split distance splits wherever one block is bad, whether or not its children are better.  These readers
 * choose the partition of the rate state's full tree by bottom-up Lagrangian pruning instead, in exact unsigned
 * 64-bit integer arithmetic (no result depends on a summation order):
 *  - distortion of node v of level k (side n = max_size >> k): q(v) = llrint(d(v) · 64n²) with d(v) the distance
 *    of the node's frac_qt_leaf — 16 × the block's summed squared error, an exact integer below 2^32 for every
 *    record the search makes; 0 for a negative or NaN distance;
 *  - bits: a leaf of level k < levels − 1 costs rb_k + 1 (its record, frac_frq1_size's record bits for these
 *    widths, and its bitmap bit), a leaf of the last level rb_k, a split node 1;
 *  - for a multiplier lambda (0 ≤ lambda ≤ 2^32): J(v) = q(v) + lambda·rb at the last level; above it
 *    leafJ = q(v) + lambda·(rb_k + 1) and splitJ = lambda + Σ_children J(c); v splits exactly when
 *    splitJ < leafJ (a tie keeps the leaf) and J(v) is the smaller of the two;
 *  - level 0 is reached; a node is reached when its parent is reached and splits; a reached node that does not
 *    split is a leaf.  With S_k the reached, splitting nodes of level k the stream's size is frac_frq1_size's
 *    closed form; the distortion reported is Σ q over the leaves.
 * At lambda = 2^32 nothing splits (q < 2^32, a split costs at least lambda more): the smallest stream there is.
 * At lambda = 0 only the distortion counts.  The partitions nest as lambda grows.
 *
 * All four are rate readers, with frac_quadtree_rate_sizes' state rules: FRAC_E_STATE without a readable rate
 * state; they search nothing, leave the state, each other's answers and a run's readable results alone and
 * ignore the tuple sink.  Widths outside [2, 16] and a lambda above 2^32 are FRAC_E_INVALID before any launch.
 * An empty state (no level-0 ranges) gives 64 bytes, no leaves, distortion 0 and fit 0.
 *  - _sizes: for n multipliers the stream's bytes, its leaf count (leaves, may be NULL), the split counts S_k
 *    (splits [n][4], may be NULL; 0 from the last level on) and the distortion (may be NULL), all multipliers
 *    in one pass over the tree.
 *  - _fit: a lambda in [0, 2^32] whose stream has at most max_bytes and whose predecessor lambda − 1 does not fit
 *    (or lambda = 0) — the least fitting one wherever the size does not grow with lambda, which it does only
 *    where the dword padding of two sections trades a word — with its size, leaf count and distortion (each
 *    pointer may be NULL).  FRAC_E_INVALID when the stream at 2^32 is above max_bytes; the message names that
 *    smallest size.
 *  - _leaves: the partition's leaves in canonical order, every field as frac_quadtree_rate_leaves gives it for
 *    the same nodes; out, cap and n_out as there (host, device or pinned host memory).
 *  - _stream: byte for byte what frac_pack_frq1 makes of _leaves' output with these widths, packed on the device
 *    as frac_quadtree_rate_stream packs; out, cap and n_out as there. */
int frac_quadtree_rd_sizes(frac_ctx* ctx, uint32_t contrast_bits, uint32_t brightness_bits, const uint64_t* lambda,
                           size_t n, uint64_t* bytes, uint32_t* leaves, uint32_t* splits, uint64_t* distortion);
int frac_quadtree_rd_fit(frac_ctx* ctx, uint32_t contrast_bits, uint32_t brightness_bits, uint64_t max_bytes,
                         uint64_t* lambda, uint64_t* bytes, uint32_t* leaves, uint64_t* distortion);
int frac_quadtree_rd_leaves(frac_ctx* ctx, uint32_t contrast_bits, uint32_t brightness_bits, uint64_t lambda,
                            frac_qt_leaf* out, size_t cap, size_t* n_out);
int frac_quadtree_rd_stream(frac_ctx* ctx, uint64_t lambda, uint32_t contrast_bits, uint32_t brightness_bits,
                            uint8_t* out, size_t cap, size_t* n_out);

/* ---- decoded quality: the error of a stream against the frame, and the rate state steered by it ----
 * These three symbols were added after ABI 9 without changing FRAC_ABI_VERSION: probe for them by name
 * (dlsym) when the library may be older.
 *
 * The search's distances are collage errors.  These calls measure what a viewer gets: the stream decoded (after
 * quantization, iterated to convergence) against the frame set on ctx — the plane the ranges lie on, the target
 * plane when frac_set_planes gave one.  The decoded plane, the frame and the leaves stay on the device; only
 * scalars (and, when asked, the block sums) come back.  Every sum is an exact unsigned 64-bit integer.
 *
 * frac_decode_error: `stream` is an FRC1 or an FRQ1 stream, told apart by its magic, parsed and validated as
 * frac_decode_frc1 / frac_decode_frq1 do and decoded at scale 1 from a zero plane with max_iter and rms_eps as
 * there.  Its width and height must be the frame's (FRAC_E_INVALID); no frame set is FRAC_E_STATE.  With g the
 * FRC1 range_size or the FRQ1 max_size, the covered rectangle is (W − W % g) × (H − H % g) from the origin —
 * what a uniform range grid or the level-0 grid covers: *pixels is its area, *sse is Σ(decoded − frame)² over
 * it, and block_sse (may be NULL) gets the sums of its g × g blocks, row-major, (W / g)·(H / g) of them:
 * min(count, block_cap) entries are written and *n_blocks is the count.  A leaf or record without a domain leaves
 * its pixels at zero and is counted like any other.  A frame smaller than g gives pixels = sse = 0.  Every
 * output pointer may be NULL.  The frame compared is the one the next frac_run would search: the call is
 * ordered behind a pending frac_set_frame_async copy.  It returns synchronised.  It is a reader: a run's readable
 * results, the rate state and the tuple sink are left alone; only the decoder's buffers are touched.
 *
 * frac_quadtree_rate_errors and frac_quadtree_rate_quality are rate readers, with frac_quadtree_rate_sizes' state
 * rules (FRAC_E_STATE without a readable rate state; widths outside [2, 16] are FRAC_E_INVALID before any launch;
 * they search nothing and leave the state and a run's readable results alone).
 *  - _errors: for each of n split distances the stream frac_quadtree_rate_stream packs there, decoded and
 *    compared as above: sse[n], bytes[n] (the stream's size) and iterations[n], each of which may be NULL.  Every
 *    probe equals frac_decode_error of frac_quadtree_rate_stream's bytes.
 *  - _quality: a split distance whose decoded error is at most max_sse.  With c[0] < … < c[m − 1] the state's
 *    candidates {0.0} ∪ {e(v)}, E(i) the decoded sse at c[i] and meets(i) = E(i) ≤ max_sse, the rule is exactly:
 *      1. probe m − 1; if it meets, the answer is m − 1;
 *      2. otherwise, when m > 1, probe 0; if it fails (or m = 1), FRAC_E_INVALID, the message naming E(0);
 *      3. lo = 0, hi = m − 1; while hi − lo > 1: mid = lo + (hi − lo) / 2; probe mid; lo = mid if it meets,
 *         else hi = mid;
 *      4. the answer is lo.
 *    Outputs (each may be NULL): c[answer], its stream's bytes and leaves, E(answer) and the probes made.
 *    Guarantee: the answer meets the target and the next larger candidate does not, unless the answer is the
 *    largest candidate.  The decoded error is NOT monotone in the split distance, so the answer need not be the
 *    largest candidate that meets the target; a caller who needs that sweeps the candidates with _errors.
 *    An empty state (no level-0 ranges) has m = 1, E = 0: 64 bytes, no leaves, one probe. */
int frac_decode_error(frac_ctx* ctx, const uint8_t* stream, size_t len, int max_iter, double rms_eps, uint64_t* sse,
                      uint64_t* pixels, uint64_t* block_sse, size_t block_cap, size_t* n_blocks, int* iterations,
                      double* rms);
int frac_quadtree_rate_errors(frac_ctx* ctx, uint32_t contrast_bits, uint32_t brightness_bits, const double* split,
                              size_t n, int max_iter, double rms_eps, uint64_t* sse, uint64_t* bytes,
                              int* iterations);
int frac_quadtree_rate_quality(frac_ctx* ctx, uint32_t contrast_bits, uint32_t brightness_bits, uint64_t max_sse,
                               int max_iter, double rms_eps, double* split, uint64_t* bytes, uint32_t* leaves,
                               uint64_t* sse, uint32_t* probes);

/* ---- FRC3: one colour frame — the Y, U and V plane streams in one container, decoded to RGB on the device ----
 * These four symbols were added after ABI 9 without changing FRAC_ABI_VERSION: probe for them by name
 * (dlsym) when the library may be older.
 *
 * FRC3 (fractencode_amd/codec.py documents the layout) holds, after a 32-byte header with the RGB frame's
 * width and height and the three lengths, the Y, U and V plane streams in that order, each a complete FRC1
 * or FRQ1 stream (told apart by its own magic; kinds may be mixed), each zero-padded to a multiple of 8 bytes.
 * Y is width × height, U and V are (width/2) × (height/2), as frac_rgb_to_yuv makes them.
 * Offsets are bytes from the start of the container. */
#define FRAC_FRC3_HEADER_BYTES 32
struct frac_frc3_info {
    uint32_t width, height, flags;
    uint32_t kind[3];                 /* 1 = FRC1, 2 = FRQ1 */
    uint64_t offset[3], length[3];    /* each plane stream, without its padding */
    uint64_t total_bytes;             /* header, streams and padding */
};
/* Host only, no device and no ctx (message via frac_last_error(NULL)): parse and validate a container, the
 * three plane streams included.  FRAC_E_INVALID for: len < 32; wrong magic or version; non-zero flags or
 * reserved word; a width or height outside 2..65535; a plane section (padding included) that runs past len; a
 * non-zero padding byte; a plane stream that its own parser (frac_frc1_info / frac_frq1_info) refuses, or
 * whose magic is neither kind; a Y stream whose frame is not width × height; a U or V stream whose frame is
 * not (width/2) × (height/2).  Trailing bytes are ignored. */
int frac_frc3_info(const uint8_t* stream, size_t len, struct frac_frc3_info* out);
/* Host only, no ctx: the three plane streams (Y, U, V) of a width × height RGB frame as one container, refused
 * for the same reasons.  *n_out = container size; writes min(cap, size) bytes (out may be NULL to query the
 * size). */
int frac_pack_frc3(const uint8_t* const planes[3], const size_t lens[3], uint32_t width, uint32_t height,
                   uint8_t* out, size_t cap, size_t* n_out);
/* frac_decode_frc1 / frac_decode_frq1 of each plane stream at `scale` from a zero initial plane
 * (main.cpp:171-173), the three planes kept on the device, converted as frac_yuv_to_rgb_device does and only
 * the packed RGB copied out: (scale·width) × (scale·height) pixels, rows rgb_stride bytes apart
 * (>= 3·scale·width), rgb_bytes the buffer's capacity (the last row included, else FRAC_E_INVALID).  Y decodes
 * to scale·width × scale·height, U and V to scale·(width/2) × scale·(height/2): for an odd width or height
 * narrower than half the frame, where the conversion's chroma clamp applies.  scale, max_iter and rms_eps as
 * frac_decode_frc1's; iterations[k] and rms[k] (either may be NULL) are what the single-plane call reports for
 * plane k.  The container and its plane streams are validated on the host before anything is launched; a
 * record index out of range inside a plane stream fails the call before rgb is written.
 * _device: rgb is a device pointer, the conversion is enqueued on the ctx stream and not synchronised. */
int frac_decode_frc3(frac_ctx* ctx, const uint8_t* stream, size_t len, uint32_t scale, int max_iter, double rms_eps,
                     uint8_t* rgb, uint32_t rgb_stride, size_t rgb_bytes, int iterations[3], double rms[3]);
int frac_decode_frc3_device(frac_ctx* ctx, const uint8_t* stream, size_t len, uint32_t scale, int max_iter,
                            double rms_eps, void* d_rgb, uint32_t rgb_stride, size_t rgb_bytes, int iterations[3],
                            double rms[3]);

/* ---- colour quality: the RGB error of an FRC3 container, and a rate state's candidates ----
 * These three symbols were added after ABI 9 without changing FRAC_ABI_VERSION: probe for them by name
 * (dlsym) when the library may be older.
 *
 * frac_decode_error_frc3 measures what a viewer of a colour stream gets, as frac_decode_error does for one
 * plane: the container is parsed and validated as frac_frc3_info does, its three plane streams are decoded at
 * scale 1 from zero planes exactly as frac_decode_frc3 decodes them, and the decoded planes are converted pixel by
 * pixel as frac_yuv_to_rgb_device converts them and compared, in registers, with the packed RGB reference `rgb`
 * (width × height pixels, rows rgb_stride bytes apart).  No RGB plane is written and nothing decoded crosses PCIe.
 * The reference is an argument: no frame needs to be set on ctx, and any context can make the call.
 * Covered rectangle: with g_k plane k's FRC1 range_size or FRQ1 max_size, cov(w, g) = w − w % g, W and H the
 * container's width and height,
 *     rw = min(cov(W, g_Y), 2·cov(W/2, g_U), 2·cov(W/2, g_V)),  rh likewise from H,
 * the pixels from the origin that all three planes' grids cover.  *pixels = rw·rh; sse[0..2] are Σ(R − R_ref)²,
 * Σ(G − G_ref)² and Σ(B − B_ref)² over the rectangle, exact unsigned 64-bit integers.  A plane smaller than its g
 * gives pixels = 0 and all sums 0: the decode still runs (iterations and rms are reported), nothing is launched
 * for the comparison.  A record or leaf without a domain leaves its pixels at zero and is counted like any other.
 * iterations[k] and rms[k] are what frac_decode_frc3 reports for plane k.  Every output pointer may be NULL.
 * FRAC_E_INVALID, before any launch: a NULL rgb; rgb_stride < 3·W; a container that frac_frc3_info refuses; a
 * plane stream that the decoders refuse.  The call returns synchronised.  It is a reader, like frac_decode_error:
 * a run's readable results, the rate state and the tuple sink stay as they were; only the decoder's buffers and
 * the container decoder's planes are touched.
 * frac_decode_error_frc3: rgb is host memory, read up to the rectangle's last pixel and uploaded into a buffer of
 * the context.  _device: d_rgb is a device pointer, read on the ctx stream.
 *
 * frac_quadtree_rate_candidates is a rate reader, with frac_quadtree_rate_sizes' state rules (FRAC_E_STATE
 * without a readable rate state; it searches nothing and leaves the state and a run's readable results alone).
 * It returns the state's candidates {0.0} ∪ {e(v)}, ascending and distinct: the very list c[0] < … < c[m − 1]
 * that frac_quadtree_rate_quality bisects.  *n_out = m (may be NULL); min(m, cap) entries are written; out may
 * be NULL to query the count.  An empty state (no level-0 ranges) gives the single candidate 0.0. */
int frac_decode_error_frc3(frac_ctx* ctx, const uint8_t* stream, size_t len, const uint8_t* rgb, uint32_t rgb_stride,
                           int max_iter, double rms_eps, uint64_t sse[3], uint64_t* pixels, int iterations[3],
                           double rms[3]);
int frac_decode_error_frc3_device(frac_ctx* ctx, const uint8_t* stream, size_t len, const void* d_rgb,
                                  uint32_t rgb_stride, int max_iter, double rms_eps, uint64_t sse[3],
                                  uint64_t* pixels, int iterations[3], double rms[3]);
int frac_quadtree_rate_candidates(frac_ctx* ctx, double* out, size_t cap, size_t* n_out);

/* ---- inter-coded frames: a stream decoded against a reference plane ----
 * These four symbols were added after ABI 9 without changing FRAC_ABI_VERSION: probe for them by name
 * (dlsym) when the library may be older.
 *
 * A search over two planes (frac_set_planes: domains on the source plane, ranges on the target plane) gives
 * records that mean "range = s·(domain of the other plane) + o".  Packed, they are ordinary FRC1 / FRQ1 bytes: a
 * record carries no source plane, as it carries no resolution, and no header flag says how a stream is to be
 * decoded.  That is the caller's choice of call: the iterative decoders take a stream to its fixed point on one
 * plane, frac_decode_inter applies it once to a reference plane.  One application needs no convergence test and
 * puts no contractivity condition on the contrast; with the decoder's own previous output as the reference a
 * sequence is coded closed-loop, without drift.
 *
 * frac_decode_inter / frac_decode_inter_device: `stream` is an FRC1 or an FRQ1 stream, told apart by its magic,
 * parsed and validated exactly as frac_decode_frc1 / frac_decode_frq1 do; `scale` as there (1..16, the scaled
 * frame at most 65535 a side).  `ref` and `plane` are each (scale·W) × (scale·H).  The result, which is the
 * definition: `plane` is a copy of `ref`; then, for every record or leaf that has a domain, one Frac::copy —
 * clamp(trunc(fma(s, sample/4, o))) with the sampler's 2×2 integer sum and the dequantized s and o, the iterative
 * decoders' arithmetic — reads the domain patch in `ref` and writes the range in `plane`, every coordinate and
 * size multiplied by `scale`.  Pixels that no such range covers (margins, records whose index is the domain
 * count) keep the reference's value.  Ranges do not overlap, so the order does not matter.  There is one pass:
 * no iterations or rms outputs.
 * The host variant takes tight planes (row stride scale·W), stages them in buffers of the context and returns
 * synchronised.  In the device variant the planes are read and written in place, every stride is in bytes and at
 * least scale·W, and plane_bytes covers the last row (plane_stride·(scale·H − 1) + scale·W); no byte between
 * the rows of d_plane or after its last row is written.  The call is ordered on the ctx stream; it may block for
 * the record pass's status word, as frac_decode_frc1 does, and does not wait for the pixel pass.
 * FRAC_E_INVALID, with no byte of `plane` written: everything the iterative decoders refuse (a record index above
 * its domain count included: the record or layout pass finds it before any plane write); a NULL ref or plane; a
 * stride below scale·W; plane_bytes too small; device ref and plane whose byte spans overlap (an apply in place
 * would read what it wrote; a plane's span runs from its first byte to its last row's end, stride·(scale·H − 1) +
 * scale·W bytes, the bytes between its rows included: two strided views that interleave in one buffer, such as its
 * left and right halves, are refused although they share no pixel); a device reference plane whose span exceeds
 * 2^32 bytes (the pixel pass addresses the reference with 32-bit offsets).
 * The calls are readers, like frac_decode_error: a run's readable results, the rate state and the tuple sink stay
 * as they were, no frame needs to be set, only the decoder's buffers are touched.
 *
 * frac_inter_error: the stream applied at scale 1 to the context's source plane (the plane the domains lie on) and
 * compared with the plane the ranges lie on: the target plane of frac_set_planes, or the same plane after
 * frac_set_frame — the exact post-quantization error of a two-plane stream, or the quantized collage error of an
 * ordinary one.  The covered rectangle and *pixels are frac_decode_error's: (W − W % g) × (H − H % g) with g the
 * FRC1 range_size or the FRQ1 max_size; *sse is the exact unsigned 64-bit Σ(applied − frame)² over it; pixels
 * left at the reference's value are counted like any other.  FRAC_E_STATE without planes; FRAC_E_INVALID when the
 * stream's frame is not both planes' size, and for every stream frac_decode_inter refuses.  Returns synchronised;
 * a reader, ordered behind a pending frac_set_frame_async copy as frac_decode_error is.  Either output may be
 * NULL.  Where the ranges or leaves tile the frame, each with a domain of twice its side, no plane is written:
 * the pass compares in registers.
 *
 * frac_set_planes_device: frac_set_planes with both planes already in device memory (strides in bytes), copied
 * device to device as frac_set_frame_device copies one; d_tgt NULL or equal to d_src is frac_set_frame_device.  A
 * setter: it ends the last run's results and the rate state; a failed argument check changes nothing.  It blocks
 * until the copies are done. */
int frac_decode_inter(frac_ctx* ctx, const uint8_t* stream, size_t len, uint32_t scale, const uint8_t* ref,
                      uint8_t* plane, size_t plane_bytes);
int frac_decode_inter_device(frac_ctx* ctx, const uint8_t* stream, size_t len, uint32_t scale, const void* d_ref,
                             uint32_t ref_stride, void* d_plane, uint32_t plane_stride, size_t plane_bytes);
int frac_inter_error(frac_ctx* ctx, const uint8_t* stream, size_t len, uint64_t* sse, uint64_t* pixels);
int frac_set_planes_device(frac_ctx* ctx, const void* d_src, uint32_t sw, uint32_t sh, uint32_t sstride,
                           const void* d_tgt, uint32_t tw, uint32_t th, uint32_t tstride);

/* ---- host helpers (no device needed) ------------------------------------ */
/* createUniformGrid (image/partition2.hpp:109-135): returns the item count and
 * writes min(count, cap) items (categories -1).  Returns 0 where the reference's loop has no
 * meaningful grid: a zero size or offset (it never ends) or an item larger than the plane (its
 * do-while emits one item outside the plane, which every search entry refuses). */
size_t frac_uniform_grid(uint32_t width, uint32_t height, uint32_t item_size, uint32_t item_offset,
                         frac_grid_item* out, size_t cap);
/* The same with createUniformGrid's Size32u item size and offset (partition2.hpp:110-113): items
 * size_w × size_h, x stepping by off_x, rows by off_y (e.g. tests/OpenCLTest.cpp:76-78's 4×4 items
 * at offset (4, 2)). */
size_t frac_uniform_grid2(uint32_t width, uint32_t height, uint32_t size_w, uint32_t size_h, uint32_t off_x,
                          uint32_t off_y, frac_grid_item* out, size_t cap);
/* BrightnessBlocksClassifier2::preclassify over items (encode/Classifier2.cpp:64-68):
 * writes each item's category computed on `plane`. */
int frac_classify(const uint8_t* plane, uint32_t w, uint32_t h, uint32_t stride, frac_grid_item* items, size_t n);
/* The ratio-2 sample permutation the kernels use: range pixel pix = y·n + x under
 * transform t meets decimated domain cell frac_transform_index(n, t, pix)
 * (image/sampler.h:21-38 with image/transform.h:96-109).  −1 on bad arguments. */
int frac_transform_index(uint32_t n, uint32_t t, uint32_t pix);
/* Largest integer S16 = 16·Σ(r − d̄)² whose reference distance (S16/16)/(4n²) is
 * <= rms_threshold, or −1 (TransformMatcher::checkDistance, transformmatcher.h:32-34). */
int64_t frac_hit_limit(double rms_threshold, uint32_t n);

/* ---- test hooks (outside the ABI contract) ------------------------------ */
/* Not part of the ABI: these exist for the test suite, may change or go without a new FRAC_ABI_VERSION, and
 * a caller outside it probes for them by name.
 * frac_debug_sort_pairs runs the tiled SEA form's stable sort (csrc/fracenc_tpsort.hip) on host arrays: the
 * (key, value) pairs of two sides, n and n_b of them (either may be 0), go through the same launches on the
 * current device and come back sorted by the low `bits` key bits (1..32), equal keys in input order.
 * frac_debug_sort_chunk is the sort's items per workgroup.
 * frac_debug_resolve_group is the number of consecutive ranges (or slots) one workgroup of the tiled form's
 * grouped resolve takes (csrc/fracenc_dft.hip, resolve_dft_groups). */
uint32_t frac_debug_sort_chunk(void);
uint32_t frac_debug_resolve_group(void);
int frac_debug_sort_pairs(const uint32_t* keys, const uint32_t* vals, uint32_t n, const uint32_t* keys_b,
                          const uint32_t* vals_b, uint32_t n_b, uint32_t bits, uint32_t* out_keys,
                          uint32_t* out_vals, uint32_t* out_keys_b, uint32_t* out_vals_b);
/* frac_debug_bucket_keys computes the classifier bucket keys (category + 1; a stored category other than -1 is
 * passed through) of nd domains on the context's source plane and nr ranges on its target plane, as a classified
 * run does before it sorts its pool (csrc/fracenc_bucket.hip).  path: 0 the run's own choice of kernels, 1 the
 * row kernels grid by grid (one wave per item above 64 rows), 2 the paired launch, 3 the planes' block sums.
 * FRAC_E_INVALID, before any launch: no frame set, an item outside its plane, a category outside -1..5, or, where
 * the row kernels run, a grid of more than one item size.  It changes nothing another call reads.
 * frac_debug_bucket_sort runs the stable bucket sort on two host key arrays (keys 0..7, either side may be
 * empty), both through the same launches: dn_* is a count the kernels read from device memory (only the first
 * min(dn, n) keys are sorted) or UINT32_MAX for none; order_* [n] is filled with 0xffffffff before the sort and
 * receives the sorted indices, first_* [9] the first sorted position of each key and the count.
 * frac_debug_bucket_tile is the sort's items per workgroup, frac_debug_bucket_self_tiles the most tiles of a
 * sort that runs without the separate scan launch. */
uint32_t frac_debug_bucket_tile(void);
uint32_t frac_debug_bucket_self_tiles(void);
/* frac_debug_frame_twin_bytes is the capacity of the second plane buffers the overlapped uploads of
 * frac_set_frame / frac_set_planes / frac_set_frame_async use (0: none allocated); frac_debug_frame_copy_stream
 * is 1 once the context has created its copy stream. */
uint64_t frac_debug_frame_twin_bytes(const frac_ctx* ctx);
int frac_debug_frame_copy_stream(const frac_ctx* ctx);
int frac_debug_bucket_keys(frac_ctx* ctx, const frac_grid_item* doms, uint32_t nd, const frac_grid_item* rngs,
                           uint32_t nr, int path, uint32_t* dom_keys, uint32_t* rng_keys);
int frac_debug_bucket_sort(const uint32_t* keys_a, uint32_t na, uint32_t dn_a, const uint32_t* keys_b, uint32_t nb,
                           uint32_t dn_b, uint32_t* order_a, uint32_t* first_a, uint32_t* order_b,
                           uint32_t* first_b);

#ifdef __cplusplus
}
#endif

#endif /* FRACENC_H */
