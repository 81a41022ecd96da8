// fracenc_api.hip — C ABI (include/fracenc.h), the one translation unit of the library: it includes the
// kernel files and the host layer's other files, and holds contexts, parameters, frames, grids, runs,
// fetches, tuples, streams and the host-only helpers.
//   fracenc_ctx.h        the resource owners, frac_ctx, error macros, timing events, parameter checks
//   fracenc_plan.hip     validation, device bucketing, prepare(): work lists and buffers per engine
//   fracenc_launch.hip   variant selection, the engines' launch paths, the fp32 fallback
//   fracenc_quadtree.hip quadtree frames, host- and device-planned
//   fracenc_codec.hip    decode, FRC1 and FRQ1 pack / parse / decode, inter-frame decode, colour conversion
//   fracenc_qtrate.hip   quadtree rate sweep: the full tree searched once, sizes, fit and leaves per threshold
//   fracenc_qtrd.hip     rate–distortion-optimal partitions of that tree: sizes, fit, leaves and stream per multiplier
//   fracenc_quality.hip  decoded error of a stream against the frame; the rate state's errors and quality fit;
//                        the error of a stream applied once to the other plane
//
// Host logic mirrored from the reference:
//   classifier gating      encode/Classifier2.cpp:8-81   (categories computed on the host,
//                          a stored −1 re-computed on the item's own plane like compare())
//   rejected-mapping count encode/TransformEstimator2.hpp:43-45,59 (derived from the winner)
//   search order / ties    encode/TransformEstimator2.hpp:29-48
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "fracenc_common.h"
#include "fracenc_kernels.hip"
#include "fracenc_mfma.hip"
#include "fracenc_dft.hip"
#include "fracenc_decode.hip"
#include "fracenc_color.hip"
#include "fracenc_classify.hip"
#include "fracenc_sea.hip"
#include "fracenc_stream.hip"
#include "fracenc_frc1dec.hip"
#include "fracenc_frq1dec.hip"
#include "fracenc_inter.hip"
#include "fracenc_tp.hip"
#include "fracenc_tpsort.hip"
#include "fracenc_gen.hip"
#include "fracenc_bucket.hip"

using namespace fracenc;

#include "fracenc_ctx.h"
#include "fracenc_plan.hip"
#include "fracenc_launch.hip"
#include "fracenc_quadtree.hip"
#include "fracenc_codec.hip"
#include "fracenc_qtrate.hip"
#include "fracenc_frq1pack.hip"
#include "fracenc_qtrd.hip"
#include "fracenc_quality.hip"

namespace {

struct HostPlane {
    std::vector<uint8_t> data; // tightly packed, stride == w
    uint32_t w = 0, h = 0;
};

// --- classifier (host) -------------------------------------------------------
// ImageStatistics2::sum (image/ImageStatistics.hpp:12-17): u16 up to 16 wide.
double block_sum(const HostPlane& p, uint32_t x, uint32_t y, uint32_t w, uint32_t h)
{
    uint32_t s = 0;
    for (uint32_t j = 0; j < h; ++j) {
        const uint8_t* row = p.data.data() + (size_t)(y + j) * p.w + x;
        for (uint32_t i = 0; i < w; ++i)
            s += row[i];
    }
    return w <= 16 ? (double)(uint16_t)s : (double)s;
}

// BrightnessBlocksClassifier2::getCategory(a1..a4) — encode/Classifier2.cpp:8-62
int category4(double a1, double a2, double a3, double a4)
{
    // rule (i, j, k): a_i > a_j && a_j > a_k && a_k > a_l, listed as quadruples (i j k l)
    static const unsigned char rules[24][4] = {
        {1, 2, 3, 4}, {3, 1, 4, 2}, {4, 3, 2, 1}, {2, 4, 1, 3}, // 0
        {1, 3, 2, 4}, {2, 1, 4, 3}, {4, 2, 3, 1}, {3, 4, 1, 2}, // 1
        {1, 4, 3, 2}, {4, 1, 2, 3}, {3, 2, 4, 1}, {2, 3, 1, 4}, // 2
        {1, 2, 4, 3}, {3, 1, 2, 4}, {4, 3, 1, 2}, {2, 4, 3, 1}, // 3
        {2, 1, 3, 4}, {1, 3, 4, 2}, {3, 4, 2, 1}, {4, 2, 1, 3}, // 4
        {1, 4, 2, 3}, {4, 1, 3, 4}, {2, 3, 4, 1}, {3, 2, 1, 4}, // 5
    };
    const double a[5] = {0.0, a1, a2, a3, a4};
    for (int r = 0; r < 24; ++r) {
        const unsigned char* q = rules[r];
        if (a[q[0]] > a[q[1]] && a[q[1]] > a[q[2]] && a[q[2]] > a[q[3]])
            return r / 4;
    }
    return -1;
}

int category(const HostPlane& p, const frac_grid_item& it)
{
    const uint32_t hw = it.w / 2, hh = it.h / 2;
    return category4(block_sum(p, it.x, it.y, hw, hh), block_sum(p, it.x + hw, it.y, hw, hh),
                     block_sum(p, it.x, it.y + hh, hw, hh), block_sum(p, it.x + hw, it.y + hh, hw, hh));
}

// Categories of items[list[k]] on the device plane (classify_items); synchronous.
int classify_on_device(frac_ctx* c, const std::vector<frac_grid_item>& items, const std::vector<uint32_t>& list,
                       const uint8_t* dplane, uint32_t dstride, std::vector<int32_t>& out)
{
    out.assign(list.size(), -1);
    if (list.empty())
        return FRAC_OK;
    HostTrace tr("classify");
    FRAC_HIP(c, c->d_cls_out.ensure(list.size()));
    FRAC_TRY(upload(c, c->d_cls_items, items));
    FRAC_TRY(upload(c, c->d_cls_list, list));
    ClassifyArgs a;
    a.plane = dplane;
    a.stride = dstride;
    a.items = c->d_cls_items.ptr;
    a.list = c->d_cls_list.ptr;
    a.n = (uint32_t)list.size();
    a.out = c->d_cls_out.ptr;
    tr.mark("alloc + H2D");
    classify_items<<<(unsigned)((list.size() + 3) / 4), 256, 0, c->stream>>>(a);
    FRAC_HIP(c, hipGetLastError());
    tr.mark("launch");
    FRAC_HIP(c, hipMemcpyAsync(out.data(), c->d_cls_out.ptr, list.size() * sizeof(int32_t), hipMemcpyDeviceToHost,
                               c->stream));
    FRAC_HIP(c, hipStreamSynchronize(c->stream));
    tr.mark("D2H + sync");
    return FRAC_OK;
}

// one host plane of an upload: the caller's memory, the buffer the runs read, its twin and its pitch
struct PlaneUpload {
    const uint8_t* p;
    uint32_t w, h, stride;
    DBuf<uint8_t>* cur;
    DBuf<uint8_t>* next;
    uint32_t* dstride;
};

// both of the context's streams idle: before a plane buffer or a twin is (re)allocated, nothing may still
// read or write the one that goes
int planes_idle(frac_ctx* c)
{
    FRAC_HIP(c, hipStreamSynchronize(c->stream));
    if (c->frame.copy_stream)
        FRAC_HIP(c, hipStreamSynchronize(c->frame.copy_stream));
    return FRAC_OK;
}

// The caller's planes (the source, or source and target: `same`) straight to the device, for the blocking
// setters (wait: the planes have been consumed, and may be overwritten, when the call returns) and for
// frac_set_frame_async (no wait).  The first planes of a geometry go into the current buffers on the context's
// stream, behind everything it holds.  Planes that follow others of their geometry go into the twins on the
// copy stream (frac_ctx::FrameStream has the ordering) while the runs already enqueued go on: the host then
// waits for the copies alone.  On an error the current planes, their pitches and the context's flags are as
// they were: nothing swaps before every copy has been enqueued.
int upload_planes(frac_ctx* c, const PlaneUpload* up, int n, bool same, bool wait)
{
    FRAC_TRY(settle_fallback(c)); // the last run's fp32-regime ranges read the current planes: before any swap
    auto& f = c->frame;
    uint32_t pitch[2] = {0, 0};
    size_t need[2] = {0, 0};
    for (int k = 0; k < n; ++k) {
        pitch[k] = plane_pitch(up[k].w);
        // one extra row + column of slack: kernels never read it, but keeps every 2×2 read in-bounds
        need[k] = (size_t)pitch[k] * (up[k].h + 1);
    }
    bool twin = c->planes_set && c->same_plane == same && c->src.w == up[0].w && c->src.h == up[0].h;
    if (twin && !same)
        twin = c->tgt.w == up[1].w && c->tgt.h == up[1].h;
    if (!twin) {
        bool grow = false;
        for (int k = 0; k < n; ++k)
            grow = grow || !up[k].cur->ptr || up[k].cur->cap < need[k];
        if (grow)
            FRAC_TRY(planes_idle(c));
        for (int k = 0; k < n; ++k)
            FRAC_HIP(c, up[k].cur->ensure(need[k]));
        for (int k = 0; k < n; ++k)
            FRAC_TRY(copy_plane(c, up[k].cur->ptr, pitch[k], up[k].p, up[k].stride, up[k].w, up[k].h,
                                hipMemcpyHostToDevice, c->stream));
        if (wait)
            FRAC_HIP(c, hipStreamSynchronize(c->stream));
        for (int k = 0; k < n; ++k)
            *up[k].dstride = pitch[k];
        return FRAC_OK;
    }
    if (!f.copy_stream) {
        FRAC_HIP(c, hipStreamCreateWithFlags(&f.copy_stream.s, hipStreamNonBlocking));
        FRAC_HIP(c, hipEventCreateWithFlags(&f.up_done.e, hipEventDisableTiming));
        FRAC_HIP(c, hipEventCreateWithFlags(&f.next_free.e, hipEventDisableTiming));
    }
    bool grow = false;
    for (int k = 0; k < n; ++k)
        grow = grow || !up[k].next->ptr || up[k].next->cap < need[k];
    if (grow) { // an earlier upload may still write, an earlier run still read, the twin that goes
        FRAC_TRY(planes_idle(c));
        for (int k = 0; k < n; ++k)
            FRAC_HIP(c, up[k].next->ensure(need[k]));
    }
    if (f.next_free_recorded) // the runs that read the twins before the last swap are done
        FRAC_HIP(c, hipStreamWaitEvent(f.copy_stream, f.next_free, 0));
    for (int k = 0; k < n; ++k) {
        const int rc = copy_plane(c, up[k].next->ptr, pitch[k], up[k].p, up[k].stride, up[k].w, up[k].h,
                                  hipMemcpyHostToDevice, f.copy_stream);
        if (rc != FRAC_OK) { // no copy of this call may still read the caller's planes after it returned
            (void)hipStreamSynchronize(f.copy_stream);
            return rc;
        }
    }
    FRAC_HIP(c, hipEventRecord(f.up_done, f.copy_stream));
    FRAC_HIP(c, hipStreamWaitEvent(c->stream, f.up_done, 0));
    for (int k = 0; k < n; ++k) {
        std::swap(*up[k].cur, *up[k].next);
        *up[k].dstride = pitch[k];
    }
    // the planes now in the twins are free once everything the context enqueued so far has run
    FRAC_HIP(c, hipEventRecord(f.next_free, c->stream));
    f.next_free_recorded = true;
    if (wait)
        FRAC_HIP(c, hipEventSynchronize(f.up_done));
    return FRAC_OK;
}

} // namespace

extern "C" {

int frac_abi_version(void) { return FRAC_ABI_VERSION; }

int frac_device_count(void)
{
    int count = 0;
    const hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess) {
        g_last_error = std::string("hipGetDeviceCount: ") + hipGetErrorString(e);
        return FRAC_E_DEVICE;
    }
    return count;
}

// The source id build() compiles in (-DFRAC_SOURCE_ID="…": the hash fractencode_amd.source_id()
// computes over csrc/ and include/fracenc.h), so a result can name the binary that produced it.
#ifndef FRAC_SOURCE_ID
#define FRAC_SOURCE_ID "unknown"
#endif
const char* frac_build_id(void) { return FRAC_SOURCE_ID; }

int frac_build_flags(void) { return kTuningBuild ? FRAC_BUILD_TUNING : 0; }

const char* frac_last_error(const frac_ctx* ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }

uint32_t frac_debug_sort_chunk(void) { return kTpSortChunk; }

uint32_t frac_debug_resolve_group(void) { return kTpGrpItems; }

// Test hook: what the context holds for overlapped uploads (frac_ctx::FrameStream): the twins' bytes, and
// whether the copy stream exists.
uint64_t frac_debug_frame_twin_bytes(const frac_ctx* c)
{
    return c ? (uint64_t)c->frame.d_src_next.cap + c->frame.d_tgt_next.cap : 0;
}

int frac_debug_frame_copy_stream(const frac_ctx* c) { return c && c->frame.copy_stream ? 1 : 0; }

// Test hook: the tiled form's sort (tp_sort_pairs) on host arrays, both sides through the same launches on the
// current device's null stream, then a synchronous copy back.
int frac_debug_sort_pairs(const uint32_t* keys, const uint32_t* vals, uint32_t n, const uint32_t* keys_b,
                          const uint32_t* vals_b, uint32_t n_b, uint32_t bits, uint32_t* out_keys, uint32_t* out_vals,
                          uint32_t* out_keys_b, uint32_t* out_vals_b)
{
    auto bad = [](const std::string& m, int code) {
        g_last_error = m;
        return code;
    };
    if (bits == 0 || bits > 32)
        return bad("frac_debug_sort_pairs: bits must be 1..32", FRAC_E_INVALID);
    if ((n && !(keys && vals && out_keys && out_vals)) || (n_b && !(keys_b && vals_b && out_keys_b && out_vals_b)))
        return bad("frac_debug_sort_pairs: NULL array", FRAC_E_INVALID);
    DBuf<uint32_t> d[2][4], table; // per side: key, val, key2, val2
    const uint32_t* in[2][2] = {{keys, vals}, {keys_b, vals_b}};
    uint32_t* out[2][2] = {{out_keys, out_vals}, {out_keys_b, out_vals_b}};
    const uint32_t cnt[2] = {n, n_b};
    hipError_t e = table.ensure(tp_sort_table_words(n, n_b));
    for (int s = 0; s < 2 && e == hipSuccess; ++s) {
        for (int k = 0; k < 4 && e == hipSuccess; ++k)
            e = d[s][k].ensure(cnt[s]);
        for (int k = 0; k < 2 && e == hipSuccess && cnt[s]; ++k)
            e = hipMemcpy(d[s][k].ptr, in[s][k], (size_t)cnt[s] * sizeof(uint32_t), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess)
        e = tp_sort_pairs(table.ptr, TpSortBufs{d[0][0].ptr, d[0][1].ptr, d[0][2].ptr, d[0][3].ptr, n},
                          TpSortBufs{d[1][0].ptr, d[1][1].ptr, d[1][2].ptr, d[1][3].ptr, n_b}, bits, nullptr);
    const int from = tp_sort_in_second(bits) ? 2 : 0;
    for (int s = 0; s < 2 && e == hipSuccess; ++s)
        for (int k = 0; k < 2 && e == hipSuccess && cnt[s]; ++k)
            e = hipMemcpy(out[s][k], d[s][from + k].ptr, (size_t)cnt[s] * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess)
        return bad(std::string("frac_debug_sort_pairs: ") + hipGetErrorString(e), FRAC_E_DEVICE);
    return FRAC_OK;
}

uint32_t frac_debug_bucket_tile(void) { return kBkTile; }
uint32_t frac_debug_bucket_self_tiles(void) { return kBkSelfTiles; }

// Test hook: the classifier keys of two host item arrays by the key kernels of fracenc_bucket.hip, the domains on
// the context's source plane and the ranges on its target plane.  Everything is checked on the host before the
// first launch; the items and keys live in buffers of the call's own, so the context's prepared state stays as
// it is (the planes' block sums are scratch that every run rebuilds).
int frac_debug_bucket_keys(frac_ctx* c, const frac_grid_item* doms, uint32_t nd, const frac_grid_item* rngs, uint32_t nr,
                           int path, uint32_t* dom_keys, uint32_t* rng_keys)
{
    if (!c)
        return FRAC_E_INVALID;
    if (!c->planes_set)
        return c->fail(FRAC_E_INVALID, "debug_bucket_keys: no frame set");
    if (path < 0 || path > 3)
        return c->fail(FRAC_E_INVALID, "debug_bucket_keys: path must be 0..3");
    if ((nd && !(doms && dom_keys)) || (nr && !(rngs && rng_keys)))
        return c->fail(FRAC_E_INVALID, "debug_bucket_keys: NULL array");
    const frac_grid_item* items[2] = {doms, rngs};
    const uint32_t cnt[2] = {nd, nr};
    const frac_ctx::PlaneSize size[2] = {c->src, c->same_plane ? c->src : c->tgt};
    uint32_t w[2] = {0, 0}, h[2] = {0, 0}; // the grids' item sizes: the first item's
    bool one_size = true;
    for (int s = 0; s < 2; ++s) {
        if (cnt[s]) {
            w[s] = items[s][0].w;
            h[s] = items[s][0].h;
        }
        for (uint32_t i = 0; i < cnt[s]; ++i) {
            const frac_grid_item& it = items[s][i];
            if ((uint64_t)it.x + it.w > size[s].w || (uint64_t)it.y + it.h > size[s].h)
                return c->fail(FRAC_E_INVALID, "debug_bucket_keys: item outside the plane");
            if (it.category < -1 || it.category > 5)
                return c->fail(FRAC_E_INVALID, "item category outside -1..5");
            one_size = one_size && it.w == w[s] && it.h == h[s];
        }
    }
    const bool sums = path == 3 || (path == 0 && w[0] <= 32 && h[0] <= 32 && w[1] <= 32 && h[1] <= 32);
    if (!sums && !one_size) // the row kernels size their lane groups by the grid's first item
        return c->fail(FRAC_E_INVALID, "debug_bucket_keys: a grid of more than one item size");
    FRAC_HIP(c, hipSetDevice(c->device));
    DBuf<frac_grid_item> d_items[2];
    DBuf<uint32_t> d_keys[2], d_err;
    FRAC_HIP(c, d_err.ensure(1));
    FRAC_HIP(c, hipMemsetAsync(d_err.ptr, 0, sizeof(uint32_t), c->stream));
    for (int s = 0; s < 2; ++s) {
        FRAC_HIP(c, d_items[s].ensure(cnt[s]));
        FRAC_HIP(c, d_keys[s].ensure(cnt[s]));
        if (cnt[s])
            FRAC_HIP(c, hipMemcpyAsync(d_items[s].ptr, items[s], (size_t)cnt[s] * sizeof(frac_grid_item),
                                       hipMemcpyHostToDevice, c->stream));
    }
    int rc = FRAC_OK;
    hipError_t e = hipSuccess;
    {
        const auto [tplane, tstride] = target_plane(c);
        const KeySeg kd{d_items[0].ptr, nd, c->d_src.ptr, c->d_sstride, d_keys[0].ptr, nullptr, d_err.ptr, nullptr};
        const KeySeg kr{d_items[1].ptr, nr, tplane, tstride, d_keys[1].ptr, nullptr, d_err.ptr, nullptr};
        if (path == 0) {
            rc = launch_grid_keys(c, kd, w[0], h[0], kr, w[1], h[1]);
        } else if (path == 1) {
            if (nd)
                launch_bucket_keys(kd.items, nd, h[0], kd.plane, kd.stride, kd.key, nullptr, kd.err, c->stream);
            if (nr)
                launch_bucket_keys(kr.items, nr, h[1], kr.plane, kr.stride, kr.key, nullptr, kr.err, c->stream);
        } else if (path == 2) {
            launch_bucket_keys_pair(kd, h[0], kr, h[1], c->stream);
        } else {
            BlockSums bs, bt;
            rc = plane_block_sums(c, bs, bt);
            if (rc == FRAC_OK)
                launch_bucket_keys_bs(kd, bs, w[0], h[0], kr, bt, w[1], h[1], c->stream);
        }
        if (rc == FRAC_OK)
            e = hipGetLastError();
        uint32_t err = 0;
        uint32_t* out[2] = {dom_keys, rng_keys};
        for (int s = 0; s < 2 && rc == FRAC_OK && e == hipSuccess; ++s)
            if (cnt[s])
                e = hipMemcpyAsync(out[s], d_keys[s].ptr, (size_t)cnt[s] * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                   c->stream);
        if (rc == FRAC_OK && e == hipSuccess)
            e = hipMemcpyAsync(&err, d_err.ptr, sizeof(err), hipMemcpyDeviceToHost, c->stream);
        // the call's buffers go when it returns: the stream is idle by then, whatever happened above
        const hipError_t es = hipStreamSynchronize(c->stream);
        if (rc != FRAC_OK)
            return rc;
        FRAC_HIP(c, e);
        FRAC_HIP(c, es);
        if (err)
            return c->fail(FRAC_E_INVALID, "item category outside -1..5");
    }
    return FRAC_OK;
}

// Test hook: the stable bucket sort (launch_bucket_sorts) of two host key arrays, both sides through the same
// launches on the current device's null stream.  dn: a device-side count (UINT32_MAX: none).  The orders are
// filled with 0xffffffff first, so the positions the sort did not write show.
int frac_debug_bucket_sort(const uint32_t* keys_a, uint32_t na, uint32_t dn_a, const uint32_t* keys_b, uint32_t nb,
                           uint32_t dn_b, uint32_t* order_a, uint32_t* first_a, uint32_t* order_b, uint32_t* first_b)
{
    auto bad = [](const std::string& m, int code) {
        g_last_error = m;
        return code;
    };
    const uint32_t* in[2] = {keys_a, keys_b};
    uint32_t* order[2] = {order_a, order_b};
    uint32_t* first[2] = {first_a, first_b};
    const uint32_t cnt[2] = {na, nb}, dn[2] = {dn_a, dn_b};
    for (int s = 0; s < 2; ++s) {
        if (!first[s] || (cnt[s] && !(in[s] && order[s])))
            return bad("frac_debug_bucket_sort: NULL array", FRAC_E_INVALID);
        for (uint32_t i = 0; i < cnt[s]; ++i)
            if (in[s][i] >= (uint32_t)kMaxBuckets)
                return bad("frac_debug_bucket_sort: key outside 0..7", FRAC_E_INVALID);
    }
    DBuf<uint32_t> d_keys[2], d_out[2], d_cnt, d_first, d_dn;
    const uint32_t tiles[2] = {std::max<uint32_t>((na + kBkTile - 1) / kBkTile, 1u),
                               std::max<uint32_t>((nb + kBkTile - 1) / kBkTile, 1u)};
    hipError_t e = d_cnt.ensure((size_t)(tiles[0] + tiles[1]) * kMaxBuckets);
    if (e == hipSuccess)
        e = d_first.ensure(2 * (kMaxBuckets + 1));
    if (e == hipSuccess)
        e = d_dn.ensure(2);
    if (e == hipSuccess)
        e = hipMemcpy(d_dn.ptr, dn, sizeof(dn), hipMemcpyHostToDevice);
    for (int s = 0; s < 2 && e == hipSuccess; ++s) {
        e = d_keys[s].ensure(cnt[s]);
        if (e == hipSuccess)
            e = d_out[s].ensure(cnt[s]);
        if (e == hipSuccess && cnt[s])
            e = hipMemcpy(d_keys[s].ptr, in[s], (size_t)cnt[s] * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMemset(d_out[s].ptr, 0xff, std::max<size_t>(cnt[s], 1) * sizeof(uint32_t));
    }
    if (e == hipSuccess) {
        const BkSeg sa = bk_seg_of(d_keys[0].ptr, na, dn_a == UINT32_MAX ? nullptr : d_dn.ptr, d_cnt.ptr, d_first.ptr,
                                   d_out[0].ptr);
        const BkSeg sb = bk_seg_of(d_keys[1].ptr, nb, dn_b == UINT32_MAX ? nullptr : d_dn.ptr + 1,
                                   d_cnt.ptr + (size_t)sa.tiles * kMaxBuckets, d_first.ptr + kMaxBuckets + 1,
                                   d_out[1].ptr);
        launch_bucket_sorts(sa, sb, nullptr);
        e = hipGetLastError();
    }
    for (int s = 0; s < 2 && e == hipSuccess; ++s) {
        e = hipMemcpy(first[s], d_first.ptr + s * (kMaxBuckets + 1), (kMaxBuckets + 1) * sizeof(uint32_t),
                      hipMemcpyDeviceToHost);
        if (e == hipSuccess && cnt[s])
            e = hipMemcpy(order[s], d_out[s].ptr, (size_t)cnt[s] * sizeof(uint32_t), hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) {
        (void)hipDeviceSynchronize(); // nothing may still run on the buffers that go with this call
        return bad(std::string("frac_debug_bucket_sort: ") + hipGetErrorString(e), FRAC_E_DEVICE);
    }
    return FRAC_OK;
}

frac_ctx* frac_create(int device, const frac_params* params)
{
    std::string msg;
    if (check_params(params, msg) != FRAC_OK) {
        g_last_error = msg;
        return nullptr;
    }
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0) {
        g_last_error = std::string("no HIP device: ") + hipGetErrorString(e);
        return nullptr;
    }
    if (device < 0 || device >= count) {
        g_last_error = "device index out of range";
        return nullptr;
    }
    e = hipSetDevice(device);
    if (e != hipSuccess) {
        g_last_error = std::string("hipSetDevice: ") + hipGetErrorString(e);
        return nullptr;
    }
    auto* c = new frac_ctx();
    c->device = device;
    c->p = *params;
    if (hipStreamCreateWithFlags(&c->own_stream.s, hipStreamNonBlocking) != hipSuccess) {
        g_last_error = "hipStreamCreate failed";
        delete c;
        return nullptr;
    }
    c->stream = c->own_stream;
    for (size_t k = 0; k < 5; ++k)
        if ((k < 4 ? create_timing_event(&c->ev[k].e, k) : hipEventCreate(&c->ev[k].e)) != hipSuccess) {
            g_last_error = "hipEventCreate failed";
            delete c;
            return nullptr;
        }
    return c;
}

void frac_destroy(frac_ctx* c) { delete c; } // ~frac_ctx: idle first, then every member frees itself

// A change of parameters, domains or ranges ends the last run's results: until the next frac_run every reader
// refuses them (FRAC_E_STATE) rather than pair the old winners with the new parameters or lists.  The run's
// unsettled fp32 fallback goes with them: nothing may read its records any more, and its saved arguments
// name buffers the next prepare() may reallocate.  (The plane setters clear `ran` in planes_changed; they settle
// the fallback instead, before their upload overwrites the plane it reads.)
static void results_gone(frac_ctx* c)
{
    c->ran = false;
    c->fb_pending = false;
    c->rate.ready = false;
}

int frac_set_params(frac_ctx* c, const frac_params* params)
{
    if (!c)
        return FRAC_E_INVALID;
    std::string msg;
    if (check_params(params, msg) != FRAC_OK)
        return c->fail(FRAC_E_INVALID, msg);
    c->p = *params;
    c->dirty = true;
    results_gone(c);
    return FRAC_OK;
}

static int copy_host_plane(HostPlane& hp, const uint8_t* p, uint32_t w, uint32_t h, uint32_t stride)
{
    if (!p || w == 0 || h == 0 || stride < w)
        return FRAC_E_INVALID;
    hp.w = w;
    hp.h = h;
    hp.data.resize((size_t)w * h);
    for (uint32_t y = 0; y < h; ++y)
        std::memcpy(hp.data.data() + (size_t)y * w, p + (size_t)y * stride, w);
    return FRAC_OK;
}

// A new frame of the same geometry keeps the prepared range/domain structures unless the
// classifier is on (categories depend on the pixels): without it a video frame costs the upload
// and the search only.
static void planes_changed(frac_ctx* c, uint32_t sw, uint32_t sh, uint32_t tw, uint32_t th, bool same)
{
    const bool geometry_kept = c->planes_set && c->src.w == sw && c->src.h == sh && c->tgt.w == tw &&
                               c->tgt.h == th && c->same_plane == same;
    if (!geometry_kept || c->p.use_classifier)
        c->dirty = true;
    c->src.w = sw;
    c->src.h = sh;
    c->tgt.w = tw;
    c->tgt.h = th;
    c->same_plane = same;
    c->planes_set = true;
    c->ran = false;
    c->rate.ready = false;
}

// the host-plane setters: the blocking ones wait until the planes have been consumed, frac_set_frame_async
// does not (upload_planes)
static int set_host_planes(frac_ctx* c, const uint8_t* src, uint32_t sw, uint32_t sh, uint32_t sstride,
                           const uint8_t* tgt, uint32_t tw, uint32_t th, uint32_t tstride, bool wait)
{
    if (!c)
        return FRAC_E_INVALID;
    FRAC_HIP(c, hipSetDevice(c->device));
    if (!src || sw == 0 || sh == 0 || sstride < sw)
        return c->fail(FRAC_E_INVALID, "invalid source plane");
    const bool same = tgt == nullptr || tgt == src;
    if (!same && (tw == 0 || th == 0 || tstride < tw))
        return c->fail(FRAC_E_INVALID, "invalid target plane");
    const PlaneUpload up[2] = {{src, sw, sh, sstride, &c->d_src, &c->frame.d_src_next, &c->d_sstride},
                               {tgt, tw, th, tstride, &c->d_tgt, &c->frame.d_tgt_next, &c->d_tstride}};
    FRAC_TRY(upload_planes(c, up, same ? 1 : 2, same, wait));
    planes_changed(c, sw, sh, same ? sw : tw, same ? sh : th, same);
    return FRAC_OK;
}

int frac_set_planes(frac_ctx* c, const uint8_t* src, uint32_t sw, uint32_t sh, uint32_t sstride, const uint8_t* tgt,
                    uint32_t tw, uint32_t th, uint32_t tstride)
{
    return set_host_planes(c, src, sw, sh, sstride, tgt, tw, th, tstride, true);
}

int frac_set_frame(frac_ctx* c, const uint8_t* plane, uint32_t w, uint32_t h, uint32_t stride)
{
    return set_host_planes(c, plane, w, h, stride, nullptr, 0, 0, 0, true);
}

static int set_frame_device(frac_ctx* c, const void* d_plane, uint32_t w, uint32_t h, uint32_t stride, bool wait)
{
    if (!c)
        return FRAC_E_INVALID;
    if (!d_plane || w == 0 || h == 0 || stride < w)
        return c->fail(FRAC_E_INVALID, "invalid device plane");
    FRAC_HIP(c, hipSetDevice(c->device));
    FRAC_TRY(settle_fallback(c)); // the last run's fp32-regime ranges read the plane this copy overwrites
    // the frame stays on the device: the classifier pre-pass runs there too
    c->d_sstride = plane_pitch(w);
    FRAC_HIP(c, c->d_src.ensure((size_t)c->d_sstride * (h + 1)));
    FRAC_TRY(copy_plane(c, c->d_src.ptr, c->d_sstride, d_plane, stride, w, h, hipMemcpyDeviceToDevice, c->stream));
    if (wait)
        FRAC_HIP(c, hipStreamSynchronize(c->stream));
    planes_changed(c, w, h, w, h, true);
    return FRAC_OK;
}

int frac_set_frame_device(frac_ctx* c, const void* d_plane, uint32_t w, uint32_t h, uint32_t stride)
{
    return set_frame_device(c, d_plane, w, h, stride, true);
}

// frac_set_planes with both planes already on the device: copied as frac_set_frame_device copies one, into the
// current buffers on the context's stream, then frac_set_planes' path (planes_changed).  Every argument is
// checked before anything is touched.
int frac_set_planes_device(frac_ctx* c, const void* d_src, uint32_t sw, uint32_t sh, uint32_t sstride,
                           const void* d_tgt, uint32_t tw, uint32_t th, uint32_t tstride)
{
    if (!c)
        return FRAC_E_INVALID;
    if (!d_src || sw == 0 || sh == 0 || sstride < sw)
        return c->fail(FRAC_E_INVALID, "invalid device source plane");
    const bool same = d_tgt == nullptr || d_tgt == d_src;
    if (same)
        return set_frame_device(c, d_src, sw, sh, sstride, true);
    if (tw == 0 || th == 0 || tstride < tw)
        return c->fail(FRAC_E_INVALID, "invalid device target plane");
    FRAC_HIP(c, hipSetDevice(c->device));
    FRAC_TRY(settle_fallback(c)); // the last run's fp32-regime ranges read the planes these copies overwrite
    const uint32_t sp = plane_pitch(sw), tp = plane_pitch(tw);
    FRAC_HIP(c, c->d_src.ensure((size_t)sp * (sh + 1)));
    FRAC_HIP(c, c->d_tgt.ensure((size_t)tp * (th + 1)));
    c->d_sstride = sp;
    c->d_tstride = tp;
    FRAC_TRY(copy_plane(c, c->d_src.ptr, sp, d_src, sstride, sw, sh, hipMemcpyDeviceToDevice, c->stream));
    FRAC_TRY(copy_plane(c, c->d_tgt.ptr, tp, d_tgt, tstride, tw, th, hipMemcpyDeviceToDevice, c->stream));
    FRAC_HIP(c, hipStreamSynchronize(c->stream));
    planes_changed(c, sw, sh, tw, th, false);
    return FRAC_OK;
}

// Frame streaming from host memory (frac_ctx::FrameStream has the ordering)
int frac_set_frame_async(frac_ctx* c, const uint8_t* plane, uint32_t w, uint32_t h, uint32_t stride)
{
    return set_host_planes(c, plane, w, h, stride, nullptr, 0, 0, 0, false);
}

int frac_set_frame_device_async(frac_ctx* c, const void* d_plane, uint32_t w, uint32_t h, uint32_t stride)
{
    return set_frame_device(c, d_plane, w, h, stride, false);
}

int frac_set_domains(frac_ctx* c, const frac_grid_item* d, size_t nd)
{
    if (!c)
        return FRAC_E_INVALID;
    if (nd && !d)
        return c->fail(FRAC_E_INVALID, "domains is NULL");
    FRAC_TRY(check_domains(c, d, nd));
    c->doms.assign(d, d + nd);
    c->doms_set = true;
    c->doms_uploaded = false;
    c->doms_trusted = false;
    c->dirty = true;
    results_gone(c);
    return FRAC_OK;
}

int frac_set_ranges(frac_ctx* c, const frac_grid_item* r, size_t nr)
{
    if (!c)
        return FRAC_E_INVALID;
    if (nr && !r)
        return c->fail(FRAC_E_INVALID, "ranges is NULL");
    c->ranges.assign(r, r + nr);
    c->ranges_set = true;
    c->ranges_dev = false;
    c->dirty = true;
    results_gone(c);
    return FRAC_OK;
}

int frac_run(frac_ctx* c)
{
    if (!c)
        return FRAC_E_INVALID;
    FRAC_HIP(c, hipSetDevice(c->device));
    FRAC_TRY(check_ab_knobs(c));
    {
        // the work lists prepare() builds depend on the A/B knobs: a change re-prepares
        int var = 0;
        FRAC_TRY(mfma_variant(c, var));
        const int knobs = var * 2 + (mfma_dft_enabled(c) ? 1 : 0);
        if (knobs != c->prep_knobs)
            c->dirty = true;
        c->prep_knobs = knobs;
    }
    // a new run owns the records: the previous run's fused-resolver state and its unsettled fallback
    // (whose saved args may name buffers prepare() is about to reallocate) go, whichever path runs next
    c->rate.ready = false; // a rate state describes the frame as it was searched before this run
    c->fit_fused = false;
    c->fb_pending = false;
    if (c->dirty)
        FRAC_TRY(prepare(c));
    int rc = c->generic ? launch_generic(c) : launch_all_n(c, c->n);
    const uint32_t nr = (uint32_t)nranges(c);
    if (rc == FRAC_OK && c->tuple_sink && nr) {
        if (c->fit_fused) // the resolvers wrote the tuples; the fp32-regime ranges' come with their records
            rc = settle_fallback(c);
        else // records by a separate fit: packed from them
            pack_tuples<<<(nr + 255) / 256, 256, 0, c->stream>>>(c->d_out.ptr, c->d_aux.ptr, c->d_porig.ptr, nr,
                                                                 c->tuple_sink);
    }
    if (rc == FRAC_OK)
        c->ran = true;
    return rc;
}

int frac_set_tuple_sink(frac_ctx* c, void* dst)
{
    if (!c)
        return FRAC_E_INVALID;
    c->tuple_sink = static_cast<frac_tuple*>(dst);
    // where it lies decides the order the sorted resolve writes it in (launch_tp); an address the runtime does
    // not know counts as device memory
    hipPointerAttribute_t at{};
    c->tuple_sink_host = dst && hipPointerGetAttributes(&at, dst) == hipSuccess && at.type == hipMemoryTypeHost;
    (void)hipGetLastError();
    return FRAC_OK;
}

int frac_sync(frac_ctx* c)
{
    if (!c)
        return FRAC_E_INVALID;
    FRAC_HIP(c, hipSetDevice(c->device));
    FRAC_TRY(settle_fallback(c)); // after the sync the records are complete
    FRAC_HIP(c, hipStreamSynchronize(c->stream));
    return FRAC_OK;
}

int frac_fetch(frac_ctx* c, frac_encode_item* out, frac_stats* stats)
{
    if (!c)
        return FRAC_E_INVALID;
    if (!c->ran)
        return c->fail(FRAC_E_STATE, "frac_fetch before frac_run");
    const size_t nr = nranges(c);
    if (nr && out)
        FRAC_HIP(c, hipMemcpyAsync(out, c->d_out.ptr, nr * sizeof(frac_encode_item), hipMemcpyDeviceToHost, c->stream));
    if (nr)
        FRAC_HIP(c, hipMemcpyAsync(c->h_aux.data(), c->d_aux.ptr, nr * sizeof(RangeAux), hipMemcpyDeviceToHost,
                                   c->stream));
    if (nr && stats && c->p.use_classifier) { // the per-range buckets of the reject count
        c->h_rkey.resize(nr);
        FRAC_HIP(c, hipMemcpyAsync(c->h_rkey.data(), c->d_rkey.ptr, nr * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                   c->stream));
    }
    unsigned long long sea_count = 0;
    const bool sea_ran = c->engine_ran == FRAC_ENGINE_SEA && c->form_ran == FRAC_FORM_SEA;
    if (sea_ran)
        FRAC_HIP(c, hipMemcpyAsync(&sea_count, c->d_sea_count.ptr, sizeof(sea_count), hipMemcpyDeviceToHost,
                                   c->stream));
    uint32_t listed = 0; // the fused resolvers' fp32-regime ranges (settle_fallback)
    if (c->fb_pending)
        FRAC_HIP(c, hipMemcpyAsync(&listed, c->d_fb_count.ptr, sizeof(listed), hipMemcpyDeviceToHost, c->stream));
    FRAC_HIP(c, hipStreamSynchronize(c->stream));
    if (c->fb_pending) {
        if (listed) { // rare: their records come from fallback_grid, then the copies again
            FRAC_HIP(c, hipSetDevice(c->device));
            FRAC_TRY(settle_fallback(c));
            if (nr && out)
                FRAC_HIP(c, hipMemcpyAsync(out, c->d_out.ptr, nr * sizeof(frac_encode_item), hipMemcpyDeviceToHost,
                                           c->stream));
            if (nr)
                FRAC_HIP(c, hipMemcpyAsync(c->h_aux.data(), c->d_aux.ptr, nr * sizeof(RangeAux),
                                           hipMemcpyDeviceToHost, c->stream));
            FRAC_HIP(c, hipStreamSynchronize(c->stream));
        }
        c->fb_pending = false;
    }
    if (sea_ran)
        c->evaluated_ran = sea_count;
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->total_mappings = (uint64_t)c->doms.size() * nr;
        stats->engine = c->engine_ran;
        stats->search_form = c->form_ran;
        stats->matrix_flops = c->flops_ran;
        stats->evaluated_mappings = c->evaluated_ran;
        const uint64_t nd = c->doms.size();
        if (c->p.use_classifier) { // a hit's rejects depend on its domain's grid index: the pool order
            bool any_hit = false;
            for (size_t r = 0; r < nr && !any_hit; ++r)
                any_hit = (c->h_aux[r].flags & kAuxHit) && !(c->h_aux[r].flags & kAuxEmpty);
            if (any_hit) {
                c->h_porig.resize(c->npos);
                FRAC_HIP(c, hipMemcpyAsync(c->h_porig.data(), c->d_porig.ptr, c->npos * sizeof(uint32_t),
                                           hipMemcpyDeviceToHost, c->stream));
                FRAC_HIP(c, hipStreamSynchronize(c->stream));
            }
        }
        for (size_t r = 0; r < nr; ++r) {
            const RangeAux& ax = c->h_aux[r];
            const int b = c->p.use_classifier ? (int)c->h_rkey[r] : 0;
            const uint64_t bsize = c->bucket_end[b] - c->bucket_begin[b];
            if (ax.flags & kAuxEmpty) {
                ++stats->empty_ranges;
                if (c->p.use_classifier)
                    stats->rejected_mappings += nd;
                continue;
            }
            if (ax.flags & kAuxFallback)
                ++stats->fallback_ranges;
            if (ax.flags & kAuxHit) {
                ++stats->hit_ranges;
                if (c->p.use_classifier)
                    stats->rejected_mappings += (uint64_t)c->h_porig[ax.pos] - (ax.pos - c->bucket_begin[b]);
            } else if (c->p.use_classifier) {
                stats->rejected_mappings += nd - bsize;
            }
        }
        if (c->p.flags & FRAC_FLAG_TIMING)
            add_run_times(*stats, last_events(c)); // (the stats were zeroed above)
    }
    return FRAC_OK;
}

int frac_timing_history(frac_ctx* c, frac_run_timing* out, size_t cap, size_t* n_out)
{
    if (!c || !n_out)
        return FRAC_E_INVALID;
    *n_out = 0;
    if (!(c->p.flags & FRAC_FLAG_TIMING))
        return c->fail(FRAC_E_STATE, "timing history needs FRAC_FLAG_TIMING");
    FRAC_HIP(c, hipSetDevice(c->device));
    FRAC_HIP(c, hipStreamSynchronize(c->stream));
    const uint64_t first = std::max<uint64_t>(c->hist_read, c->hist_runs > kHistRuns ? c->hist_runs - kHistRuns : 0);
    size_t k = 0;
    for (uint64_t r = first; r < c->hist_runs; ++r, ++k) {
        if (!out || k >= cap)
            continue;
        const Event* e = &c->hist[(size_t)(r % kHistRuns) * 4];
        float ms[4] = {0.f, 0.f, 0.f, 0.f};
        const int pairs[4][2] = {{0, 3}, {0, 1}, {1, 2}, {2, 3}};
        for (int q = 0; q < 4; ++q)
            if (hipEventElapsedTime(&ms[q], e[pairs[q][0]], e[pairs[q][1]]) != hipSuccess)
                ms[q] = 0.f;
        out[k] = frac_run_timing{ms[0], ms[1], ms[2], ms[3]};
    }
    (void)hipGetLastError(); // an unrecorded boundary leaves a sticky "not ready": not an error
    *n_out = k;
    if (out)
        c->hist_read = c->hist_runs;
    return FRAC_OK;
}

int frac_search(frac_ctx* c, const frac_grid_item* ranges, size_t nr, frac_encode_item* out, frac_stats* stats)
{
    FRAC_TRY(frac_set_ranges(c, ranges, nr));
    FRAC_TRY(frac_run(c));
    return frac_fetch(c, out, stats);
}

int frac_set_stream(frac_ctx* c, void* s)
{
    if (!c)
        return FRAC_E_INVALID;
    hipStream_t next = s ? reinterpret_cast<hipStream_t>(s) : (hipStream_t)c->own_stream;
    if (next == c->stream)
        return FRAC_OK;
    FRAC_HIP(c, hipSetDevice(c->device));
    // the last run's fallback goes on the stream its search and resolve ran on, and everything enqueued on
    // that stream so far comes before what is enqueued on the new one: a switch keeps the context's order
    FRAC_TRY(settle_fallback(c));
    if (!c->handoff)
        FRAC_HIP(c, hipEventCreateWithFlags(&c->handoff.e, hipEventDisableTiming));
    FRAC_HIP(c, hipEventRecord(c->handoff, c->stream));
    FRAC_HIP(c, hipStreamWaitEvent(next, c->handoff, 0));
    c->stream = next;
    return FRAC_OK;
}

void* frac_get_stream(frac_ctx* c) { return c ? reinterpret_cast<void*>(c->stream) : nullptr; }

const frac_encode_item* frac_device_results(frac_ctx* c)
{
    if (!c)
        return nullptr;
    if (!c->ran) { // no run yet, or a setter since the last one: d_out holds nothing of the current state
        c->fail(FRAC_E_STATE, "no results: frac_run has not been called");
        return nullptr;
    }
    // work enqueued on the context's stream after this call reads complete records
    if (c->fb_pending && (hipSetDevice(c->device) != hipSuccess || settle_fallback(c) != FRAC_OK))
        return nullptr;
    return c->d_out.ptr;
}

int frac_classify_items(frac_ctx* c, frac_grid_item* items, size_t n, int target_plane)
{
    if (!c)
        return FRAC_E_INVALID;
    if (n && !items)
        return c->fail(FRAC_E_INVALID, "classify: items is NULL");
    if (!c->planes_set)
        return c->fail(FRAC_E_STATE, "classify: no frame set");
    const bool tgt = target_plane != 0 && !c->same_plane;
    const auto& hp = tgt ? c->tgt : c->src;
    std::vector<frac_grid_item> v(items, items + n);
    std::vector<uint32_t> list(n);
    for (size_t i = 0; i < n; ++i) {
        if ((uint64_t)v[i].x + v[i].w > hp.w || (uint64_t)v[i].y + v[i].h > hp.h)
            return c->fail(FRAC_E_INVALID, "classify: item outside the plane");
        list[i] = (uint32_t)i;
    }
    FRAC_HIP(c, hipSetDevice(c->device));
    std::vector<int32_t> cat;
    FRAC_TRY(classify_on_device(c, v, list, tgt ? c->d_tgt.ptr : c->d_src.ptr, tgt ? c->d_tstride : c->d_sstride,
                                cat));
    for (size_t i = 0; i < n; ++i)
        items[i].category = cat[i];
    return FRAC_OK;
}

int frac_copy_tuples_device(frac_ctx* c, void* d_dst)
{
    if (!c)
        return FRAC_E_INVALID;
    if (!c->ran)
        return c->fail(FRAC_E_STATE, "no results: frac_run has not been called");
    const uint32_t nr = (uint32_t)nranges(c);
    if (nr) {
        if (!d_dst)
            return c->fail(FRAC_E_INVALID, "copy_tuples: NULL destination");
        FRAC_HIP(c, hipSetDevice(c->device));
        FRAC_TRY(settle_fallback(c));
        pack_tuples<<<(nr + 255) / 256, 256, 0, c->stream>>>(c->d_out.ptr, c->d_aux.ptr, c->d_porig.ptr, nr,
                                                             static_cast<frac_tuple*>(d_dst));
        FRAC_HIP(c, hipGetLastError());
    }
    return FRAC_OK;
}

int frac_fetch_tuples(frac_ctx* c, frac_tuple* out)
{
    if (!c)
        return FRAC_E_INVALID;
    if (!c->ran)
        return c->fail(FRAC_E_STATE, "no results: frac_run has not been called");
    const size_t nr = nranges(c);
    if (!nr)
        return FRAC_OK;
    if (!out)
        return c->fail(FRAC_E_INVALID, "fetch_tuples: NULL destination");
    FRAC_HIP(c, c->d_tuples.ensure(nr));
    FRAC_TRY(frac_copy_tuples_device(c, c->d_tuples.ptr));
    FRAC_HIP(c, hipMemcpyAsync(out, c->d_tuples.ptr, nr * sizeof(frac_tuple), hipMemcpyDeviceToHost, c->stream));
    FRAC_HIP(c, hipStreamSynchronize(c->stream));
    return FRAC_OK;
}

int frac_copy_results_device(frac_ctx* c, void* d_dst)
{
    if (!c)
        return FRAC_E_INVALID;
    if (!c->ran)
        return c->fail(FRAC_E_STATE, "no results: frac_run has not been called");
    const size_t nr = nranges(c);
    FRAC_HIP(c, hipSetDevice(c->device));
    FRAC_TRY(settle_fallback(c));
    if (nr)
        FRAC_HIP(c, hipMemcpyAsync(d_dst, c->d_out.ptr, nr * sizeof(frac_encode_item), hipMemcpyDeviceToDevice,
                                   c->stream));
    return FRAC_OK;
}

size_t frac_uniform_grid2(uint32_t W, uint32_t H, uint32_t size_w, uint32_t size_h, uint32_t off_x, uint32_t off_y,
                          frac_grid_item* out, size_t cap)
{
    // createUniformGrid's loop (image/partition2.hpp:123-133): x advances by the offset's x, a row
    // ends when the next item would cross the right edge, the grid when the next row would cross
    // the bottom edge
    // — so a row holds ⌊(W − w)/off_x⌋ + 1 items and the grid ⌊(H − h)/off_y⌋ + 1 rows (the count in closed
    // form: the loop took 0.2 ms for the 4-pixel quadtree level's domains at 2048², on every quadtree call)
    if (size_w == 0 || size_h == 0 || off_x == 0 || off_y == 0 || W < size_w || H < size_h)
        return 0;
    const size_t cols = (W - size_w) / off_x + 1, rows = (H - size_h) / off_y + 1;
    if (out) {
        size_t n = 0;
        for (size_t r = 0; r < rows && n < cap; ++r)
            for (size_t k = 0; k < cols && n < cap; ++k)
                out[n++] = frac_grid_item{(uint32_t)(k * off_x), (uint32_t)(r * off_y), size_w, size_h, -1};
    }
    return cols * rows;
}

size_t frac_uniform_grid(uint32_t W, uint32_t H, uint32_t size, uint32_t offset, frac_grid_item* out, size_t cap)
{
    return frac_uniform_grid2(W, H, size, size, offset, offset, out, cap);
}

int frac_classify(const uint8_t* plane, uint32_t w, uint32_t h, uint32_t stride, frac_grid_item* items, size_t n)
{
    HostPlane hp;
    if (copy_host_plane(hp, plane, w, h, stride) != FRAC_OK || (n && !items)) {
        g_last_error = "frac_classify: invalid arguments";
        return FRAC_E_INVALID;
    }
    for (size_t i = 0; i < n; ++i) {
        if ((uint64_t)items[i].x + items[i].w > w || (uint64_t)items[i].y + items[i].h > h) {
            g_last_error = "frac_classify: item outside the plane";
            return FRAC_E_INVALID;
        }
        items[i].category = category(hp, items[i]);
    }
    return FRAC_OK;
}

int frac_transform_index(uint32_t n, uint32_t t, uint32_t pix)
{
    if (t > 7 || pix >= n * n)
        return -1;
    switch (n) {
    case 2: return fwd_index<2>((int)t, (int)pix);
    case 4: return fwd_index<4>((int)t, (int)pix);
    case 8: return fwd_index<8>((int)t, (int)pix);
    case 16: return fwd_index<16>((int)t, (int)pix);
    default: return -1;
    }
}

int64_t frac_hit_limit(double rms_threshold, uint32_t n) { return compute_hit_limit(rms_threshold, 4u * n * n); }

} // extern "C"
