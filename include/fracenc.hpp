// fracenc.hpp — C++17 host layer over the C ABI (include/fracenc.h).
//
// The reference's host side is C++ (encode/Encoder2.hpp, encode/EncodingEngine2.hpp); this
// header gives a C++ caller the same roles without any reference types:
//
//   Engine              RAII frac_ctx: one search context on one GPU (an AbstractEncodingEngine2
//                       that takes batches, encode/EncodingEngine2.hpp:50-85)
//   EncodingEngineCore  EncodingEngineCore2's role (encode/EncodingEngine2.hpp:118-171): a host
//                       pool of engines (one std::thread each, any mix of devices) claiming
//                       BATCHES of ranges from a shared counter instead of one item at a time
//                       (:131-140); results come back in range order (the reference's order is
//                       thread-dependent, :165-168)
//   Quantizer<T>        Frac::Quantizer (encode/Quantizer.hpp:7-45) as the built reference
//                       computes it (value() with the FMA the compiler contracts)
//   createUniformGrid / preclassify / encodeQuadtree / decode / decode_frc1 / frc1_info / decode_frq1 / frq1_info /
//                       pack_frq1 / decode_frc3 / frc3_info / quadtreeRate, rateSizes, rateFit, rateLeaves /
//                       decodeError, rateErrors, rateQuality / setPlanesDevice, decodeInter, decodeInterDevice,
//                       interError — the C ABI entry points
//   Engine's ABI 8/9 methods: an external HIP stream (void*), the tuple sink and 32-byte tuples,
//                       frame streaming (setFrameAsync / setFrameDeviceAsync), 32-byte quadtree
//                       leaves, per-run device times
//
// Errors throw fracenc::Error carrying frac_last_error.
#pragma once

#include "fracenc.h"

#include <array>
#include <atomic>
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace fracenc {

class Error : public std::runtime_error {
public:
    explicit Error(const std::string& m) : std::runtime_error(m) {}
};

struct Params {
    uint32_t transforms = 4;    // 4: TransformMatcher::match (transformmatcher.h:41-45); 8: all dihedral
    bool use_classifier = false;
    double rms_threshold = 0.0; // encode_parameters_t::rmsThreshold
    double s_max = -1.0;        // encode_parameters_t::sMax
    uint32_t engine = FRAC_ENGINE_AUTO;
    bool timing = false;

    frac_params c() const
    {
        frac_params p{};
        p.transforms = transforms;
        p.use_classifier = use_classifier ? 1 : 0;
        p.rms_threshold = rms_threshold;
        p.s_max = s_max;
        p.engine = engine;
        p.flags = timing ? FRAC_FLAG_TIMING : 0u;
        return p;
    }
};

inline std::vector<frac_grid_item> createUniformGrid(uint32_t w, uint32_t h, uint32_t size, uint32_t offset)
{
    std::vector<frac_grid_item> g(frac_uniform_grid(w, h, size, offset, nullptr, 0));
    if (!g.empty())
        frac_uniform_grid(w, h, size, offset, g.data(), g.size());
    return g;
}

// BrightnessBlocksClassifier2::preclassify on the host (main.cpp:155-162)
inline void preclassify(const uint8_t* plane, uint32_t w, uint32_t h, uint32_t stride,
                        std::vector<frac_grid_item>& items)
{
    if (frac_classify(plane, w, h, stride, items.data(), items.size()) != FRAC_OK)
        throw Error(frac_last_error(nullptr));
}

// An FRC1 stream's header, parsed and validated against the stream length on the host (frac_frc1_info;
// the C name is also the function's, hence the alias).
using Frc1Info = struct ::frac_frc1_info;
inline Frc1Info frc1_info(const uint8_t* stream, size_t len)
{
    Frc1Info info{};
    if (frac_frc1_info(stream, len, &info) != FRAC_OK)
        throw Error(std::string("fracenc: ") + frac_last_error(nullptr));
    return info;
}

// The same for an FRQ1 quadtree stream: header, per-level counts and section offsets (frac_frq1_info).
using Frq1Info = struct ::frac_frq1_info;
inline Frq1Info frq1_info(const uint8_t* stream, size_t len)
{
    Frq1Info info{};
    if (frac_frq1_info(stream, len, &info) != FRAC_OK)
        throw Error(std::string("fracenc: ") + frac_last_error(nullptr));
    return info;
}

// The same for an FRC3 colour container: the frame, and each plane stream's kind and place (frac_frc3_info).
using Frc3Info = struct ::frac_frc3_info;
inline Frc3Info frc3_info(const uint8_t* stream, size_t len)
{
    Frc3Info info{};
    if (frac_frc3_info(stream, len, &info) != FRAC_OK)
        throw Error(std::string("fracenc: ") + frac_last_error(nullptr));
    return info;
}

// Quadtree leaves (Engine::encodeQuadtreeLeaves' order) as an FRQ1 stream, packed on the host (frac_pack_frq1).
inline std::vector<uint8_t> pack_frq1(const std::vector<frac_qt_leaf>& leaves, uint32_t w, uint32_t h,
                                      uint32_t max_size, uint32_t min_size, uint32_t transforms = 4,
                                      bool use_classifier = false, uint32_t contrast_bits = 5,
                                      uint32_t brightness_bits = 7)
{
    size_t n = 0;
    std::vector<uint8_t> out;
    for (int pass = 0; pass < 2; ++pass) {
        if (frac_pack_frq1(leaves.data(), leaves.size(), w, h, max_size, min_size, transforms, use_classifier ? 1u : 0u,
                           contrast_bits, brightness_bits, pass ? out.data() : nullptr, out.size(), &n) != FRAC_OK)
            throw Error(std::string("fracenc: ") + frac_last_error(nullptr));
        out.resize(n);
    }
    return out;
}

class Engine {
public:
    Engine(int device, const Params& p)
    {
        const frac_params cp = p.c();
        ctx_ = frac_create(device, &cp);
        if (!ctx_)
            throw Error(std::string("frac_create: ") + frac_last_error(nullptr));
    }
    ~Engine() { frac_destroy(ctx_); }
    Engine(const Engine&) = delete;
    Engine& operator=(const Engine&) = delete;
    Engine(Engine&& o) noexcept : ctx_(std::exchange(o.ctx_, nullptr)), w_(o.w_), h_(o.h_), rate_min_(o.rate_min_) {}

    frac_ctx* get() const { return ctx_; }

    void setFrame(const uint8_t* plane, uint32_t w, uint32_t h, uint32_t stride)
    {
        check(frac_set_frame(ctx_, plane, w, h, stride));
        w_ = w;
        h_ = h;
    }
    void setFrameDevice(const void* d_plane, uint32_t w, uint32_t h, uint32_t stride)
    {
        check(frac_set_frame_device(ctx_, d_plane, w, h, stride));
        w_ = w;
        h_ = h;
    }
    // domains on d_src, ranges on d_tgt, both already on the device, strides in bytes (frac_set_planes_device;
    // probe for the symbol by name when the library may be older)
    void setPlanesDevice(const void* d_src, uint32_t sw, uint32_t sh, uint32_t sstride, const void* d_tgt, uint32_t tw,
                         uint32_t th, uint32_t tstride)
    {
        check(frac_set_planes_device(ctx_, d_src, sw, sh, sstride, d_tgt, tw, th, tstride));
        w_ = sw;
        h_ = sh;
    }
    // ABI 9: frame streaming.  setFrameAsync uploads on the context's copy stream into its second plane buffer
    // while the runs already enqueued read the current one (pinned host memory makes it asynchronous; the plane
    // must stay unchanged until a later sync / fetch); setFrameDeviceAsync copies a device plane on the
    // context's stream without a host wait.
    void setFrameAsync(const uint8_t* plane, uint32_t w, uint32_t h, uint32_t stride)
    {
        check(frac_set_frame_async(ctx_, plane, w, h, stride));
        w_ = w;
        h_ = h;
    }
    void setFrameDeviceAsync(const void* d_plane, uint32_t w, uint32_t h, uint32_t stride)
    {
        check(frac_set_frame_device_async(ctx_, d_plane, w, h, stride));
        w_ = w;
        h_ = h;
    }
    // an external hipStream_t (as void*; nullptr: the context's own), ordered after the previous stream's work
    void setStream(void* hip_stream) { check(frac_set_stream(ctx_, hip_stream)); }
    void* stream() const { return frac_get_stream(ctx_); }
    // ABI 8: every later run writes its 32-byte tuples into dst (device memory or pinned host memory); nullptr
    // clears it
    void setTupleSink(void* dst) { check(frac_set_tuple_sink(ctx_, dst)); }
    // the last run's tuples (north_star's (domain, transform, s, o, rms)), synchronously
    void fetchTuples(frac_tuple* out) { check(frac_fetch_tuples(ctx_, out)); }
    // per-run device times since the previous call (FRAC_FLAG_TIMING, Params::timing)
    std::vector<frac_run_timing> timingHistory()
    {
        size_t n = 0;
        check(frac_timing_history(ctx_, nullptr, 0, &n));
        std::vector<frac_run_timing> out(n);
        check(frac_timing_history(ctx_, out.data(), out.size(), &n));
        out.resize(n);
        return out;
    }
    void setDomains(const std::vector<frac_grid_item>& d) { check(frac_set_domains(ctx_, d.data(), d.size())); }
    void setRanges(const frac_grid_item* r, size_t n) { check(frac_set_ranges(ctx_, r, n)); }
    void run() { check(frac_run(ctx_)); }
    void sync() { check(frac_sync(ctx_)); }
    void fetch(frac_encode_item* out, frac_stats* st = nullptr)
    {
        frac_stats tmp{};
        check(frac_fetch(ctx_, out, st ? st : &tmp));
    }
    std::vector<frac_encode_item> search(const std::vector<frac_grid_item>& ranges, frac_stats* st = nullptr)
    {
        std::vector<frac_encode_item> out(ranges.size());
        frac_stats tmp{};
        check(frac_search(ctx_, ranges.data(), ranges.size(), out.data(), st ? st : &tmp));
        return out;
    }
    std::vector<frac_grid_item> classify(std::vector<frac_grid_item> items)
    {
        check(frac_classify_items(ctx_, items.data(), items.size(), 0));
        return items;
    }
    std::vector<frac_encode_item> encodeQuadtree(uint32_t max_size, uint32_t min_size, double split_distance,
                                                 frac_stats* st = nullptr)
    {
        const frac_quadtree_params qp{max_size, min_size, split_distance};
        size_t cap = (size_t)(w_ / min_size) * (h_ / min_size), n = 0;
        std::vector<frac_encode_item> out(cap);
        frac_stats tmp{};
        check(frac_encode_quadtree(ctx_, &qp, out.data(), cap, &n, st ? st : &tmp));
        out.resize(n);
        return out;
    }
    // the same partition as 32-byte frac_qt_leaf items (ABI 7): half the bytes of encodeQuadtree's records
    std::vector<frac_qt_leaf> encodeQuadtreeLeaves(uint32_t max_size, uint32_t min_size, double split_distance,
                                                   frac_stats* st = nullptr)
    {
        const frac_quadtree_params qp{max_size, min_size, split_distance};
        size_t cap = (size_t)(w_ / min_size) * (h_ / min_size), n = 0;
        std::vector<frac_qt_leaf> out(cap);
        frac_stats tmp{};
        check(frac_encode_quadtree_leaves(ctx_, &qp, out.data(), cap, &n, st ? st : &tmp));
        out.resize(n);
        return out;
    }
    // The quadtree rate sweep (probe for the symbols by name when the library may be older): quadtreeRate
    // searches the full tree once; rateSizes / rateFit / rateLeaves then answer for any split distance without a
    // search, until the next setter, run or quadtree encode.
    void quadtreeRate(uint32_t max_size, uint32_t min_size, frac_stats* st = nullptr)
    {
        check(frac_quadtree_rate_build(ctx_, max_size, min_size, st));
        rate_min_ = min_size;
    }
    // per split distance the FRQ1 stream's bytes; leaves and splits ([n][4]) when asked for
    std::vector<uint64_t> rateSizes(const std::vector<double>& split, uint32_t contrast_bits = 5,
                                    uint32_t brightness_bits = 7, std::vector<uint32_t>* leaves = nullptr,
                                    std::vector<uint32_t>* splits = nullptr)
    {
        std::vector<uint64_t> bytes(split.size());
        if (leaves)
            leaves->resize(split.size());
        if (splits)
            splits->resize(4 * split.size());
        check(frac_quadtree_rate_sizes(ctx_, contrast_bits, brightness_bits, split.data(), split.size(), bytes.data(),
                                       leaves ? leaves->data() : nullptr, splits ? splits->data() : nullptr));
        return bytes;
    }
    struct RateFit {
        double split_distance;
        uint64_t bytes;
        uint32_t leaves;
    };
    // the smallest split distance whose stream has at most max_bytes; throws when none fits
    RateFit rateFit(uint64_t max_bytes, uint32_t contrast_bits = 5, uint32_t brightness_bits = 7)
    {
        RateFit f{};
        check(frac_quadtree_rate_fit(ctx_, contrast_bits, brightness_bits, max_bytes, &f.split_distance, &f.bytes,
                                     &f.leaves));
        return f;
    }
    std::vector<frac_qt_leaf> rateLeaves(double split_distance)
    {
        size_t cap = rate_min_ ? (size_t)(w_ / rate_min_) * (h_ / rate_min_) : 0, n = 0;
        std::vector<frac_qt_leaf> out(cap);
        check(frac_quadtree_rate_leaves(ctx_, split_distance, out.data(), cap, &n));
        out.resize(n < cap ? n : cap);
        return out;
    }
    // Decoded quality (probe for the symbols by name when the library may be older; include/fracenc.h states
    // the rules).  decodeError: an FRC1 or FRQ1 stream decoded on the device and compared there with the frame
    // set on this engine, over the rectangle its g × g grid covers; block_sse, when given, receives the
    // (W / g)·(H / g) block sums, row-major.
    struct DecodeError {
        uint64_t sse, pixels;
        int iterations;
        double rms;
        // 10·log10(255²·pixels / sse); +inf at sse == 0
        double psnr() const
        {
            return sse ? 10.0 * std::log10(255.0 * 255.0 * (double)pixels / (double)sse)
                       : std::numeric_limits<double>::infinity();
        }
    };
    DecodeError decodeError(const uint8_t* stream, size_t len, int max_iter = -1, double rms_eps = 1e-5,
                            std::vector<uint64_t>* block_sse = nullptr)
    {
        DecodeError r{};
        size_t n = 0;
        if (block_sse) { // sized from the header; a stream the parsers refuse throws there
            uint32_t W, H, g;
            if (stream && len >= 4 && std::memcmp(stream, "FRQ1", 4) == 0) {
                const Frq1Info i = frq1_info(stream, len);
                W = i.width, H = i.height, g = i.max_size;
            } else {
                const Frc1Info i = frc1_info(stream, len);
                W = i.width, H = i.height, g = i.range_size;
            }
            n = g ? (size_t)(W / g) * (H / g) : 0;
            block_sse->assign(n, 0);
        }
        check(frac_decode_error(ctx_, stream, len, max_iter, rms_eps, &r.sse, &r.pixels,
                                block_sse && n ? block_sse->data() : nullptr, n, &n, &r.iterations, &r.rms));
        return r;
    }
    // per split distance of the rate state the decoded sse; the streams' bytes and the iterations when asked for
    std::vector<uint64_t> rateErrors(const std::vector<double>& split, uint32_t contrast_bits = 5,
                                     uint32_t brightness_bits = 7, int max_iter = -1, double rms_eps = 1e-5,
                                     std::vector<uint64_t>* bytes = nullptr, std::vector<int>* iterations = nullptr)
    {
        std::vector<uint64_t> sse(split.size());
        if (bytes)
            bytes->resize(split.size());
        if (iterations)
            iterations->resize(split.size());
        check(frac_quadtree_rate_errors(ctx_, contrast_bits, brightness_bits, split.data(), split.size(), max_iter,
                                        rms_eps, sse.data(), bytes ? bytes->data() : nullptr,
                                        iterations ? iterations->data() : nullptr));
        return sse;
    }
    struct RateQuality {
        double split_distance;
        uint64_t bytes;
        uint32_t leaves;
        uint64_t sse;
        uint32_t probes;
    };
    // a split distance whose decoded sse is at most max_sse while the next larger candidate's is not (the stated
    // bisection; not necessarily the largest that meets it: the error is not monotone); throws when the smallest
    // split distance fails
    RateQuality rateQuality(uint64_t max_sse, uint32_t contrast_bits = 5, uint32_t brightness_bits = 7,
                            int max_iter = -1, double rms_eps = 1e-5)
    {
        RateQuality q{};
        check(frac_quadtree_rate_quality(ctx_, contrast_bits, brightness_bits, max_sse, max_iter, rms_eps,
                                         &q.split_distance, &q.bytes, &q.leaves, &q.sse, &q.probes));
        return q;
    }
    // the rate state's candidates {0.0} ∪ {e(v)}, ascending and distinct: the list rateQuality bisects
    // (frac_quadtree_rate_candidates)
    std::vector<double> rateCandidates()
    {
        size_t n = 0;
        check(frac_quadtree_rate_candidates(ctx_, nullptr, 0, &n));
        std::vector<double> c(n);
        check(frac_quadtree_rate_candidates(ctx_, c.data(), c.size(), &n));
        c.resize(std::min(n, c.size()));
        return c;
    }
    // The decoded RGB error of an FRC3 colour container against a packed RGB reference of the container's frame,
    // rows rgb_stride bytes apart (frac_decode_error_frc3; device = true: rgb is a device pointer, read on the
    // context's stream, frac_decode_error_frc3_device): the R, G and B sums over the rectangle all three planes'
    // grids cover, its area, and per plane (Y, U, V) the iteration count and the final rms.
    struct ColorError {
        uint64_t channel_sse[3], pixels;
        int iterations[3];
        double rms[3];
        uint64_t sse() const { return channel_sse[0] + channel_sse[1] + channel_sse[2]; }
        // 10·log10(255²·3·pixels / sse); +inf at sse == 0
        double psnr() const
        {
            return sse() ? 10.0 * std::log10(255.0 * 255.0 * 3.0 * (double)pixels / (double)sse())
                         : std::numeric_limits<double>::infinity();
        }
    };
    ColorError decodeErrorFrc3(const uint8_t* stream, size_t len, const void* rgb, uint32_t rgb_stride,
                               bool device = false, int max_iter = -1, double rms_eps = 1e-5)
    {
        ColorError r{};
        check(device ? frac_decode_error_frc3_device(ctx_, stream, len, rgb, rgb_stride, max_iter, rms_eps,
                                                     r.channel_sse, &r.pixels, r.iterations, r.rms)
                     : frac_decode_error_frc3(ctx_, stream, len, static_cast<const uint8_t*>(rgb), rgb_stride, max_iter,
                                              rms_eps, r.channel_sse, &r.pixels, r.iterations, r.rms));
        return r;
    }
    // Inter-coded frames (include/fracenc.h states the rules): an FRC1 or FRQ1 stream applied once to a reference
    // plane of scale·W × scale·H.  decodeInter: tight host planes; `plane` is resized and receives the result.
    // decodeInterDevice: device planes read and written in place on the context's stream, strides in bytes,
    // plane_bytes up to the last row's end.  interError: the stream applied at scale 1 to the plane the domains
    // lie on and compared with the plane the ranges lie on, over decodeError's covered rectangle.
    void decodeInter(const uint8_t* stream, size_t len, const std::vector<uint8_t>& ref, std::vector<uint8_t>& plane,
                     uint32_t scale = 1)
    {
        plane.resize(ref.size());
        check(frac_decode_inter(ctx_, stream, len, scale, ref.data(), plane.data(), plane.size()));
    }
    void decodeInterDevice(const uint8_t* stream, size_t len, const void* d_ref, uint32_t ref_stride, void* d_plane,
                           uint32_t plane_stride, size_t plane_bytes, uint32_t scale = 1)
    {
        check(frac_decode_inter_device(ctx_, stream, len, scale, d_ref, ref_stride, d_plane, plane_stride, plane_bytes));
    }
    struct InterError {
        uint64_t sse, pixels;
        // 10·log10(255²·pixels / sse); +inf at sse == 0
        double psnr() const
        {
            return sse ? 10.0 * std::log10(255.0 * 255.0 * (double)pixels / (double)sse)
                       : std::numeric_limits<double>::infinity();
        }
    };
    InterError interError(const uint8_t* stream, size_t len)
    {
        InterError r{};
        check(frac_inter_error(ctx_, stream, len, &r.sse, &r.pixels));
        return r;
    }
    // Decoder2::decode (encode/Encoder2.hpp:67-88); plane holds the caller's initial target
    // (main.cpp zeroes it) and receives the result.  Returns {iterations, rms}.
    std::pair<int, double> decode(const std::vector<frac_encode_item>& items, uint32_t w, uint32_t h,
                                  std::vector<uint8_t>& plane, int max_iter = -1, double rms_eps = 1e-5)
    {
        plane.resize((size_t)w * h);
        int it = 0;
        double rms = 0.0;
        check(frac_decode(ctx_, items.data(), items.size(), w, h, max_iter, rms_eps, plane.data(), &it, &rms));
        return {it, rms};
    }
    // The same for an FRC1 stream (frac_decode_frc1), unpacked and decoded on the device with every
    // coordinate and size multiplied by `scale`; plane becomes scale·W × scale·H (kept when it already
    // has that size: the caller's initial target, else zero-filled).
    std::pair<int, double> decode_frc1(const uint8_t* stream, size_t len, std::vector<uint8_t>& plane,
                                       uint32_t scale = 1, int max_iter = -1, double rms_eps = 1e-5)
    {
        const Frc1Info info = frc1_info(stream, len);
        const uint32_t k = scale >= 1 && scale <= 16 ? scale : 0; // the library refuses the scale itself
        const size_t need = (size_t)k * info.width * k * info.height;
        if (plane.size() != need)
            plane.assign(need, 0);
        int it = 0;
        double rms = 0.0;
        check(frac_decode_frc1(ctx_, stream, len, scale, max_iter, rms_eps, plane.data(), plane.size(), &it, &rms));
        return {it, rms};
    }
    std::pair<int, double> decode_frc1(const std::vector<uint8_t>& stream, std::vector<uint8_t>& plane,
                                       uint32_t scale = 1, int max_iter = -1, double rms_eps = 1e-5)
    {
        return decode_frc1(stream.data(), stream.size(), plane, scale, max_iter, rms_eps);
    }
    // The same for an FRQ1 quadtree stream (frac_decode_frq1).
    std::pair<int, double> decode_frq1(const uint8_t* stream, size_t len, std::vector<uint8_t>& plane,
                                       uint32_t scale = 1, int max_iter = -1, double rms_eps = 1e-5)
    {
        const Frq1Info info = frq1_info(stream, len);
        const uint32_t k = scale >= 1 && scale <= 16 ? scale : 0; // the library refuses the scale itself
        const size_t need = (size_t)k * info.width * k * info.height;
        if (plane.size() != need)
            plane.assign(need, 0);
        int it = 0;
        double rms = 0.0;
        check(frac_decode_frq1(ctx_, stream, len, scale, max_iter, rms_eps, plane.data(), plane.size(), &it, &rms));
        return {it, rms};
    }
    std::pair<int, double> decode_frq1(const std::vector<uint8_t>& stream, std::vector<uint8_t>& plane,
                                       uint32_t scale = 1, int max_iter = -1, double rms_eps = 1e-5)
    {
        return decode_frq1(stream.data(), stream.size(), plane, scale, max_iter, rms_eps);
    }
    // An FRC3 colour container to packed RGB (frac_decode_frc3): the three plane streams decoded and converted
    // on the device; rgb becomes 3·scale·W × scale·H bytes, rows tight.  Per plane (Y, U, V) the iteration
    // count and the final rms.
    std::array<std::pair<int, double>, 3> decode_frc3(const uint8_t* stream, size_t len, std::vector<uint8_t>& rgb,
                                                      uint32_t scale = 1, int max_iter = -1, double rms_eps = 1e-5)
    {
        const Frc3Info info = frc3_info(stream, len);
        const uint32_t k = scale >= 1 && scale <= 16 ? scale : 0; // the library refuses the scale itself
        rgb.assign((size_t)3 * k * info.width * k * info.height, 0);
        int it[3] = {0, 0, 0};
        double rms[3] = {0.0, 0.0, 0.0};
        check(frac_decode_frc3(ctx_, stream, len, scale, max_iter, rms_eps, rgb.data(), 3 * k * info.width, rgb.size(),
                               it, rms));
        return {{{it[0], rms[0]}, {it[1], rms[1]}, {it[2], rms[2]}}};
    }
    std::array<std::pair<int, double>, 3> decode_frc3(const std::vector<uint8_t>& stream, std::vector<uint8_t>& rgb,
                                                      uint32_t scale = 1, int max_iter = -1, double rms_eps = 1e-5)
    {
        return decode_frc3(stream.data(), stream.size(), rgb, scale, max_iter, rms_eps);
    }

private:
    void check(int rc) const
    {
        if (rc != FRAC_OK)
            throw Error(std::string("fracenc: ") + frac_last_error(ctx_));
    }
    frac_ctx* ctx_ = nullptr;
    uint32_t w_ = 0, h_ = 0;
    uint32_t rate_min_ = 0; // quadtreeRate's min_size: rateLeaves' worst-case capacity
};

// EncodingEngineCore2's role with batch claims.  One engine per entry of `devices` (a device
// may repeat: several contexts and streams on one GPU), each on its own host thread; the frame
// and domain grid are set once per engine, then every engine claims `batch` ranges at a time.
class EncodingEngineCore {
public:
    EncodingEngineCore(const Params& p, std::vector<int> devices, size_t batch = 65536)
        : params_(p), batch_(batch ? batch : 1)
    {
        if (devices.empty())
            devices.push_back(0);
        for (int d : devices)
            engines_.emplace_back(d, p);
    }

    size_t engineCount() const { return engines_.size(); }

    std::vector<frac_encode_item> encode(const uint8_t* plane, uint32_t w, uint32_t h, uint32_t stride,
                                         const std::vector<frac_grid_item>& domains,
                                         const std::vector<frac_grid_item>& ranges, frac_stats* total = nullptr)
    {
        std::vector<frac_encode_item> out(ranges.size());
        std::atomic<size_t> next{0};
        std::mutex m;
        frac_stats sum{};
        std::string err;
        auto worker = [&](Engine& e) {
            try {
                e.setFrame(plane, w, h, stride);
                e.setDomains(domains);
                for (;;) {
                    const size_t b0 = next.fetch_add(batch_);
                    if (b0 >= ranges.size())
                        break;
                    const size_t nb = std::min(batch_, ranges.size() - b0);
                    e.setRanges(ranges.data() + b0, nb);
                    e.run();
                    frac_stats st{};
                    e.fetch(out.data() + b0, &st);
                    std::lock_guard<std::mutex> lk(m);
                    sum.rejected_mappings += st.rejected_mappings;
                    sum.total_mappings += st.total_mappings;
                    sum.hit_ranges += st.hit_ranges;
                    sum.fallback_ranges += st.fallback_ranges;
                    sum.empty_ranges += st.empty_ranges;
                    sum.engine = st.engine;
                    sum.search_form = st.search_form;
                    sum.matrix_flops += st.matrix_flops;
                    sum.evaluated_mappings += st.evaluated_mappings;
                }
            } catch (const std::exception& ex) {
                std::lock_guard<std::mutex> lk(m);
                err = ex.what();
                next.store(ranges.size()); // stop the other engines' claims
            }
        };
        std::vector<std::thread> pool;
        for (auto& e : engines_)
            pool.emplace_back(worker, std::ref(e));
        for (auto& t : pool)
            t.join();
        if (!err.empty())
            throw Error(err);
        if (total)
            *total = sum;
        return out;
    }

private:
    Params params_;
    size_t batch_;
    std::vector<Engine> engines_;
};

// Frac::Quantizer<T> (encode/Quantizer.hpp:7-45).  value() is computed as the FMA-built
// reference does: fl(fma(q, step, min) + step/2) (GCC contracts q·step + min).
template <typename T>
class Quantizer {
public:
    using Int = uint64_t;
    Quantizer(T minValue, T maxValue, int numberOfBits)
        : min_(minValue), max_(maxValue), bits_(numberOfBits),
          step_(std::abs(maxValue - minValue) / (T)((Int)1 << numberOfBits)),
          maxQuantized_(((Int)1 << numberOfBits) - 1)
    {
        if (!(maxValue > minValue) || numberOfBits <= 1 || numberOfBits > 63)
            throw Error("Quantizer: needs max > min and 1 < bits < 64 (Quantizer.hpp:19-22)");
    }
    Int quantized(T value) const
    {
        const T q = std::floor((value - min_) / step_);
        return std::min(maxQuantized_, (Int)q);
    }
    T value(Int quant) const { return std::fma((T)quant, step_, min_) + step_ / 2; }
    T step() const { return step_; }

private:
    T min_, max_;
    int bits_;
    T step_;
    Int maxQuantized_;
};

} // namespace fracenc
