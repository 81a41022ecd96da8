// fracenc_codec.hip — the decoders (items, a run's results, FRC1 / FRQ1 streams iteratively or once against a
// reference plane, FRC3 colour containers), the stream packers and parsers, and the colour conversion entry points.
// Included by fracenc_api.hip.
extern "C" {

int frac_rgb_to_yuv_device(frac_ctx* c, const void* d_rgb, uint32_t w, uint32_t h, uint32_t rgb_stride, void* d_y,
                           uint32_t y_stride, void* d_u, uint32_t u_stride, void* d_v, uint32_t v_stride)
{
    if (!c)
        return FRAC_E_INVALID;
    if (w == 0 || h == 0)
        return FRAC_OK;
    if (!d_rgb || !d_y || ((w >= 2 && h >= 2) && (!d_u || !d_v)) || rgb_stride < 3ull * w || y_stride < w ||
        (w >= 2 && h >= 2 && (u_stride < w / 2 || v_stride < w / 2)))
        return c->fail(FRAC_E_INVALID, "rgb_to_yuv: invalid plane pointers or strides");
    FRAC_HIP(c, hipSetDevice(c->device));
    ColorArgs a;
    a.rgb = static_cast<const uint8_t*>(d_rgb);
    a.w = w;
    a.h = h;
    a.rgb_stride = rgb_stride;
    a.y = static_cast<uint8_t*>(d_y);
    a.ys = y_stride;
    a.u = static_cast<uint8_t*>(d_u);
    a.us = u_stride;
    a.v = static_cast<uint8_t*>(d_v);
    a.vs = v_stride;
    if (color_fast_path(a)) {
        const size_t n = (size_t)(w / 4) * (h / 2);
        rgb2yuv_quads4<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(a);
    } else {
        const size_t n = (size_t)((w + 1) / 2) * ((h + 1) / 2);
        rgb2yuv_generic<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(a);
    }
    FRAC_HIP(c, hipGetLastError());
    return FRAC_OK;
}

int frac_rgb_to_yuv(frac_ctx* c, const uint8_t* rgb, uint32_t w, uint32_t h, uint32_t rgb_stride, uint8_t* y,
                    uint8_t* u, uint8_t* v)
{
    if (!c)
        return FRAC_E_INVALID;
    if (w == 0 || h == 0)
        return FRAC_OK;
    if (!rgb || !y || (w >= 2 && h >= 2 && (!u || !v)) || rgb_stride < 3ull * w)
        return c->fail(FRAC_E_INVALID, "rgb_to_yuv: invalid buffers");
    FRAC_HIP(c, hipSetDevice(c->device));
    const uint32_t cw = w / 2, ch = h / 2;
    const uint32_t ys = plane_pitch(w), cs = plane_pitch(cw);
    const size_t rgb_bytes = (size_t)rgb_stride * h, y_bytes = (size_t)ys * h, c_bytes = (size_t)cs * std::max(ch, 1u);
    FRAC_HIP(c, c->d_color.ensure(rgb_bytes + y_bytes + 2 * c_bytes));
    uint8_t* d_rgb = c->d_color.ptr;
    uint8_t* d_y = d_rgb + rgb_bytes;
    uint8_t* d_u = d_y + y_bytes;
    uint8_t* d_v = d_u + c_bytes;
    FRAC_HIP(c, hipMemcpyAsync(d_rgb, rgb, rgb_bytes, hipMemcpyHostToDevice, c->stream));
    FRAC_TRY(frac_rgb_to_yuv_device(c, d_rgb, w, h, rgb_stride, d_y, ys, d_u, cs, d_v, cs));
    FRAC_HIP(c, hipMemcpy2DAsync(y, w, d_y, ys, w, h, hipMemcpyDeviceToHost, c->stream));
    if (cw && ch) {
        FRAC_HIP(c, hipMemcpy2DAsync(u, cw, d_u, cs, cw, ch, hipMemcpyDeviceToHost, c->stream));
        FRAC_HIP(c, hipMemcpy2DAsync(v, cw, d_v, cs, cw, ch, hipMemcpyDeviceToHost, c->stream));
    }
    FRAC_HIP(c, hipStreamSynchronize(c->stream));
    return FRAC_OK;
}

// The conversion back, enqueued on the context's stream, with chroma planes of their own size cw × ch
// (frac_yuv_to_rgb_device passes w/2 × h/2; a scaled decode of an odd frame has narrower ones).
static int yuv_to_rgb_launch(frac_ctx* c, const void* d_y, uint32_t w, uint32_t h, uint32_t y_stride, const void* d_u,
                             uint32_t u_stride, const void* d_v, uint32_t v_stride, uint32_t cw, uint32_t ch,
                             void* d_rgb, uint32_t rgb_stride)
{
    if (w < 2 || h < 2 || cw == 0 || ch == 0)
        return c->fail(FRAC_E_INVALID, "yuv_to_rgb: a frame below 2 pixels a side has no chroma plane");
    if (!d_y || !d_u || !d_v || !d_rgb || rgb_stride < 3ull * w || y_stride < w || u_stride < cw || v_stride < cw)
        return c->fail(FRAC_E_INVALID, "yuv_to_rgb: invalid plane pointers or strides");
    FRAC_HIP(c, hipSetDevice(c->device));
    YuvArgs a;
    a.y = static_cast<const uint8_t*>(d_y);
    a.w = w;
    a.h = h;
    a.ys = y_stride;
    a.u = static_cast<const uint8_t*>(d_u);
    a.us = u_stride;
    a.v = static_cast<const uint8_t*>(d_v);
    a.vs = v_stride;
    a.cw = cw;
    a.ch = ch;
    a.rgb = static_cast<uint8_t*>(d_rgb);
    a.rgb_stride = rgb_stride;
    if (yuv_fast_path(a)) {
        const size_t n = (size_t)(w / 4) * (h / 2);
        yuv2rgb_quads4<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(a);
    } else {
        const size_t n = (size_t)((w + 1) / 2) * ((h + 1) / 2);
        yuv2rgb_generic<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(a);
    }
    FRAC_HIP(c, hipGetLastError());
    return FRAC_OK;
}

int frac_yuv_to_rgb_device(frac_ctx* c, const void* d_y, uint32_t w, uint32_t h, uint32_t y_stride, const void* d_u,
                           uint32_t u_stride, const void* d_v, uint32_t v_stride, void* d_rgb, uint32_t rgb_stride)
{
    if (!c)
        return FRAC_E_INVALID;
    return yuv_to_rgb_launch(c, d_y, w, h, y_stride, d_u, u_stride, d_v, v_stride, w / 2, h / 2, d_rgb, rgb_stride);
}

int frac_yuv_to_rgb(frac_ctx* c, const uint8_t* y, const uint8_t* u, const uint8_t* v, uint32_t w, uint32_t h,
                    uint8_t* rgb, uint32_t rgb_stride)
{
    if (!c)
        return FRAC_E_INVALID;
    if (w < 2 || h < 2)
        return c->fail(FRAC_E_INVALID, "yuv_to_rgb: a frame below 2 pixels a side has no chroma plane");
    if (!y || !u || !v || !rgb || rgb_stride < 3ull * w)
        return c->fail(FRAC_E_INVALID, "yuv_to_rgb: invalid buffers");
    FRAC_HIP(c, hipSetDevice(c->device));
    const uint32_t cw = w / 2, ch = h / 2;
    const uint32_t ys = plane_pitch(w), cs = plane_pitch(cw), rs = plane_pitch(3 * w);
    const size_t y_bytes = (size_t)ys * h, c_bytes = (size_t)cs * ch, rgb_bytes = (size_t)rs * h;
    FRAC_HIP(c, c->d_color.ensure(rgb_bytes + y_bytes + 2 * c_bytes));
    uint8_t* d_rgb = c->d_color.ptr;
    uint8_t* d_y = d_rgb + rgb_bytes;
    uint8_t* d_u = d_y + y_bytes;
    uint8_t* d_v = d_u + c_bytes;
    FRAC_HIP(c, hipMemcpy2DAsync(d_y, ys, y, w, w, h, hipMemcpyHostToDevice, c->stream));
    FRAC_HIP(c, hipMemcpy2DAsync(d_u, cs, u, cw, cw, ch, hipMemcpyHostToDevice, c->stream));
    FRAC_HIP(c, hipMemcpy2DAsync(d_v, cs, v, cw, cw, ch, hipMemcpyHostToDevice, c->stream));
    FRAC_TRY(yuv_to_rgb_launch(c, d_y, w, h, ys, d_u, cs, d_v, cs, cw, ch, d_rgb, rs));
    FRAC_HIP(c, hipMemcpy2DAsync(rgb, rgb_stride, d_rgb, rs, 3ull * w, h, hipMemcpyDeviceToHost, c->stream));
    FRAC_HIP(c, hipStreamSynchronize(c->stream));
    return FRAC_OK;
}

// Do the items (x, y, w, h) cover the w×h plane exactly once?  Checked on a bitmap of cells of
// the smallest item size (every item a multiple of it, aligned), so O(cells), not O(pixels).
static bool covers_exactly(const std::vector<frac_grid_item>& rects, uint32_t w, uint32_t h)
{
    if (rects.empty())
        return false;
    uint32_t g = ~0u;
    for (const auto& r : rects) {
        if (r.w == 0 || r.w != r.h)
            return false;
        g = std::min(g, r.w);
    }
    if (w % g || h % g)
        return false;
    const uint32_t cw = w / g, ch = h / g;
    std::vector<uint8_t> cell((size_t)cw * ch, 0);
    size_t covered = 0;
    for (const auto& r : rects) {
        if (r.x % g || r.y % g || r.w % g || (uint64_t)r.x + r.w > w || (uint64_t)r.y + r.h > h)
            return false;
        for (uint32_t y = r.y / g; y < (r.y + r.h) / g; ++y)
            for (uint32_t x = r.x / g; x < (r.x + r.w) / g; ++x) {
                if (cell[(size_t)y * cw + x]++)
                    return false;
                ++covered;
            }
    }
    return covered == cell.size();
}

// The fused decoders' loop: `step(src, tgt, stride)` enqueues one iteration that writes every pixel of tgt
// from src and adds its (source − new)² sums to the kDecodeSlots slots (decode_fused over items, frc1dec_step
// over a stream's records); decode_check, the buffer swap and the host's look at the flag every few steps
// are shared.
// Where a decode's plane comes from and goes to.  The initial target is a host plane (stride w) or, absent,
// zeros; the decoded plane goes to a host plane (stride w; the call returns synchronised), or stays on the
// device, copied to d_out with its pitch on the context's stream, or goes nowhere: `final` then learns which
// decoder buffer holds it, and its pitch, once the context's stream has run (fracenc_quality.hip compares it
// with the frame there).
struct PlaneIO {
    const uint8_t* h_init = nullptr;
    uint8_t* h_out = nullptr;
    uint8_t* d_out = nullptr;
    uint32_t d_pitch = 0;
    struct Final {
        const uint8_t* ptr = nullptr;
        uint32_t pitch = 0;
    }* final = nullptr;
    bool valid() const { return h_out || d_out || final; }
};
// the public decoders' plane: host in, host out
static PlaneIO host_plane(uint8_t* plane)
{
    PlaneIO io;
    io.h_init = io.h_out = plane;
    return io;
}

// the decoded plane `fin` (on the device, row pitch `stride`) to its destination
static int decode_deliver(frac_ctx* c, const PlaneIO& io, const uint8_t* fin, uint32_t stride, uint32_t w, uint32_t h)
{
    if (io.final) {
        io.final->ptr = fin;
        io.final->pitch = stride;
    } else if (io.h_out) {
        FRAC_HIP(c, hipMemcpy2DAsync(io.h_out, w, fin, stride, w, h, hipMemcpyDeviceToHost, c->stream));
        FRAC_HIP(c, hipStreamSynchronize(c->stream));
    } else {
        FRAC_TRY(copy_plane(c, io.d_out, io.d_pitch, fin, stride, w, h, hipMemcpyDeviceToDevice, c->stream));
    }
    FRAC_HIP(c, hipGetLastError());
    return FRAC_OK;
}

extern "C++" template <class Step>
static int decode_fused_loop(frac_ctx* c, uint32_t w, uint32_t h, int iters, double eps, const PlaneIO& io,
                             int* iterations, double* rms, Step&& step)
{
    const uint32_t stride = plane_pitch(w);
    const size_t bytes = (size_t)stride * (h + 1);
    FRAC_HIP(c, c->d_dec_src.ensure(bytes));
    FRAC_HIP(c, c->d_dec_tgt.ensure(bytes));
    FRAC_HIP(c, c->d_dec_part.ensure(kDecodeSlots));
    FRAC_HIP(c, hipMemsetAsync(c->d_dec_part.ptr, 0, kDecodeSlots * sizeof(unsigned long long), c->stream));
    FRAC_HIP(c, c->d_dec_state.ensure(1));
    FRAC_HIP(c, c->h_dec_state.ensure());
    uint8_t* buf[2] = {c->d_dec_src.ptr, c->d_dec_tgt.ptr};
    FRAC_HIP(c, hipMemsetAsync(buf[0], 100, bytes, c->stream)); // Decoder2: source filled with 100
    FRAC_HIP(c, hipMemsetAsync(buf[1], 0, bytes, c->stream));
    if (io.h_init)
        FRAC_HIP(c, hipMemcpy2DAsync(buf[1], stride, io.h_init, w, w, h, hipMemcpyHostToDevice, c->stream));
    FRAC_HIP(c, hipMemsetAsync(c->d_dec_state.ptr, 0, sizeof(DecodeState), c->stream));
    constexpr int kChunk = 8; // iterations enqueued between host checks of the convergence flag
    int enq = 0;
    while (enq < iters) {
        const int stop = std::min(iters, enq + kChunk);
        for (; enq < stop; ++enq) {
            step(buf[enq & 1], buf[(enq + 1) & 1], stride);
            decode_check<<<1, kDecodeSlots, 0, c->stream>>>(c->d_dec_part.ptr, (uint64_t)w * h, eps, enq, iters - 1,
                                                            c->d_dec_state.ptr);
        }
        FRAC_HIP(c, hipMemcpyAsync(c->h_dec_state.ptr, c->d_dec_state.ptr, sizeof(DecodeState), hipMemcpyDeviceToHost,
                                   c->stream));
        FRAC_HIP(c, hipStreamSynchronize(c->stream));
        if (c->h_dec_state->done)
            break;
    }
    int it = 0;
    double r = 0.0;
    if (iters > 0) {
        it = c->h_dec_state->iterations;
        r = c->h_dec_state->rms;
    }
    // the final target: step `it` when the loop broke there, else step iters − 1
    const int last = iters > 0 ? (c->h_dec_state->done ? it : iters - 1) : -1;
    const uint8_t* fin = last >= 0 ? buf[(last + 1) & 1] : buf[1];
    FRAC_TRY(decode_deliver(c, io, fin, stride, w, h));
    if (iterations)
        *iterations = it;
    if (rms)
        *rms = r;
    return FRAC_OK;
}

// Fused decode (fracenc_decode.hip decode_fused / decode_check): the items tile the plane.
static int decode_fused_impl(frac_ctx* c, const frac_encode_item* d_items, size_t n, uint32_t w, uint32_t h,
                             int iters, double eps, const PlaneIO& io, int* iterations, double* rms)
{
    DecodeArgs a;
    a.items = d_items;
    a.n = (uint32_t)n;
    const uint32_t nblk = (uint32_t)((n + 3) / 4);
    return decode_fused_loop(c, w, h, iters, eps, io, iterations, rms,
                             [&](const uint8_t* src, uint8_t* tgt, uint32_t stride) {
                                 a.src = src;
                                 a.tgt = tgt;
                                 a.stride = stride;
                                 decode_fused<<<nblk, 256, 0, c->stream>>>(a, c->d_dec_state.ptr, c->d_dec_part.ptr);
                             });
}

static int decode_impl(frac_ctx* c, const frac_encode_item* d_items, size_t n, uint32_t w, uint32_t h, int max_iter,
                       double eps, const PlaneIO& io, int* iterations, double* rms, bool fused = false)
{
    if (!io.valid() || w == 0 || h == 0)
        return c->fail(FRAC_E_INVALID, "decode: invalid plane");
    FRAC_TRY(check_ab_knobs(c));
    if (fused &&!(c->p.flags & FRAC_FLAG_DECODE_STEPWISE) && ab_knob("FRAC_DECODE_UNFUSED") == nullptr)
        return decode_fused_impl(c, d_items, n, w, h, max_iter < 0 ? 300 : max_iter, eps, io, iterations, rms);
    const uint32_t stride = plane_pitch(w);
    const size_t bytes = (size_t)stride * (h + 1);
    FRAC_HIP(c, c->d_dec_src.ensure(bytes));
    FRAC_HIP(c, c->d_dec_tgt.ensure(bytes));
    FRAC_HIP(c, c->d_dec_sum.ensure(1));
    FRAC_HIP(c, c->h_dec_sum.ensure());
    // Decoder2::decode: source filled with 100, target = the caller's plane
    FRAC_HIP(c, hipMemsetAsync(c->d_dec_src.ptr, 100, bytes, c->stream));
    FRAC_HIP(c, hipMemsetAsync(c->d_dec_tgt.ptr, 0, bytes, c->stream));
    if (io.h_init)
        FRAC_HIP(c, hipMemcpy2DAsync(c->d_dec_tgt.ptr, stride, io.h_init, w, w, h, hipMemcpyHostToDevice, c->stream));
    const int iters = max_iter < 0 ? 300 : max_iter;
    DecodeArgs a;
    a.src = c->d_dec_src.ptr;
    a.tgt = c->d_dec_tgt.ptr;
    a.stride = stride;
    a.items = d_items;
    a.n = (uint32_t)n;
    const uint32_t rms_blocks = (uint32_t)std::min<size_t>(1024, ((size_t)w * h + 255) / 256);
    int i = 0;
    double r = 0.0;
    for (; i < iters; ++i) {
        if (n)
            decode_apply<<<(unsigned)((n + 3) / 4), 256, 0, c->stream>>>(a);
        FRAC_HIP(c, hipMemsetAsync(c->d_dec_sum.ptr, 0, sizeof(unsigned long long), c->stream));
        decode_rms<<<rms_blocks, 256, 0, c->stream>>>(c->d_dec_src.ptr, c->d_dec_tgt.ptr, w, h, stride, c->d_dec_sum.ptr);
        FRAC_HIP(c, hipMemcpyAsync(c->h_dec_sum.ptr, c->d_dec_sum.ptr, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                   c->stream));
        FRAC_HIP(c, hipStreamSynchronize(c->stream));
        // the reference accumulates in int32 (metrics.h:29): reproduce its wrap-around
        const int32_t s32 = (int32_t)(uint32_t)(*c->h_dec_sum.ptr & 0xffffffffull);
        r = (double)s32 / (double)((uint64_t)w * h);
        if (r < eps)
            break;
        FRAC_HIP(c, hipMemcpyAsync(c->d_dec_src.ptr, c->d_dec_tgt.ptr, bytes, hipMemcpyDeviceToDevice, c->stream));
    }
    FRAC_TRY(decode_deliver(c, io, c->d_dec_tgt.ptr, stride, w, h));
    if (iterations)
        *iterations = i;
    if (rms)
        *rms = r;
    return FRAC_OK;
}

int frac_decode(frac_ctx* c, const frac_encode_item* items, size_t n, uint32_t w, uint32_t h, int max_iter,
                double rms_eps, uint8_t* plane, int* iterations, double* rms)
{
    if (!c)
        return FRAC_E_INVALID;
    if (n && !items)
        return c->fail(FRAC_E_INVALID, "decode: items is NULL");
    for (size_t i = 0; i < n; ++i) {
        const frac_encode_item& e = items[i];
        if ((uint64_t)e.x + e.w > w || (uint64_t)e.y + e.h > h || e.match.score.transform < 0 ||
            e.match.score.transform > 7 ||
            (e.match.sw && ((uint64_t)e.match.x + e.match.sw > w || (uint64_t)e.match.y + e.match.sh > h)))
            return c->fail(FRAC_E_INVALID, "decode: item outside the plane or bad transform");
        // a rectangular (or degenerate) domain: the transformed 2×2 samples (Frac::copy's fit points,
        // DecodeUtils.hpp:9-25) may leave the patch; they must stay inside the plane
        if (e.match.sw && (e.match.sw != e.match.sh || e.match.sw < 2) &&
            (e.match.sw < 2 || e.match.sh < 2 || e.w == 0 || e.h == 0 ||
             !box_inside(sample_box(e.match.score.transform, (int)e.match.sw, (int)e.match.sh, (int)e.w, (int)e.h,
                                    false, true),
                         e.match.x, e.match.y, w, h)))
            return c->fail(FRAC_E_INVALID, "decode: a transformed sample of item " + std::to_string(i) +
                                               " falls outside the plane");
    }
    FRAC_HIP(c, hipSetDevice(c->device));
    FRAC_HIP(c, c->d_dec_items.ensure(n));
    if (n)
        FRAC_HIP(c, hipMemcpyAsync(c->d_dec_items.ptr, items, n * sizeof(frac_encode_item), hipMemcpyHostToDevice,
                                   c->stream));
    std::vector<frac_grid_item> rects(n);
    bool all_domains = true;
    for (size_t i = 0; i < n; ++i) {
        rects[i] = frac_grid_item{items[i].x, items[i].y, items[i].w, items[i].h, -1};
        all_domains = all_domains && items[i].match.sw != 0 && items[i].match.sh != 0;
    }
    const bool fused = all_domains && covers_exactly(rects, w, h);
    return decode_impl(c, c->d_dec_items.ptr, n, w, h, max_iter, rms_eps, host_plane(plane), iterations, rms, fused);
}

int frac_decode_results(frac_ctx* c, uint32_t w, uint32_t h, int max_iter, double rms_eps, uint8_t* plane,
                        int* iterations, double* rms)
{
    if (!c)
        return FRAC_E_INVALID;
    if (!c->ran)
        return c->fail(FRAC_E_STATE, "decode: frac_run has not been called");
    if (c->src.w > w || c->src.h > h || c->tgt.w > w || c->tgt.h > h)
        return c->fail(FRAC_E_INVALID, "decode: plane smaller than the encoded planes");
    FRAC_HIP(c, hipSetDevice(c->device));
    FRAC_TRY(settle_fallback(c));
    // the fused form needs every range written: no empty (domain-less) record among the results
    bool fused = covers_exactly(c->ranges, w, h);
    if (fused && !c->ranges.empty()) {
        c->h_aux.resize(nranges(c));
        FRAC_HIP(c, hipMemcpyAsync(c->h_aux.data(), c->d_aux.ptr, nranges(c) * sizeof(RangeAux),
                                   hipMemcpyDeviceToHost, c->stream));
        FRAC_HIP(c, hipStreamSynchronize(c->stream));
        for (const RangeAux& x : c->h_aux)
            if (x.flags & kAuxEmpty) {
                fused = false;
                break;
            }
    }
    return decode_impl(c, c->d_out.ptr, nranges(c), w, h, max_iter, rms_eps, host_plane(plane), iterations, rms, fused);
}

int frac_pack_frc1(frac_ctx* c, uint32_t cbits, uint32_t bbits, uint8_t* out, size_t cap, size_t* n_out)
{
    if (!c)
        return FRAC_E_INVALID;
    if (!n_out)
        return c->fail(FRAC_E_INVALID, "pack_frc1: n_out is NULL");
    if (!c->ran)
        return c->fail(FRAC_E_STATE, "pack_frc1: frac_run has not been called");
    if (cbits < 2 || cbits > 16 || bbits < 2 || bbits > 16)
        return c->fail(FRAC_E_INVALID, "pack_frc1: contrast/brightness bits must be in [2, 16]");
    const uint32_t W = c->tgt.w, H = c->tgt.h, n = (uint32_t)c->n;
    if (c->src.w != W || c->src.h != H)
        return c->fail(FRAC_E_INVALID, "pack_frc1: source and target planes must have one size");
    // the stream's implicit geometry: createUniformGrid ranges (row-major) and domains
    // (compared item by item against the closed-form lattice, without building it: at C3 the two grids
    // hold 0.5 M items)
    auto same_grid = [&](const std::vector<frac_grid_item>& g, uint32_t size, uint32_t off) {
        const size_t cnt = frac_uniform_grid(W, H, size, off, nullptr, 0);
        if (cnt != g.size())
            return false;
        if (!cnt)
            return true;
        const size_t cols = (W - size) / off + 1;
        const frac_grid_item* it = g.data();
        for (size_t r = 0, k = 0; k < cnt; ++r)
            for (size_t q = 0; q < cols; ++q, ++k, ++it)
                if (it->x != q * off || it->y != r * off || it->w != size || it->h != size)
                    return false;
        return true;
    };
    if (n == 0)
        return c->fail(FRAC_E_INVALID, "pack_frc1: the stream holds square items only");
    if (!same_grid(c->ranges, n, n))
        return c->fail(FRAC_E_INVALID, "pack_frc1: ranges are not the row-major range grid");
    if (!same_grid(c->doms, 2 * n, n))
        return c->fail(FRAC_E_INVALID, "pack_frc1: domains are not the domain lattice (size 2n, stride n)");
    const uint32_t nr = (uint32_t)nranges(c), nd = (uint32_t)c->doms.size(), T = c->p.transforms;
    auto bitlen = [](uint64_t v) { uint32_t b = 0; while (v) { ++b; v >>= 1; } return b; };
    const uint32_t ib = std::max(1u, bitlen(nd)), tb = std::max(1u, bitlen(T - 1));
    const uint32_t width = ib + tb + cbits + bbits;
    if (width > 64)
        return c->fail(FRAC_E_INVALID, "pack_frc1: record wider than 64 bits");
    const uint64_t body = ((uint64_t)nr * width + 7) / 8, nwords = ((uint64_t)nr * width + 31) / 32;
    *n_out = FRAC_FRC1_HEADER_BYTES + body;
    if (!out)
        return FRAC_OK;
    FRAC_HIP(c, hipSetDevice(c->device));
    FRAC_TRY(settle_fallback(c));
    Frc1MinMax mm{~0ull, 0ull, ~0ull, 0ull};
    std::vector<uint32_t> words(nwords);
    if (nr) {
        FRAC_HIP(c, c->d_frc_mm.ensure(1));
        FRAC_HIP(c, c->d_frc_rec.ensure(nr));
        FRAC_HIP(c, c->d_frc_words.ensure(nwords));
        FRAC_HIP(c, hipMemsetAsync(c->d_frc_mm.ptr, 0xff, sizeof(unsigned long long), c->stream));
        FRAC_HIP(c, hipMemsetAsync(&c->d_frc_mm.ptr->cmax, 0, sizeof(unsigned long long), c->stream));
        FRAC_HIP(c, hipMemsetAsync(&c->d_frc_mm.ptr->bmin, 0xff, sizeof(unsigned long long), c->stream));
        FRAC_HIP(c, hipMemsetAsync(&c->d_frc_mm.ptr->bmax, 0, sizeof(unsigned long long), c->stream));
        frc1_minmax<<<std::min<uint32_t>(1024, (nr + 255) / 256), 256, 0, c->stream>>>(c->d_out.ptr, nr,
                                                                                          c->d_frc_mm.ptr);
        Frc1Args a;
        a.out = c->d_out.ptr;
        a.n = nr;
        a.dstride = n;
        a.dcols = (uint32_t)((W - 2 * n) / n + 1);
        a.ndomains = nd;
        a.index_bits = ib;
        a.t_bits = tb;
        a.c_bits = cbits;
        a.b_bits = bbits;
        a.mm = c->d_frc_mm.ptr;
        a.rec = c->d_frc_rec.ptr;
        frc1_records<<<(nr + 255) / 256, 256, 0, c->stream>>>(a);
        frc1_words<<<(unsigned)((nwords + 255) / 256), 256, 0, c->stream>>>(c->d_frc_rec.ptr, nr, width, nwords,
                                                                             c->d_frc_words.ptr);
        FRAC_HIP(c, hipGetLastError());
        FRAC_HIP(c, hipMemcpyAsync(&mm, c->d_frc_mm.ptr, sizeof(mm), hipMemcpyDeviceToHost, c->stream));
        FRAC_HIP(c, hipMemcpyAsync(words.data(), c->d_frc_words.ptr, nwords * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                   c->stream));
        FRAC_HIP(c, hipStreamSynchronize(c->stream));
    }
    // header "<4sHHIIIIIBBBBIIdddd" (fractencode_amd/codec.py)
    uint8_t hdr[FRAC_FRC1_HEADER_BYTES] = {};
    size_t o = 0;
    auto put = [&](const void* v, size_t k) { std::memcpy(hdr + o, v, k); o += k; };
    const uint16_t version = 1, flags = c->p.use_classifier ? 1 : 0;
    const uint32_t u32s[5] = {W, H, n, 2 * n, n};
    const uint8_t u8s[4] = {(uint8_t)T, (uint8_t)cbits, (uint8_t)bbits, (uint8_t)ib};
    const uint32_t counts[2] = {nr, nd};
    const double mm_d[4] = {nr ? dkey_inv(mm.cmin) : 0.0, nr ? dkey_inv(mm.cmax) : 0.0, nr ? dkey_inv(mm.bmin) : 0.0,
                            nr ? dkey_inv(mm.bmax) : 0.0};
    put("FRC1", 4);
    put(&version, 2);
    put(&flags, 2);
    put(u32s, sizeof(u32s));
    put(u8s, sizeof(u8s));
    put(counts, sizeof(counts));
    put(mm_d, sizeof(mm_d));
    const size_t total = FRAC_FRC1_HEADER_BYTES + body;
    std::memcpy(out, hdr, std::min<size_t>(cap, FRAC_FRC1_HEADER_BYTES));
    if (cap > FRAC_FRC1_HEADER_BYTES)
        std::memcpy(out + FRAC_FRC1_HEADER_BYTES, words.data(), std::min<size_t>(cap, total) - FRAC_FRC1_HEADER_BYTES);
    return FRAC_OK;
}

// The FRC1 header "<4sHHIIIIIBBBBIIdddd" (fractencode_amd/codec.py) parsed and checked against the stream
// length; on failure `msg` names the rule.
using Frc1Info = struct frac_frc1_info; // the plain name is the function's
static int frc1_parse(const uint8_t* s, size_t len, Frc1Info* o, std::string& msg)
{
    auto bad = [&](const char* why) {
        msg = std::string("FRC1: ") + why;
        return FRAC_E_INVALID;
    };
    if (!s || !o)
        return bad("NULL argument");
    if (len < FRAC_FRC1_HEADER_BYTES)
        return bad("truncated header");
    uint16_t version, flags;
    uint32_t u[5], counts[2];
    double mm[4];
    std::memcpy(&version, s + 4, 2);
    std::memcpy(&flags, s + 6, 2);
    std::memcpy(u, s + 8, sizeof(u));
    std::memcpy(counts, s + 32, sizeof(counts));
    std::memcpy(mm, s + 40, sizeof(mm));
    if (std::memcmp(s, "FRC1", 4) != 0 || version != 1)
        return bad("bad magic or version");
    *o = Frc1Info{};
    o->width = u[0], o->height = u[1], o->range_size = u[2], o->domain_size = u[3], o->domain_stride = u[4];
    o->transforms = s[28], o->contrast_bits = s[29], o->brightness_bits = s[30], o->index_bits = s[31];
    o->n_ranges = counts[0], o->n_domains = counts[1], o->flags = flags;
    o->contrast_min = mm[0], o->contrast_max = mm[1], o->brightness_min = mm[2], o->brightness_max = mm[3];
    if (o->width == 0 || o->height == 0 || o->range_size == 0)
        return bad("zero width, height or range size");
    if (o->domain_size < 2 || (o->domain_size & 1u) || o->domain_stride != o->domain_size / 2)
        return bad("domain size must be even and at least 2, its stride half of it");
    if (o->transforms < 1 || o->transforms > 8)
        return bad("transforms outside 1..8");
    if (o->contrast_bits < 2 || o->contrast_bits > 24 || o->brightness_bits < 2 || o->brightness_bits > 24)
        return bad("contrast / brightness bits outside [2, 24]");
    auto bitlen = [](uint64_t v) { uint32_t b = 0; while (v) { ++b; v >>= 1; } return b; };
    if (o->index_bits != std::max(1u, bitlen(o->n_domains)))
        return bad("index bits do not match the domain count");
    o->record_bits = o->index_bits + std::max(1u, bitlen(o->transforms - 1)) + o->contrast_bits + o->brightness_bits;
    if (o->record_bits > 64)
        return bad("record wider than 64 bits");
    if (o->n_ranges != frac_uniform_grid(o->width, o->height, o->range_size, o->range_size, nullptr, 0))
        return bad("range count is not the range grid's");
    if (o->n_domains != frac_uniform_grid(o->width, o->height, o->domain_size, o->domain_stride, nullptr, 0))
        return bad("domain count is not the domain grid's");
    o->body_bytes = ((uint64_t)o->n_ranges * o->record_bits + 7) / 8;
    if (len - FRAC_FRC1_HEADER_BYTES < o->body_bytes)
        return bad("truncated records");
    for (double v : mm)
        if (!std::isfinite(v))
            return bad("non-finite quantizer bound");
    return FRAC_OK;
}

int frac_frc1_info(const uint8_t* stream, size_t len, struct frac_frc1_info* out)
{
    std::string msg;
    const int rc = frc1_parse(stream, len, out, msg);
    if (rc != FRAC_OK)
        g_last_error = msg;
    return rc;
}

// A parsed FRC1 stream's records on the device, validated: what the iterative and the inter decoders share.
struct Frc1Device {
    Frc1Layout L{};
    uint32_t n = 0;     // records, in d_frc_rec
    bool tiles = false; // the ranges tile the frame and every range has a domain
    bool fast = false;  // the step kernels' geometry: tiles, domain side twice the range side, no stepwise flag
};

// The record pass of the parsed stream `h` (records at stream + 72): the layout by value, the records unpacked
// into d_frc_rec and their indices checked.  Blocks for the status word; FRAC_E_INVALID for an index above the
// domain count, before anything else has been launched.
static int frc1_records_device(frac_ctx* c, const Frc1Info& h, const uint8_t* stream, Frc1Device* d)
{
    const uint32_t n = h.n_ranges;
    Frc1Layout& L = d->L;
    L = Frc1Layout{};
    L.n_ranges = n;
    L.n_domains = h.n_domains;
    L.rcols = n ? (h.width - h.range_size) / h.range_size + 1 : 0;
    L.dcols = h.n_domains ? (h.width - h.domain_size) / h.domain_stride + 1 : 0;
    L.range_size = h.range_size;
    L.domain_size = h.domain_size;
    L.domain_stride = h.domain_stride;
    L.index_bits = h.index_bits;
    L.c_bits = h.contrast_bits;
    L.b_bits = h.brightness_bits;
    L.t_bits = h.record_bits - h.index_bits - h.contrast_bits - h.brightness_bits;
    L.record_bits = h.record_bits;
    // Quantizer (encode/Quantizer.hpp:19-22): step = |max − min| / 2^bits; !(max > min): every code is min
    auto step = [](double lo, double hi, uint32_t bits) {
        return hi > lo ? std::fabs(hi - lo) / (double)(1u << bits) : 0.0;
    };
    L.c_step = step(h.contrast_min, h.contrast_max, h.contrast_bits);
    L.c_min = h.contrast_min;
    L.b_step = step(h.brightness_min, h.brightness_max, h.brightness_bits);
    L.b_min = h.brightness_min;

    FRAC_HIP(c, hipSetDevice(c->device));
    // record pass: reads only the stream buffer (the body and kFrc1PadWords zeroed dwords after it)
    uint32_t status[2] = {0, 0};
    if (n) {
        const size_t body_words = (size_t)((h.body_bytes + 3) / 4);
        FRAC_HIP(c, c->d_frc_in.ensure(body_words + kFrc1PadWords));
        FRAC_HIP(c, c->d_frc_rec.ensure(n));
        FRAC_HIP(c, c->d_frc_status.ensure(2));
        // from the body's last whole dword on: its tail bytes and the padding
        FRAC_HIP(c, hipMemsetAsync(c->d_frc_in.ptr + (body_words - 1), 0, (1 + kFrc1PadWords) * sizeof(uint32_t),
                                   c->stream));
        FRAC_HIP(c, hipMemsetAsync(c->d_frc_status.ptr, 0, sizeof(status), c->stream));
        FRAC_HIP(c, hipMemcpyAsync(c->d_frc_in.ptr, stream + FRAC_FRC1_HEADER_BYTES, (size_t)h.body_bytes,
                                   hipMemcpyHostToDevice, c->stream));
        frc1dec_records<<<(n + 255) / 256, 256, 0, c->stream>>>(c->d_frc_in.ptr, L, c->d_frc_rec.ptr,
                                                                 c->d_frc_status.ptr);
        FRAC_HIP(c, hipGetLastError());
        FRAC_HIP(c, hipMemcpyAsync(status, c->d_frc_status.ptr, sizeof(status), hipMemcpyDeviceToHost, c->stream));
        FRAC_HIP(c, hipStreamSynchronize(c->stream));
        if (status[0])
            return c->fail(FRAC_E_INVALID, "FRC1: domain index out of range");
    }
    d->n = n;
    d->tiles = n && h.width % h.range_size == 0 && h.height % h.range_size == 0 && status[1] == 0;
    d->fast = d->tiles && h.domain_size == 2 * h.range_size && !(c->p.flags & FRAC_FLAG_DECODE_STEPWISE);
    return FRAC_OK;
}

// the step kernels' arguments of a stream on their geometry at `scale`, but for the planes
static Frc1StepArgs frc1_step_args(frac_ctx* c, const Frc1Info& h, uint32_t scale)
{
    Frc1StepArgs a{};
    a.w = scale * h.width;
    a.h = scale * h.height;
    a.R = scale * h.range_size;
    a.rrows = h.height / h.range_size;
    a.scale = scale;
    a.rec = c->d_frc_rec.ptr;
    return a;
}

// frac_decode_frc1 past its argument checks: the parsed stream `h` (records at stream + 72) decoded at `scale`
// (checked by the caller) from and to `io`.
static int decode_frc1_parsed(frac_ctx* c, const Frc1Info& h, const uint8_t* stream, uint32_t scale, int max_iter,
                              double rms_eps, const PlaneIO& io, int* iterations, double* rms)
{
    const uint32_t W = scale * h.width, H = scale * h.height;
    Frc1Device d;
    FRAC_TRY(frc1_records_device(c, h, stream, &d));
    const Frc1Layout& L = d.L;
    const uint32_t n = d.n;
    const bool tiles = d.tiles;
    if (d.fast) {
        Frc1StepArgs a = frc1_step_args(c, h, scale);
        const dim3 grid((W + kFrc1TileW - 1) / kFrc1TileW, (H + kFrc1TileH - 1) / kFrc1TileH);
        return decode_fused_loop(c, W, H, max_iter < 0 ? 300 : max_iter, rms_eps, io, iterations, rms,
                                 [&](const uint8_t* src, uint8_t* tgt, uint32_t stride) {
                                     a.src = src;
                                     a.tgt = tgt;
                                     a.stride = stride;
                                     frc1dec_step<<<grid, 256, 0, c->stream>>>(a, L, c->d_dec_state.ptr,
                                                                               c->d_dec_part.ptr);
                                 });
    }
    // every other stream: the records as scaled encode items, through the item decoder (fused when they
    // tile the plane and every range has a domain, as frac_decode decides)
    FRAC_HIP(c, c->d_dec_items.ensure(n));
    if (n) {
        frc1dec_expand<<<(n + 255) / 256, 256, 0, c->stream>>>(c->d_frc_rec.ptr, L, scale, c->d_dec_items.ptr);
        FRAC_HIP(c, hipGetLastError());
    }
    return decode_impl(c, c->d_dec_items.ptr, n, W, H, max_iter, rms_eps, io, iterations, rms, tiles);
}

int frac_decode_frc1(frac_ctx* c, const uint8_t* stream, size_t len, uint32_t scale, int max_iter, double rms_eps,
                     uint8_t* plane, size_t plane_bytes, int* iterations, double* rms)
{
    if (!c)
        return FRAC_E_INVALID;
    Frc1Info h;
    {
        std::string msg;
        if (frc1_parse(stream, len, &h, msg) != FRAC_OK)
            return c->fail(FRAC_E_INVALID, msg);
    }
    FRAC_TRY(check_ab_knobs(c));
    if (scale < 1 || scale > 16 || (uint64_t)scale * h.width > 65535 || (uint64_t)scale * h.height > 65535)
        return c->fail(FRAC_E_INVALID, "decode_frc1: scale must be in 1..16 and the scaled frame at most 65535 a side");
    if (!plane || plane_bytes < (uint64_t)scale * h.width * scale * h.height)
        return c->fail(FRAC_E_INVALID, "decode_frc1: the plane is smaller than the scaled frame");
    return decode_frc1_parsed(c, h, stream, scale, max_iter, rms_eps, host_plane(plane), iterations, rms);
}

// ---- FRQ1: the quadtree stream (fractencode_amd/codec.py documents the layout) -------------------

static uint32_t frq1_bitlen(uint64_t v)
{
    uint32_t b = 0;
    while (v) {
        ++b;
        v >>= 1;
    }
    return b;
}

// the level sides max, max / 2, …, min into n[]; 0 when the sizes are not the format's
static uint32_t frq1_levels(uint32_t max_size, uint32_t min_size, uint32_t n[4])
{
    auto ok = [](uint32_t s) { return s == 2 || s == 4 || s == 8 || s == 16; };
    if (!ok(max_size) || !ok(min_size) || min_size > max_size)
        return 0;
    uint32_t L = 0;
    for (uint32_t s = max_size; s >= min_size; s >>= 1)
        n[L++] = s;
    return L;
}

// The FRQ1 header "<4sHHIIBBBBB3xIIdddd" parsed, the bitmaps walked, everything checked against the stream
// length; on failure `msg` names the rule.
using Frq1Info = struct frac_frq1_info; // the plain name is the function's
static int frq1_parse(const uint8_t* s, size_t len, Frq1Info* o, std::string& msg)
{
    auto bad = [&](const char* why) {
        msg = std::string("FRQ1: ") + why;
        return FRAC_E_INVALID;
    };
    if (!s || !o)
        return bad("NULL argument");
    if (len < FRAC_FRQ1_HEADER_BYTES)
        return bad("truncated header");
    uint16_t version, flags;
    uint32_t wh[2], counts[2];
    double mm[4];
    std::memcpy(&version, s + 4, 2);
    std::memcpy(&flags, s + 6, 2);
    std::memcpy(wh, s + 8, sizeof(wh));
    std::memcpy(counts, s + 24, sizeof(counts));
    std::memcpy(mm, s + 32, sizeof(mm));
    if (std::memcmp(s, "FRQ1", 4) != 0 || version != 1)
        return bad("bad magic or version");
    *o = Frq1Info{};
    o->width = wh[0], o->height = wh[1], o->max_size = s[16], o->min_size = s[17];
    o->transforms = s[18], o->contrast_bits = s[19], o->brightness_bits = s[20], o->flags = flags;
    o->n_leaves = counts[0];
    o->contrast_min = mm[0], o->contrast_max = mm[1], o->brightness_min = mm[2], o->brightness_max = mm[3];
    if (o->width == 0 || o->height == 0 || o->width > 65535 || o->height > 65535)
        return bad("width and height must be in 1..65535");
    uint32_t side[4];
    o->levels = frq1_levels(o->max_size, o->min_size, side);
    if (!o->levels)
        return bad("sizes must be 2, 4, 8 or 16, min_size at most max_size");
    if (o->transforms < 1 || o->transforms > 8)
        return bad("transforms outside 1..8");
    if (o->contrast_bits < 2 || o->contrast_bits > 24 || o->brightness_bits < 2 || o->brightness_bits > 24)
        return bad("contrast / brightness bits outside [2, 24]");
    if (s[21] || s[22] || s[23] || counts[1])
        return bad("a reserved byte or word is not zero");
    const uint32_t t_bits = std::max(1u, frq1_bitlen(o->transforms - 1));
    for (uint32_t k = 0; k < o->levels; ++k) {
        o->n_domains[k] = (uint32_t)frac_uniform_grid(o->width, o->height, 2 * side[k], side[k], nullptr, 0);
        o->index_bits[k] = std::max(1u, frq1_bitlen(o->n_domains[k]));
        o->record_bits[k] = o->index_bits[k] + t_bits + o->contrast_bits + o->brightness_bits;
        if (o->record_bits[k] > 64)
            return bad("record wider than 64 bits");
    }
    uint64_t pos = FRAC_FRQ1_HEADER_BYTES, total = 0;
    uint64_t N = frac_uniform_grid(o->width, o->height, o->max_size, o->max_size, nullptr, 0);
    for (uint32_t k = 0; k < o->levels; ++k) {
        uint64_t S = 0;
        o->bitmap_offset[k] = pos;
        if (k + 1 < o->levels) {
            const uint64_t nw = (N + 31) / 32;
            if (len - pos < nw * 4)
                return bad("the stream ends inside a split bitmap");
            for (uint64_t j = 0; j < nw; ++j) {
                uint32_t w;
                std::memcpy(&w, s + pos + 4 * j, 4);
                if (j == nw - 1 && (N & 31u) && (w >> (N & 31u)))
                    return bad("a padding bit of a split bitmap is set");
                S += (uint32_t)__builtin_popcount(w);
            }
            pos += nw * 4;
        }
        const uint64_t M = N - S, nb = (M * o->record_bits[k] + 31) / 32 * 4;
        if (len - pos < nb)
            return bad("the stream ends inside a record section");
        o->nodes[k] = (uint32_t)N, o->leaves[k] = (uint32_t)M, o->record_offset[k] = pos;
        pos += nb;
        total += M;
        N = 4 * S;
    }
    o->body_bytes = pos - FRAC_FRQ1_HEADER_BYTES;
    if (total != o->n_leaves)
        return bad("n_leaves is not the levels' leaf count");
    for (double v : mm)
        if (!std::isfinite(v))
            return bad("non-finite quantizer bound");
    return FRAC_OK;
}

int frac_frq1_info(const uint8_t* stream, size_t len, struct frac_frq1_info* out)
{
    std::string msg;
    const int rc = frq1_parse(stream, len, out, msg);
    if (rc != FRAC_OK)
        g_last_error = msg;
    return rc;
}

// the 64 header bytes of a stream of nl leaves quantized between mm = {cmin, cmax, bmin, bmax}
static void frq1_header(uint8_t hdr[FRAC_FRQ1_HEADER_BYTES], uint32_t W, uint32_t H, uint32_t max_size,
                        uint32_t min_size, uint32_t T, uint32_t stream_flags, uint32_t cbits, uint32_t bbits,
                        uint32_t nl, const double mm[4])
{
    const uint16_t version = 1, flags = (uint16_t)stream_flags;
    const uint32_t wh[2] = {W, H};
    const uint8_t u8s[5] = {(uint8_t)max_size, (uint8_t)min_size, (uint8_t)T, (uint8_t)cbits, (uint8_t)bbits};
    std::memset(hdr, 0, FRAC_FRQ1_HEADER_BYTES);
    std::memcpy(hdr, "FRQ1", 4);
    std::memcpy(hdr + 4, &version, 2);
    std::memcpy(hdr + 6, &flags, 2);
    std::memcpy(hdr + 8, wh, 8);
    std::memcpy(hdr + 16, u8s, 5);
    std::memcpy(hdr + 24, &nl, 4);
    std::memcpy(hdr + 32, mm, 32);
}

int frac_pack_frq1(const frac_qt_leaf* leaves, size_t n, uint32_t W, uint32_t H, uint32_t max_size, uint32_t min_size,
                   uint32_t T, uint32_t stream_flags, uint32_t cbits, uint32_t bbits, uint8_t* out, size_t cap,
                   size_t* n_out)
{
    auto bad = [&](const std::string& why) {
        g_last_error = "pack_frq1: " + why;
        return FRAC_E_INVALID;
    };
    if (!n_out || (n && !leaves))
        return bad("NULL argument");
    if (cbits < 2 || cbits > 16 || bbits < 2 || bbits > 16)
        return bad("contrast/brightness bits must be in [2, 16]");
    if (W == 0 || H == 0 || W > 65535 || H > 65535)
        return bad("width and height must be in 1..65535");
    uint32_t side[4];
    const uint32_t L = frq1_levels(max_size, min_size, side);
    if (!L)
        return bad("sizes must be 2, 4, 8 or 16, min_size at most max_size");
    if (T < 1 || T > 8)
        return bad("transforms outside 1..8");
    // one quantizer pair over every leaf (codec._Field): min and max, the degenerate field coded as 0
    double cmin = 0.0, cmax = 0.0, bmin = 0.0, bmax = 0.0;
    for (size_t i = 0; i < n; ++i) {
        const double cv = leaves[i].contrast, bv = leaves[i].brightness;
        if (!std::isfinite(cv) || !std::isfinite(bv))
            return bad("leaf " + std::to_string(i) + ": non-finite contrast or brightness");
        cmin = i ? std::min(cmin, cv) : cv, cmax = i ? std::max(cmax, cv) : cv;
        bmin = i ? std::min(bmin, bv) : bv, bmax = i ? std::max(bmax, bv) : bv;
    }
    // Frac::Quantizer::quantized in FP64 (codec.Quantizer.quantized)
    auto quant = [](double v, double lo, double hi, uint32_t bits) -> uint64_t {
        if (!(hi > lo))
            return 0;
        const double step = std::fabs(hi - lo) / (double)(1u << bits);
        const double q = std::floor((v - lo) / step), qmax = (double)((1u << bits) - 1u);
        return (uint64_t)(q < qmax ? q : qmax);
    };
    const uint32_t tb = std::max(1u, frq1_bitlen(T - 1));
    std::vector<uint32_t> body, nodes, next;
    // level 0: createUniformGrid(max, max), row-major
    {
        const size_t cnt = frac_uniform_grid(W, H, max_size, max_size, nullptr, 0);
        const uint32_t cols = cnt ? (W - max_size) / max_size + 1 : 0;
        nodes.resize(cnt);
        for (size_t i = 0; i < cnt; ++i)
            nodes[i] = (uint32_t)(i % cols) * max_size | ((uint32_t)(i / cols) * max_size) << 16;
    }
    size_t p = 0; // the next leaf
    for (uint32_t k = 0; k < L; ++k) {
        const uint32_t sz = side[k], lg = frq1_bitlen(sz) - 1;
        const uint64_t nd = frac_uniform_grid(W, H, 2 * sz, sz, nullptr, 0);
        const uint32_t ib = std::max(1u, frq1_bitlen(nd)), width = ib + tb + cbits + bbits;
        if (width > 64)
            return bad("record wider than 64 bits");
        const bool last = k + 1 == L;
        const size_t bm = body.size();
        if (!last)
            body.resize(bm + (nodes.size() + 31) / 32, 0u);
        std::vector<uint32_t> recs; // the level's record section, filled bit by bit
        uint64_t bit = 0;
        next.clear();
        for (size_t i = 0; i < nodes.size(); ++i) {
            const uint32_t x = nodes[i] & 0xffffu, y = nodes[i] >> 16;
            const bool leaf = p < n && (leaves[p].code >> 28) == lg && leaves[p].x == x && leaves[p].y == y;
            if (!leaf) {
                if (last)
                    return bad("leaf " + std::to_string(p) + " is not the next leaf of the canonical order (the node at (" +
                               std::to_string(x) + ", " + std::to_string(y) + ") of the last level has none)");
                body[bm + (i >> 5)] |= 1u << (i & 31u);
                const uint32_t h = sz / 2;
                next.push_back(x | y << 16);
                next.push_back((x + h) | y << 16);
                next.push_back(x | (y + h) << 16);
                next.push_back((x + h) | (y + h) << 16);
                continue;
            }
            const frac_qt_leaf& e = leaves[p];
            const uint32_t d = e.code & FRAC_QT_NO_DOMAIN, t = (e.code >> 24) & 15u;
            if (d != FRAC_QT_NO_DOMAIN && d >= nd)
                return bad("leaf " + std::to_string(p) + ": domain index outside its level's grid");
            if (t >= T)
                return bad("leaf " + std::to_string(p) + ": transform outside the stream's");
            const uint64_t rec = (d == FRAC_QT_NO_DOMAIN ? nd : (uint64_t)d) | (uint64_t)t << ib |
                                 quant(e.contrast, cmin, cmax, cbits) << (ib + tb) |
                                 quant(e.brightness, bmin, bmax, bbits) << (ib + tb + cbits);
            recs.resize((size_t)((bit + width + 31) / 32), 0u);
            const uint32_t sh = (uint32_t)(bit & 31u);
            const size_t w = (size_t)(bit >> 5);
            recs[w] |= (uint32_t)(rec << sh);
            if (sh + width > 32)
                recs[w + 1] |= (uint32_t)(rec >> (32 - sh));
            if (sh + width > 64)
                recs[w + 2] |= (uint32_t)(rec >> (64 - sh));
            bit += width;
            ++p;
        }
        // a leaf of this level still next: it is no node of the level, or out of order, or there twice
        if (p < n && (leaves[p].code >> 28) >= lg)
            return bad("leaf " + std::to_string(p) + " is not the next leaf of the canonical order");
        body.insert(body.end(), recs.begin(), recs.end());
        nodes.swap(next);
    }
    if (p != n)
        return bad("leaf " + std::to_string(p) + " is not the next leaf of the canonical order");
    const size_t total = FRAC_FRQ1_HEADER_BYTES + body.size() * 4;
    *n_out = total;
    if (!out)
        return FRAC_OK;
    uint8_t hdr[FRAC_FRQ1_HEADER_BYTES];
    const double mm[4] = {cmin, cmax, bmin, bmax};
    frq1_header(hdr, W, H, max_size, min_size, T, stream_flags, cbits, bbits, (uint32_t)n, mm);
    std::memcpy(out, hdr, std::min<size_t>(cap, FRAC_FRQ1_HEADER_BYTES));
    if (cap > FRAC_FRQ1_HEADER_BYTES && !body.empty())
        std::memcpy(out + FRAC_FRQ1_HEADER_BYTES, body.data(), std::min(cap, total) - FRAC_FRQ1_HEADER_BYTES);
    return FRAC_OK;
}

// what frac_decode_frq1 refuses of a parsed stream beyond its parser
static int frq1_decodable(frac_ctx* c, const Frq1Info& h)
{
    for (uint32_t k = 0; k < h.levels; ++k)
        if (h.n_domains[k] >= (1u << 24))
            return c->fail(FRAC_E_INVALID, "decode_frq1: a level with 2^24 or more domains");
    return FRAC_OK;
}

// A parsed FRQ1 stream's leaves on the device, validated: what the iterative and the inter decoders share.
struct Frq1Device {
    Frq1Layout L{};
    uint32_t n = 0;     // leaves, in d_frq_leaves
    uint32_t mcols = 0; // the cell map's columns (d_frq_map, filled when the level-0 grid covers the frame)
    bool whole = false; // the leaves tile the frame and every leaf has a domain
    bool fast = false;  // the step kernels' geometry: whole, no stepwise flag
};

// The layout pass of the parsed stream `h` (body at stream + 64): the layout by value, the leaf entries in
// d_frq_leaves, the cell map and the indices checked.  Blocks for the status word; FRAC_E_INVALID for an index
// above its level's domain count, before anything else has been launched.
static int frq1_layout_device(frac_ctx* c, const Frq1Info& h, const uint8_t* stream, Frq1Device* d)
{
    const uint32_t n = h.n_leaves;
    Frq1Layout& L = d->L;
    L = Frq1Layout{};
    L.n_leaves = n;
    L.dc1 = L.dc2 = L.dc3 = L.dc4 = 1;
    for (uint32_t k = 0; k < h.levels; ++k) {
        const uint32_t sz = h.max_size >> k, nd = h.n_domains[k];
        const uint32_t dc = nd ? (h.width - 2 * sz) / sz + 1 : 1;
        (sz == 2 ? L.dc1 : sz == 4 ? L.dc2 : sz == 8 ? L.dc3 : L.dc4) = dc;
        (sz == 2 ? L.nd1 : sz == 4 ? L.nd2 : sz == 8 ? L.nd3 : L.nd4) = nd;
    }
    // Quantizer (encode/Quantizer.hpp:19-22): step = |max − min| / 2^bits; !(max > min): every code is min
    auto step = [](double lo, double hi, uint32_t bits) {
        return hi > lo ? std::fabs(hi - lo) / (double)(1u << bits) : 0.0;
    };
    L.c_step = step(h.contrast_min, h.contrast_max, h.contrast_bits);
    L.c_min = h.contrast_min;
    L.b_step = step(h.brightness_min, h.brightness_max, h.brightness_bits);
    L.b_min = h.brightness_min;

    FRAC_HIP(c, hipSetDevice(c->device));
    // the fast path's geometry: the level-0 grid covers the frame, so the leaves tile it
    const bool tiles = n && h.width % h.max_size == 0 && h.height % h.max_size == 0;
    const uint32_t mcols = h.width / h.min_size, mrows = h.height / h.min_size;
    // layout pass: reads only the stream buffer (the body and kFrc1PadWords zeroed dwords after it)
    uint32_t status[2] = {0, 0};
    if (n) {
        const size_t body_words = (size_t)(h.body_bytes / 4); // every section is whole dwords
        uint32_t max_nodes = 1, max_bm_words = 1;
        for (uint32_t k = 0; k < h.levels; ++k) {
            if (k)
                max_nodes = std::max(max_nodes, h.nodes[k]);
            if (k + 1 < h.levels)
                max_bm_words = std::max(max_bm_words, (h.nodes[k] + 31) / 32);
        }
        FRAC_HIP(c, c->d_frq_in.ensure(body_words + kFrc1PadWords));
        FRAC_HIP(c, c->d_frq_nodes[0].ensure(max_nodes));
        FRAC_HIP(c, c->d_frq_nodes[1].ensure(max_nodes));
        FRAC_HIP(c, c->d_frq_rank.ensure(max_bm_words));
        FRAC_HIP(c, c->d_frq_leaves.ensure(n));
        FRAC_HIP(c, c->d_frc_status.ensure(2));
        if (tiles)
            FRAC_HIP(c, c->d_frq_map.ensure((size_t)mcols * mrows));
        using PopcIter = hipcub::TransformInputIterator<uint32_t, Frq1Popc, const uint32_t*>;
        size_t need = 0;
        FRAC_HIP(c, hipcub::DeviceScan::ExclusiveSum(nullptr, need, PopcIter(c->d_frq_in.ptr, Frq1Popc()),
                                                     c->d_frq_rank.ptr, (int)max_bm_words, c->stream));
        if (need > c->qt_tmp_bytes) {
            FRAC_HIP(c, c->d_qt_tmp.ensure(need));
            c->qt_tmp_bytes = need;
        }
        FRAC_HIP(c, hipMemsetAsync(c->d_frq_in.ptr + body_words, 0, kFrc1PadWords * sizeof(uint32_t), c->stream));
        FRAC_HIP(c, hipMemsetAsync(c->d_frc_status.ptr, 0, sizeof(status), c->stream));
        FRAC_HIP(c, hipMemcpyAsync(c->d_frq_in.ptr, stream + FRAC_FRQ1_HEADER_BYTES, (size_t)h.body_bytes,
                                   hipMemcpyHostToDevice, c->stream));
        uint32_t leaf_base = 0;
        for (uint32_t k = 0; k < h.levels; ++k) {
            const uint32_t N = h.nodes[k];
            if (!N)
                break; // no node, none below
            Frq1Level lv{};
            lv.n_nodes = N;
            lv.lg = frq1_bitlen(h.max_size >> k) - 1;
            lv.cols0 = k ? 0 : h.width / h.max_size;
            lv.has_bitmap = k + 1 < h.levels;
            lv.bitmap_word = (uint32_t)((h.bitmap_offset[k] - FRAC_FRQ1_HEADER_BYTES) / 4);
            lv.rec_word = (uint32_t)((h.record_offset[k] - FRAC_FRQ1_HEADER_BYTES) / 4);
            lv.leaf_base = leaf_base;
            lv.n_domains = h.n_domains[k];
            lv.index_bits = h.index_bits[k];
            lv.c_bits = h.contrast_bits;
            lv.b_bits = h.brightness_bits;
            lv.t_bits = h.record_bits[k] - h.index_bits[k] - h.contrast_bits - h.brightness_bits;
            lv.record_bits = h.record_bits[k];
            lv.mcols = tiles ? mcols : 0;
            lv.cell_lg = frq1_bitlen(h.min_size) - 1;
            if (lv.has_bitmap) {
                size_t tb = c->qt_tmp_bytes;
                FRAC_HIP(c, hipcub::DeviceScan::ExclusiveSum(c->d_qt_tmp.ptr, tb,
                                                             PopcIter(c->d_frq_in.ptr + lv.bitmap_word, Frq1Popc()),
                                                             c->d_frq_rank.ptr, (int)((N + 31) / 32), c->stream));
            }
            frq1dec_level<<<(N + 255) / 256, 256, 0, c->stream>>>(c->d_frq_in.ptr, lv, c->d_frq_rank.ptr,
                                                                 c->d_frq_nodes[k & 1].ptr, c->d_frq_nodes[(k + 1) & 1].ptr,
                                                                 c->d_frq_leaves.ptr, c->d_frq_map.ptr,
                                                                 c->d_frc_status.ptr);
            leaf_base += h.leaves[k];
        }
        FRAC_HIP(c, hipGetLastError());
        FRAC_HIP(c, hipMemcpyAsync(status, c->d_frc_status.ptr, sizeof(status), hipMemcpyDeviceToHost, c->stream));
        FRAC_HIP(c, hipStreamSynchronize(c->stream));
        if (status[0])
            return c->fail(FRAC_E_INVALID, "FRQ1: domain index out of range");
    }
    d->n = n;
    d->mcols = mcols;
    d->whole = tiles && status[1] == 0; // every pixel written by a leaf with a domain
    d->fast = d->whole && !(c->p.flags & FRAC_FLAG_DECODE_STEPWISE);
    return FRAC_OK;
}

// the step kernels' arguments of a stream on their geometry at `scale`, but for the planes
static Frq1StepArgs frq1_step_args(frac_ctx* c, const Frq1Info& h, const Frq1Device& d, uint32_t scale)
{
    Frq1StepArgs a{};
    a.w = scale * h.width;
    a.h = scale * h.height;
    a.scale = scale;
    a.cell = h.min_size * scale;
    a.mcols = d.mcols;
    a.map = c->d_frq_map.ptr;
    a.leaves = c->d_frq_leaves.ptr;
    return a;
}

// frac_decode_frq1 past its argument checks: the parsed stream `h` (body at stream + 64) decoded at `scale`
// (checked by the caller) from and to `io`.
static int decode_frq1_parsed(frac_ctx* c, const Frq1Info& h, const uint8_t* stream, uint32_t scale, int max_iter,
                              double rms_eps, const PlaneIO& io, int* iterations, double* rms)
{
    const uint32_t W = scale * h.width, H = scale * h.height;
    Frq1Device d;
    FRAC_TRY(frq1_layout_device(c, h, stream, &d));
    const Frq1Layout& L = d.L;
    const uint32_t n = d.n;
    const bool whole = d.whole;
    if (d.fast) {
        Frq1StepArgs a = frq1_step_args(c, h, d, scale);
        const dim3 grid((W + kFrc1TileW - 1) / kFrc1TileW, (H + kFrc1TileH - 1) / kFrc1TileH);
        return decode_fused_loop(c, W, H, max_iter < 0 ? 300 : max_iter, rms_eps, io, iterations, rms,
                                 [&](const uint8_t* src, uint8_t* tgt, uint32_t stride) {
                                     a.src = src;
                                     a.tgt = tgt;
                                     a.stride = stride;
                                     frq1dec_step<<<grid, 256, 0, c->stream>>>(a, L, c->d_dec_state.ptr,
                                                                               c->d_dec_part.ptr);
                                 });
    }
    // every other stream: the leaves as scaled encode items, through the item decoder (fused when they
    // tile the plane and every leaf has a domain, as frac_decode decides)
    FRAC_HIP(c, c->d_dec_items.ensure(n));
    if (n) {
        frq1dec_expand<<<(n + 255) / 256, 256, 0, c->stream>>>(c->d_frq_leaves.ptr, L, scale, c->d_dec_items.ptr);
        FRAC_HIP(c, hipGetLastError());
    }
    return decode_impl(c, c->d_dec_items.ptr, n, W, H, max_iter, rms_eps, io, iterations, rms, whole);
}

int frac_decode_frq1(frac_ctx* c, const uint8_t* stream, size_t len, uint32_t scale, int max_iter, double rms_eps,
                     uint8_t* plane, size_t plane_bytes, int* iterations, double* rms)
{
    if (!c)
        return FRAC_E_INVALID;
    Frq1Info h;
    {
        std::string msg;
        if (frq1_parse(stream, len, &h, msg) != FRAC_OK)
            return c->fail(FRAC_E_INVALID, msg);
    }
    FRAC_TRY(check_ab_knobs(c));
    if (scale < 1 || scale > 16 || (uint64_t)scale * h.width > 65535 || (uint64_t)scale * h.height > 65535)
        return c->fail(FRAC_E_INVALID, "decode_frq1: scale must be in 1..16 and the scaled frame at most 65535 a side");
    if (!plane || plane_bytes < (uint64_t)scale * h.width * scale * h.height)
        return c->fail(FRAC_E_INVALID, "decode_frq1: the plane is smaller than the scaled frame");
    FRAC_TRY(frq1_decodable(c, h));
    return decode_frq1_parsed(c, h, stream, scale, max_iter, rms_eps, host_plane(plane), iterations, rms);
}

// ---- inter-coded frames: a stream applied once to a reference plane (fracenc_inter.hip) -----------

} // extern "C"

// An FRC1 or FRQ1 stream opened for an inter pass: told apart by its magic, parsed and checked as the iterative
// decoders check it; after inter_records also its records or leaves on the device.
struct InterStream {
    bool quad = false;
    Frc1Info h1{};
    Frq1Info hq{};
    Frc1Device d1;
    Frq1Device dq;
    uint32_t width() const { return quad ? hq.width : h1.width; }
    uint32_t height() const { return quad ? hq.height : h1.height; }
    uint32_t grid() const { return quad ? hq.max_size : h1.range_size; } // the covered rectangle's g
    uint32_t items() const { return quad ? dq.n : d1.n; }
    bool fast() const { return quad ? dq.fast : d1.fast; }
};

// everything an inter pass refuses by the stream and the scale, before any launch
static int inter_open(frac_ctx* c, const char* what, const uint8_t* stream, size_t len, uint32_t scale, InterStream* s)
{
    s->quad = stream && len >= 4 && std::memcmp(stream, "FRQ1", 4) == 0;
    {
        std::string msg;
        if (!s->quad && !(stream && len >= 4 && std::memcmp(stream, "FRC1", 4) == 0))
            return c->fail(FRAC_E_INVALID, std::string(what) + ": neither an FRC1 nor an FRQ1 stream");
        if ((s->quad ? frq1_parse(stream, len, &s->hq, msg) : frc1_parse(stream, len, &s->h1, msg)) != FRAC_OK)
            return c->fail(FRAC_E_INVALID, msg);
    }
    FRAC_TRY(check_ab_knobs(c));
    if (scale < 1 || scale > 16 || (uint64_t)scale * s->width() > 65535 || (uint64_t)scale * s->height() > 65535)
        return c->fail(FRAC_E_INVALID,
                       std::string(what) + ": scale must be in 1..16 and the scaled frame at most 65535 a side");
    if (s->quad)
        FRAC_TRY(frq1_decodable(c, s->hq));
    return FRAC_OK;
}

// the record or layout pass of an opened stream; blocks for its status word
static int inter_records(frac_ctx* c, const uint8_t* stream, InterStream* s)
{
    return s->quad ? frq1_layout_device(c, s->hq, stream, &s->dq) : frc1_records_device(c, s->h1, stream, &s->d1);
}

// a plane whose taps the fast kernels address modulo 2^32: its byte span must not exceed 2^32
static bool inter_span_ok(uint32_t pitch, uint32_t w, uint32_t h)
{
    return (uint64_t)pitch * (h - 1) + w <= (1ull << 32);
}

// The fast route of a stream for which s.fast() holds, enqueued on the context's stream: taps from `ref`
// (inter_span_ok), the result stored and / or compared as `io` says.
template <bool kWrite, bool kSse>
static int inter_launch_fast(frac_ctx* c, const InterStream& s, uint32_t scale, const uint8_t* ref, uint32_t rpitch,
                             const InterOut& io)
{
    const uint32_t W = scale * s.width(), H = scale * s.height();
    const dim3 grid((W + kFrc1TileW - 1) / kFrc1TileW, (H + kFrc1TileH - 1) / kFrc1TileH);
    if (s.quad) {
        Frq1StepArgs a = frq1_step_args(c, s.hq, s.dq, scale);
        a.src = ref;
        a.stride = rpitch;
        inter_frq1<kWrite, kSse><<<grid, 256, 0, c->stream>>>(a, s.dq.L, io);
    } else {
        Frc1StepArgs a = frc1_step_args(c, s.h1, scale);
        a.src = ref;
        a.stride = rpitch;
        inter_frc1<kWrite, kSse><<<grid, 256, 0, c->stream>>>(a, s.d1.L, io);
    }
    FRAC_HIP(c, hipGetLastError());
    return FRAC_OK;
}

// The general route, enqueued on the context's stream: `dst` filled from `ref` (row by row: the bytes between the
// destination's rows are not ours), the records or leaves expanded into scaled items, one inter_apply over them.
static int inter_launch_general(frac_ctx* c, const InterStream& s, uint32_t scale, const uint8_t* ref, uint32_t rpitch,
                                uint8_t* dst, uint32_t dpitch)
{
    const uint32_t W = scale * s.width(), H = scale * s.height(), n = s.items();
    if (rpitch == W && dpitch == W)
        FRAC_HIP(c, hipMemcpyAsync(dst, ref, (size_t)W * H, hipMemcpyDeviceToDevice, c->stream));
    else
        FRAC_HIP(c, hipMemcpy2DAsync(dst, dpitch, ref, rpitch, W, H, hipMemcpyDeviceToDevice, c->stream));
    if (!n)
        return FRAC_OK;
    FRAC_HIP(c, c->d_dec_items.ensure(n));
    if (s.quad)
        frq1dec_expand<<<(n + 255) / 256, 256, 0, c->stream>>>(c->d_frq_leaves.ptr, s.dq.L, scale, c->d_dec_items.ptr);
    else
        frc1dec_expand<<<(n + 255) / 256, 256, 0, c->stream>>>(c->d_frc_rec.ptr, s.d1.L, scale, c->d_dec_items.ptr);
    InterApplyArgs a;
    a.ref = ref;
    a.dst = dst;
    a.rpitch = rpitch;
    a.dpitch = dpitch;
    a.items = c->d_dec_items.ptr;
    a.n = n;
    inter_apply<<<(n + 3) / 4, 256, 0, c->stream>>>(a);
    FRAC_HIP(c, hipGetLastError());
    return FRAC_OK;
}

// Both entry points.  Host planes (h_ref, h_plane; tight rows) are staged in the decoder's buffers and the call
// returns synchronised; device planes are read and written in place on the context's stream.
static int decode_inter_impl(frac_ctx* c, const uint8_t* stream, size_t len, uint32_t scale, const uint8_t* h_ref,
                             uint8_t* h_plane, const void* d_ref, uint32_t ref_stride, void* d_plane,
                             uint32_t plane_stride, size_t plane_bytes)
{
    if (!c)
        return FRAC_E_INVALID;
    InterStream s;
    FRAC_TRY(inter_open(c, "decode_inter", stream, len, scale, &s));
    const uint32_t W = scale * s.width(), H = scale * s.height();
    const bool host = h_ref || h_plane;
    if (host ? (!h_ref || !h_plane) : (!d_ref || !d_plane))
        return c->fail(FRAC_E_INVALID, "decode_inter: ref or plane is NULL");
    if (host)
        ref_stride = plane_stride = W;
    if (ref_stride < W || plane_stride < W)
        return c->fail(FRAC_E_INVALID, "decode_inter: a stride below the scaled frame's width");
    const uint64_t rspan = (uint64_t)ref_stride * (H - 1) + W, pspan = (uint64_t)plane_stride * (H - 1) + W;
    if (plane_bytes < pspan)
        return c->fail(FRAC_E_INVALID, "decode_inter: plane_bytes is short of the scaled frame's last row");
    if (!host) {
        if (!inter_span_ok(ref_stride, W, H))
            return c->fail(FRAC_E_INVALID, "decode_inter: the reference plane spans more than 2^32 bytes");
        const uintptr_t r0 = reinterpret_cast<uintptr_t>(d_ref), p0 = reinterpret_cast<uintptr_t>(d_plane);
        if (r0 < p0 + pspan && p0 < r0 + rspan)
            return c->fail(FRAC_E_INVALID, "decode_inter: ref and plane overlap (an apply in place would read what it "
                                           "wrote)");
    }
    FRAC_TRY(inter_records(c, stream, &s)); // refuses a bad index before any byte of a plane is written
    const uint8_t* ref = static_cast<const uint8_t*>(d_ref);
    uint8_t* dst = static_cast<uint8_t*>(d_plane);
    if (host) {
        const uint32_t pitch = plane_pitch(W);
        const size_t bytes = (size_t)pitch * (H + 1);
        FRAC_HIP(c, c->d_dec_src.ensure(bytes));
        FRAC_HIP(c, c->d_dec_tgt.ensure(bytes));
        FRAC_HIP(c, hipMemcpy2DAsync(c->d_dec_src.ptr, pitch, h_ref, W, W, H, hipMemcpyHostToDevice, c->stream));
        ref = c->d_dec_src.ptr, dst = c->d_dec_tgt.ptr;
        ref_stride = plane_stride = pitch;
    }
    if (s.fast()) {
        InterOut io{};
        io.dst = dst;
        io.dpitch = plane_stride;
        io.dwords = (reinterpret_cast<uintptr_t>(dst) | plane_stride) % 4 == 0;
        FRAC_TRY((inter_launch_fast<true, false>(c, s, scale, ref, ref_stride, io)));
    } else {
        FRAC_TRY(inter_launch_general(c, s, scale, ref, ref_stride, dst, plane_stride));
    }
    if (host) {
        FRAC_HIP(c, hipMemcpy2DAsync(h_plane, W, dst, plane_stride, W, H, hipMemcpyDeviceToHost, c->stream));
        FRAC_HIP(c, hipStreamSynchronize(c->stream));
    }
    return FRAC_OK;
}

extern "C" {

int frac_decode_inter(frac_ctx* c, const uint8_t* stream, size_t len, uint32_t scale, const uint8_t* ref,
                      uint8_t* plane, size_t plane_bytes)
{
    if (c && (!ref || !plane))
        return c->fail(FRAC_E_INVALID, "decode_inter: ref or plane is NULL");
    return decode_inter_impl(c, stream, len, scale, ref, plane, nullptr, 0, nullptr, 0, plane_bytes);
}

int frac_decode_inter_device(frac_ctx* c, const uint8_t* stream, size_t len, uint32_t scale, const void* d_ref,
                             uint32_t ref_stride, void* d_plane, uint32_t plane_stride, size_t plane_bytes)
{
    return decode_inter_impl(c, stream, len, scale, nullptr, nullptr, d_ref, ref_stride, d_plane, plane_stride,
                             plane_bytes);
}

// ---- FRC3: the colour container (fractencode_amd/codec.py documents the layout) -------------------

using Frc3Info = struct frac_frc3_info; // the plain name is the function's
static size_t frc3_pad8(size_t n) { return (n + 7) & ~(size_t)7; }

// One plane stream of a container: told apart by its magic, parsed by its own parser, its frame compared with
// the plane's (the frame itself for Y, half of it either way for U and V).  kind: 1 = FRC1, 2 = FRQ1.
static int frc3_plane(const uint8_t* s, size_t len, uint32_t k, uint32_t width, uint32_t height, uint32_t* kind,
                      Frc1Info* h1, Frq1Info* hq, std::string& msg)
{
    static const char* const names[3] = {"Y", "U", "V"};
    auto bad = [&](const std::string& why) {
        msg = std::string("FRC3: the ") + names[k] + " stream: " + why;
        return FRAC_E_INVALID;
    };
    if (!s)
        return bad("NULL");
    uint32_t w = 0, h = 0;
    std::string inner;
    if (len >= 4 && std::memcmp(s, "FRC1", 4) == 0) {
        Frc1Info i;
        if (frc1_parse(s, len, &i, inner) != FRAC_OK)
            return bad(inner);
        *kind = 1, w = i.width, h = i.height;
        if (h1)
            *h1 = i;
    } else if (len >= 4 && std::memcmp(s, "FRQ1", 4) == 0) {
        Frq1Info i;
        if (frq1_parse(s, len, &i, inner) != FRAC_OK)
            return bad(inner);
        *kind = 2, w = i.width, h = i.height;
        if (hq)
            *hq = i;
    } else {
        return bad("neither an FRC1 nor an FRQ1 stream");
    }
    const uint32_t pw = k ? width / 2 : width, ph = k ? height / 2 : height;
    if (w != pw || h != ph)
        return bad("its frame is " + std::to_string(w) + "x" + std::to_string(h) + ", the plane's " +
                   std::to_string(pw) + "x" + std::to_string(ph));
    return FRAC_OK;
}

// The FRC3 header "<4sHHIIIIII" parsed, every section checked against the stream length and every plane
// stream by its own parser (h1 / hq, optional: the three planes' parsed headers, by kind).
static int frc3_parse(const uint8_t* s, size_t len, Frc3Info* o, Frc1Info* h1, Frq1Info* hq, std::string& msg)
{
    auto bad = [&](const char* why) {
        msg = std::string("FRC3: ") + why;
        return FRAC_E_INVALID;
    };
    if (!s || !o)
        return bad("NULL argument");
    if (len < FRAC_FRC3_HEADER_BYTES)
        return bad("truncated header");
    uint16_t version, flags;
    uint32_t u[6];
    std::memcpy(&version, s + 4, 2);
    std::memcpy(&flags, s + 6, 2);
    std::memcpy(u, s + 8, sizeof(u));
    if (std::memcmp(s, "FRC3", 4) != 0 || version != 1)
        return bad("bad magic or version");
    if (flags || u[5])
        return bad("the flags or the reserved word are not zero");
    *o = Frc3Info{};
    o->width = u[0], o->height = u[1], o->flags = flags;
    if (o->width < 2 || o->height < 2 || o->width > 65535 || o->height > 65535)
        return bad("width and height must be in 2..65535");
    uint64_t pos = FRAC_FRC3_HEADER_BYTES;
    for (uint32_t k = 0; k < 3; ++k) {
        const uint64_t n = u[2 + k], padded = (n + 7) & ~7ull;
        if (len - pos < padded)
            return bad("a plane section runs past the end of the stream");
        for (uint64_t i = n; i < padded; ++i)
            if (s[pos + i])
                return bad("a padding byte is not zero");
        o->offset[k] = pos, o->length[k] = n;
        pos += padded;
    }
    o->total_bytes = pos;
    for (uint32_t k = 0; k < 3; ++k)
        FRAC_TRY(frc3_plane(s + o->offset[k], (size_t)o->length[k], k, o->width, o->height, &o->kind[k],
                            h1 ? h1 + k : nullptr, hq ? hq + k : nullptr, msg));
    return FRAC_OK;
}

int frac_frc3_info(const uint8_t* stream, size_t len, struct frac_frc3_info* out)
{
    std::string msg;
    const int rc = frc3_parse(stream, len, out, nullptr, nullptr, msg);
    if (rc != FRAC_OK)
        g_last_error = msg;
    return rc;
}

int frac_pack_frc3(const uint8_t* const planes[3], const size_t lens[3], uint32_t width, uint32_t height, uint8_t* out,
                   size_t cap, size_t* n_out)
{
    auto bad = [&](const std::string& why) {
        g_last_error = why;
        return FRAC_E_INVALID;
    };
    if (!planes || !lens || !n_out)
        return bad("pack_frc3: NULL argument");
    if (width < 2 || height < 2 || width > 65535 || height > 65535)
        return bad("FRC3: width and height must be in 2..65535");
    size_t total = FRAC_FRC3_HEADER_BYTES;
    for (uint32_t k = 0; k < 3; ++k) {
        if (lens[k] > 0xffffffffull)
            return bad("pack_frc3: a plane stream of 4 GiB or more");
        uint32_t kind;
        std::string msg;
        if (frc3_plane(planes[k], lens[k], k, width, height, &kind, nullptr, nullptr, msg) != FRAC_OK)
            return bad(msg);
        total += frc3_pad8(lens[k]);
    }
    *n_out = total;
    if (!out)
        return FRAC_OK;
    std::vector<uint8_t> buf(total, 0);
    const uint16_t version = 1;
    const uint32_t u[6] = {width, height, (uint32_t)lens[0], (uint32_t)lens[1], (uint32_t)lens[2], 0u};
    std::memcpy(buf.data(), "FRC3", 4);
    std::memcpy(buf.data() + 4, &version, 2);
    std::memcpy(buf.data() + 8, u, sizeof(u));
    size_t pos = FRAC_FRC3_HEADER_BYTES;
    for (uint32_t k = 0; k < 3; ++k) {
        std::memcpy(buf.data() + pos, planes[k], lens[k]);
        pos += frc3_pad8(lens[k]);
    }
    std::memcpy(out, buf.data(), std::min(cap, total));
    return FRAC_OK;
}

// An FRC3 container opened for a decode at `scale`: the parsed headers and the geometry of the planes of d_frc3
// (Y at scale·W × scale·H, U and V at scale·(W/2) × scale·(H/2), each at plane_pitch of its width); after
// frc3_decode_planes also where they and the bytes asked for after them lie.
struct Frc3Decode {
    Frc3Info info;
    Frc1Info h1[3];
    Frq1Info hq[3];
    uint32_t W = 0, H = 0, cw = 0, ch = 0, ys = 0, cs = 0;
    size_t y_bytes = 0, c_bytes = 0;
    uint8_t* d_plane[3] = {nullptr, nullptr, nullptr};
    uint8_t* d_tail = nullptr;
};

// Everything a container's decode refuses by the container itself, before any launch.
static int frc3_open(frac_ctx* c, const uint8_t* stream, size_t len, uint32_t scale, Frc3Decode* p)
{
    {
        std::string msg;
        if (frc3_parse(stream, len, &p->info, p->h1, p->hq, msg) != FRAC_OK)
            return c->fail(FRAC_E_INVALID, msg);
    }
    const Frc3Info& info = p->info;
    FRAC_TRY(check_ab_knobs(c));
    if (scale < 1 || scale > 16 || (uint64_t)scale * info.width > 65535 || (uint64_t)scale * info.height > 65535)
        return c->fail(FRAC_E_INVALID, "decode_frc3: scale must be in 1..16 and the scaled frame at most 65535 a side");
    for (uint32_t k = 0; k < 3; ++k)
        if (info.kind[k] == 2)
            FRAC_TRY(frq1_decodable(c, p->hq[k]));
    p->W = scale * info.width, p->H = scale * info.height;
    p->cw = scale * (info.width / 2), p->ch = scale * (info.height / 2);
    p->ys = plane_pitch(p->W), p->cs = plane_pitch(p->cw);
    p->y_bytes = (size_t)p->ys * p->H, p->c_bytes = (size_t)p->cs * p->ch;
    return FRAC_OK;
}

// The three plane streams of an opened container decoded on the context's stream from zero planes into d_frc3,
// which also gets tail_bytes after the planes (d_tail).  Not synchronised.
static int frc3_decode_planes(frac_ctx* c, const uint8_t* stream, Frc3Decode* p, uint32_t scale, int max_iter,
                              double rms_eps, size_t tail_bytes, int* iterations, double* rms)
{
    FRAC_HIP(c, hipSetDevice(c->device));
    FRAC_HIP(c, c->d_frc3.ensure(p->y_bytes + 2 * p->c_bytes + tail_bytes));
    p->d_plane[0] = c->d_frc3.ptr;
    p->d_plane[1] = p->d_plane[0] + p->y_bytes;
    p->d_plane[2] = p->d_plane[1] + p->c_bytes;
    p->d_tail = p->d_plane[2] + p->c_bytes;
    for (uint32_t k = 0; k < 3; ++k) {
        PlaneIO io;
        io.d_out = p->d_plane[k];
        io.d_pitch = k ? p->cs : p->ys;
        const uint8_t* s = stream + p->info.offset[k];
        int it = 0;
        double r = 0.0;
        if (p->info.kind[k] == 1)
            FRAC_TRY(decode_frc1_parsed(c, p->h1[k], s, scale, max_iter, rms_eps, io, &it, &r));
        else
            FRAC_TRY(decode_frq1_parsed(c, p->hq[k], s, scale, max_iter, rms_eps, io, &it, &r));
        if (iterations)
            iterations[k] = it;
        if (rms)
            rms[k] = r;
    }
    return FRAC_OK;
}

// Both decode entry points: the planes of frc3_decode_planes converted into d_rgb, or (d_rgb NULL) into
// d_frc3's RGB section after them, which is copied to h_rgb.
static int decode_frc3_impl(frac_ctx* c, const uint8_t* stream, size_t len, uint32_t scale, int max_iter,
                            double rms_eps, void* d_rgb, uint8_t* h_rgb, uint32_t rgb_stride, size_t rgb_bytes,
                            int* iterations, double* rms)
{
    if (!c)
        return FRAC_E_INVALID;
    Frc3Decode p;
    FRAC_TRY(frc3_open(c, stream, len, scale, &p));
    const uint32_t W = p.W, H = p.H;
    if ((!d_rgb && !h_rgb) || rgb_stride < 3ull * W || rgb_bytes < (uint64_t)rgb_stride * (H - 1) + 3ull * W)
        return c->fail(FRAC_E_INVALID, "decode_frc3: rgb is NULL, its stride below 3·scale·W, or rgb_bytes short of "
                                       "the last row");
    const uint32_t rs = plane_pitch(3 * W);
    FRAC_TRY(frc3_decode_planes(c, stream, &p, scale, max_iter, rms_eps, d_rgb ? 0 : (size_t)rs * H, iterations, rms));
    if (d_rgb)
        return yuv_to_rgb_launch(c, p.d_plane[0], W, H, p.ys, p.d_plane[1], p.cs, p.d_plane[2], p.cs, p.cw, p.ch, d_rgb,
                                 rgb_stride);
    FRAC_TRY(yuv_to_rgb_launch(c, p.d_plane[0], W, H, p.ys, p.d_plane[1], p.cs, p.d_plane[2], p.cs, p.cw, p.ch,
                               p.d_tail, rs));
    FRAC_TRY(copy_plane(c, h_rgb, rgb_stride, p.d_tail, rs, 3 * W, H, hipMemcpyDeviceToHost, c->stream));
    FRAC_HIP(c, hipStreamSynchronize(c->stream));
    return FRAC_OK;
}

int frac_decode_frc3(frac_ctx* c, const uint8_t* stream, size_t len, uint32_t scale, int max_iter, double rms_eps,
                     uint8_t* rgb, uint32_t rgb_stride, size_t rgb_bytes, int iterations[3], double rms[3])
{
    return decode_frc3_impl(c, stream, len, scale, max_iter, rms_eps, nullptr, rgb, rgb_stride, rgb_bytes, iterations,
                            rms);
}

int frac_decode_frc3_device(frac_ctx* c, const uint8_t* stream, size_t len, uint32_t scale, int max_iter,
                            double rms_eps, void* d_rgb, uint32_t rgb_stride, size_t rgb_bytes, int iterations[3],
                            double rms[3])
{
    if (c && !d_rgb)
        return c->fail(FRAC_E_INVALID, "decode_frc3_device: d_rgb is NULL");
    return decode_frc3_impl(c, stream, len, scale, max_iter, rms_eps, d_rgb, nullptr, rgb_stride, rgb_bytes,
                            iterations, rms);
}

} // extern "C"
