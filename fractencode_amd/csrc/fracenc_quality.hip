// fracenc_quality.hip — the decoded error of a stream against the frame, on the device.
//
//   plane_sse_blocks  Σ(a − b)² of two pitched u8 planes over a covered rectangle of bw × bh blocks of g × g
//                     pixels from the origin: per block a u64 (optional) and the rectangle's u64 total.  Integers
//                     only, so no result depends on the order of the sums.  A block belongs to a group of
//                     `lanes` consecutive lanes of a wave (a power of two up to 64, the host's choice: the
//                     block's work units rounded up), so a wave takes 64 / lanes blocks at a time: a 16 × 16
//                     block of dwords fills a wave, a 4 × 4 one takes four lanes, and small blocks do not leave
//                     most of the wave idle.  A work unit is a dword of four pixels where g % 4 == 0 and both
//                     pitches and bases are dword-aligned (block origins are multiples of g), else a pixel.  A
//                     group's lanes stride over its block's units; the group's sum is a shuffle reduction over
//                     `lanes`, the total a per-lane u64 accumulator reduced over the wave, then over the
//                     workgroup's four waves in LDS: one atomic per workgroup.  Workgroups stride over the
//                     blocks.  Nothing outside the covered rectangle is read: a unit lies in a block, a block in
//                     the rectangle.
//   yuv_rgb_sse       Σ(R − R_ref)², Σ(G − G_ref)², Σ(B − B_ref)² of three pitched u8 planes Y (full size), U and V
//                     (half size) against a pitched packed-RGB reference over a rectangle rw × rh from the origin:
//                     each pixel converted by fracenc::yuv_pixel (the decoders' conversion, fracenc_color.hip) and
//                     compared in registers, so no RGB plane exists; nothing is written but the three u64 totals.
//                     Integers only after the conversion, so no result depends on the order of the sums.  Two
//                     paths, as the conversions have: <true> a lane takes 4 columns × 2 rows (one u16 of U and of
//                     V, two dwords of Y, 2 × 3 dwords of the reference; rw % 4 == 0, rh even, pitches and bases
//                     aligned: yuv_sse_fast_path), <false> a lane takes one 2 × 2 quad, with an odd trailing row or
//                     column.  The grid is sized to the rectangle: a lane makes one trip, nothing strides.  A
//                     lane's three sums (at most 8 · 255² each) are reduced as u32 over the wave by shuffles and
//                     over the workgroup's four waves in LDS (at most 2048 · 255² < 2^27), then added as u64: at
//                     most three atomics per workgroup, none for a zero sum.  The chroma cell of pixel (x, y) is
//                     (x / 2, y / 2), which lies inside the chroma planes for every pixel of the rectangle (the
//                     caller's rw <= 2 · chroma width, rh <= 2 · chroma height), so yuv2rgb_generic's clamp of the
//                     chroma index is never live here and is not carried.
// Included by fracenc_api.hip (after fracenc_codec.hip's decoders and fracenc_frq1pack.hip's packer, which the
// entry points chain):
//   frac_decode_error           parse as the decoders do, decode at scale 1 from a zero plane with a PlaneIO that
//                               delivers nothing and reports the final buffer, plane_sse_blocks against the plane
//                               the ranges lie on, on the context's stream (which waits for a pending frame
//                               upload: upload_planes); only the scalars and, when asked, the block sums come back
//   frac_quadtree_rate_errors   per split distance the packer's stream (through a pinned buffer of the context:
//                               the bytes frac_quadtree_rate_stream returns) into the same decode and comparison
//   frac_quadtree_rate_quality  the stated bisection over the rate state's candidates, one such probe each
//   frac_quadtree_rate_candidates  that list of candidates itself (rate_candidates_of, which the fit bisects)
//   frac_decode_error_frc3      the container opened and its planes decoded as frac_decode_frc3 does
//   (and _device)               (frc3_open, frc3_decode_planes), yuv_rgb_sse against the caller's RGB over the
//                               rectangle all three planes' grids cover; the host variant's RGB is uploaded behind
//                               the planes in d_frc3, rows as far apart as the caller's
//   frac_inter_error            the stream opened as frac_decode_inter opens it and applied once, at scale 1, to
//                               the plane the domains lie on: on the fast route inter_frc1 / inter_frq1 compare
//                               in registers with the plane the ranges lie on and write nothing; every other
//                               stream is applied into the decoder's target buffer and compared by plane_sse_blocks
// The decoded plane, the frame and the leaves never cross PCIe.

namespace {

struct PlaneSseArgs {
    const uint8_t* a; // the decoded plane
    const uint8_t* b; // the frame
    uint32_t pitch_a, pitch_b;
    uint32_t bw, bh, g;   // blocks across, down; the block side (1..65535)
    uint32_t lanes_lg;    // log2 of the lanes per block (0..6)
    uint32_t dwords;      // 1: a unit is four pixels of a row (g % 4 == 0, pitches and bases dword-aligned)
    unsigned long long* block_sse; // [min(bw·bh, block_cap)] row-major, or nullptr
    unsigned long long block_cap;
    unsigned long long* total;     // the rectangle's sum is added here
};

__global__ void __launch_bounds__(256) plane_sse_blocks(PlaneSseArgs s)
{
    __shared__ unsigned long long part[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t lanes = 1u << s.lanes_lg, per_wave = 64u >> s.lanes_lg;
    const uint32_t sub = lane >> s.lanes_lg, l = lane & (lanes - 1u);
    const unsigned long long nblocks = (unsigned long long)s.bw * s.bh;
    const uint32_t upr = s.dwords ? s.g >> 2 : s.g; // units per block row
    const uint32_t units = upr * s.g;               // at most 65535²
    const unsigned long long stride = (unsigned long long)gridDim.x * 4u * per_wave;
    unsigned long long sum = 0;
    // `first` is the wave's: every lane of a wave makes the same trips, so the shuffles below see all 64
    for (unsigned long long first = ((unsigned long long)blockIdx.x * 4u + wave) * per_wave; first < nblocks;
         first += stride) {
        const unsigned long long blk = first + sub;
        unsigned long long acc = 0;
        if (blk < nblocks) {
            const uint32_t bx = (uint32_t)(blk % s.bw), by = (uint32_t)(blk / s.bw);
            const uint8_t* pa = s.a + (size_t)by * s.g * s.pitch_a + (size_t)bx * s.g;
            const uint8_t* pb = s.b + (size_t)by * s.g * s.pitch_b + (size_t)bx * s.g;
            for (uint32_t u = l; u < units; u += lanes) {
                const uint32_t row = u / upr, col = u - row * upr;
                if (s.dwords) {
                    const uint32_t va = *reinterpret_cast<const uint32_t*>(pa + (size_t)row * s.pitch_a + 4u * col);
                    const uint32_t vb = *reinterpret_cast<const uint32_t*>(pb + (size_t)row * s.pitch_b + 4u * col);
                    uint32_t q = 0; // four squares of at most 255²
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) {
                        const int d = (int)((va >> (8 * j)) & 255u) - (int)((vb >> (8 * j)) & 255u);
                        q += (uint32_t)(d * d);
                    }
                    acc += q;
                } else {
                    const int d = (int)pa[(size_t)row * s.pitch_a + col] - (int)pb[(size_t)row * s.pitch_b + col];
                    acc += (uint32_t)(d * d);
                }
            }
        }
        sum += acc;
        if (s.block_sse) {
            for (uint32_t o = lanes >> 1; o > 0; o >>= 1)
                acc += __shfl_xor(acc, (int)o, 64);
            if (l == 0 && blk < nblocks && blk < s.block_cap)
                s.block_sse[blk] = acc;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        sum += __shfl_xor(sum, o, 64);
    if (lane == 0)
        part[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long t = part[0] + part[1] + part[2] + part[3];
        if (t)
            atomicAdd(s.total, t);
    }
}

struct YuvSseArgs {
    const uint8_t* y; // the decoded planes
    const uint8_t* u;
    const uint8_t* v;
    const uint8_t* rgb; // the reference, packed RGB
    uint32_t ys, us, vs, rs; // their pitches
    uint32_t rw, rh;         // the rectangle (both at least 1; rw <= 2 · chroma width, rh <= 2 · chroma height)
    unsigned long long* total; // [3] the R, G and B sums are added here
};

// one converted pixel (yuv_pixel's three bytes) against the reference's r, g, b
__device__ inline void rgb_sse_add(uint32_t px, uint32_t r, uint32_t g, uint32_t b, uint32_t acc[3])
{
    const int dr = (int)(px & 255u) - (int)r, dg = (int)((px >> 8) & 255u) - (int)g, db = (int)(px >> 16) - (int)b;
    acc[0] += (uint32_t)(dr * dr);
    acc[1] += (uint32_t)(dg * dg);
    acc[2] += (uint32_t)(db * db);
}

inline bool yuv_sse_fast_path(const YuvSseArgs& a)
{
    auto al = [](const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) % n) == 0; };
    return a.rw % 4 == 0 && a.rh % 2 == 0 && a.rs % 4 == 0 && a.ys % 4 == 0 && a.us % 2 == 0 && a.vs % 2 == 0 &&
           al(a.rgb, 4) && al(a.y, 4) && al(a.u, 2) && al(a.v, 2);
}

// the lanes of the rectangle on either path: its 4 × 2 blocks, or its 2 × 2 quads (a trailing row or column
// makes a quad of its own)
inline uint64_t yuv_sse_lanes(const YuvSseArgs& a, bool fast)
{
    return fast ? (uint64_t)(a.rw / 4) * (a.rh / 2) : (uint64_t)((a.rw + 1) / 2) * ((a.rh + 1) / 2);
}

template <bool kFast>
__global__ void __launch_bounds__(256) yuv_rgb_sse(YuvSseArgs s)
{
    __shared__ uint32_t part[4][3];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t acc[3] = {0, 0, 0};
    // no lane leaves before the shuffles: one past the rectangle keeps its zeros
    if (kFast) {
        const uint32_t bw = s.rw / 4, bh = s.rh / 2;
        if (t < (size_t)bw * bh) {
            const uint32_t bx = (uint32_t)(t % bw), by = (uint32_t)(t / bw);
            const uint32_t uu = *reinterpret_cast<const uint16_t*>(s.u + (size_t)by * s.us + 2 * (size_t)bx);
            const uint32_t vv = *reinterpret_cast<const uint16_t*>(s.v + (size_t)by * s.vs + 2 * (size_t)bx);
            const double up[2] = {(double)(uu & 255u) - 128.0, (double)(uu >> 8) - 128.0};
            const double vp[2] = {(double)(vv & 255u) - 128.0, (double)(vv >> 8) - 128.0};
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                const uint32_t y = 2 * by + dy;
                const uint32_t yw = *reinterpret_cast<const uint32_t*>(s.y + (size_t)y * s.ys + 4 * (size_t)bx);
                const uint32_t* ref = reinterpret_cast<const uint32_t*>(s.rgb + (size_t)y * s.rs + 12 * (size_t)bx);
                const uint32_t w0 = ref[0], w1 = ref[1], w2 = ref[2];
                // bytes: r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
                const uint32_t want[4][3] = {{w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u},
                                             {w0 >> 24, w1 & 255u, (w1 >> 8) & 255u},
                                             {(w1 >> 16) & 255u, w1 >> 24, w2 & 255u},
                                             {(w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24}};
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    rgb_sse_add(yuv_pixel((double)((yw >> (8 * k)) & 255u), up[k / 2], vp[k / 2]), want[k][0],
                                want[k][1], want[k][2], acc);
            }
        }
    } else {
        const uint32_t qw = (s.rw + 1) / 2, qh = (s.rh + 1) / 2;
        if (t < (size_t)qw * qh) {
            const uint32_t qx = (uint32_t)(t % qw), qy = (uint32_t)(t / qw);
            const double up = (double)s.u[(size_t)qy * s.us + qx] - 128.0, vp = (double)s.v[(size_t)qy * s.vs + qx] - 128.0;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                const uint32_t y = 2 * qy + dy;
                if (y >= s.rh)
                    break;
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const uint32_t x = 2 * qx + dx;
                    if (x >= s.rw)
                        break;
                    const uint8_t* p = s.rgb + (size_t)y * s.rs + 3 * (size_t)x;
                    rgb_sse_add(yuv_pixel((double)s.y[(size_t)y * s.ys + x], up, vp), p[0], p[1], p[2], acc);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            acc[k] += __shfl_xor(acc[k], o, 64);
        if (lane == 0)
            part[wave][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const uint32_t k = threadIdx.x;
        const uint32_t sum = part[0][k] + part[1][k] + part[2][k] + part[3][k];
        if (sum)
            atomicAdd(s.total + k, (unsigned long long)sum);
    }
}

// The comparison enqueued on the context's stream, on the path the arguments allow.
int yuv_rgb_sse_launch(frac_ctx* c, const YuvSseArgs& a)
{
    const bool fast = yuv_sse_fast_path(a);
    const unsigned wgs = (unsigned)((yuv_sse_lanes(a, fast) + 255) / 256); // at most 65535² / 4 / 256 < 2^23
    if (fast)
        yuv_rgb_sse<true><<<wgs, 256, 0, c->stream>>>(a);
    else
        yuv_rgb_sse<false><<<wgs, 256, 0, c->stream>>>(a);
    FRAC_HIP(c, hipGetLastError());
    return FRAC_OK;
}

// Σ(plane − frame)² over the bw × bh blocks (at least one) of g × g pixels from the origin, with the plane the
// ranges lie on as the frame; `plane` is device memory, read on the context's stream.  block_sse (host memory, or
// NULL) gets nb block sums.  Returns synchronised.
int frame_sse_of(frac_ctx* c, const uint8_t* plane, uint32_t pitch, uint32_t bw, uint32_t bh, uint32_t g,
                 uint64_t* block_sse, size_t nb, uint64_t* sse)
{
    auto& Q = c->quality;
    const uint64_t blocks = (uint64_t)bw * bh;
    FRAC_HIP(c, Q.d_total.ensure(1));
    FRAC_HIP(c, Q.h_total.ensure());
    if (nb)
        FRAC_HIP(c, Q.d_block.ensure(nb));
    FRAC_HIP(c, hipMemsetAsync(Q.d_total.ptr, 0, sizeof(unsigned long long), c->stream));
    const PlaneRef frame = target_plane(c);
    PlaneSseArgs a{};
    a.a = plane, a.pitch_a = pitch;
    a.b = frame.ptr, a.pitch_b = frame.stride;
    a.bw = bw, a.bh = bh, a.g = g;
    a.dwords = g % 4 == 0 && pitch % 4 == 0 && frame.stride % 4 == 0 &&
               (reinterpret_cast<uintptr_t>(plane) | reinterpret_cast<uintptr_t>(frame.ptr)) % 4 == 0;
    const uint64_t units = a.dwords ? (uint64_t)(g / 4) * g : (uint64_t)g * g;
    while (a.lanes_lg < 6 && (1ull << a.lanes_lg) < units)
        ++a.lanes_lg;
    a.block_sse = nb ? Q.d_block.ptr : nullptr;
    a.block_cap = nb;
    a.total = Q.d_total.ptr;
    const uint64_t per_wg = 4ull * (64u >> a.lanes_lg);
    const uint32_t wgs = (uint32_t)std::min<uint64_t>((blocks + per_wg - 1) / per_wg, 8192);
    plane_sse_blocks<<<wgs, 256, 0, c->stream>>>(a);
    FRAC_HIP(c, hipGetLastError());
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long));
    FRAC_HIP(c, hipMemcpyAsync(Q.h_total.ptr, Q.d_total.ptr, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                               c->stream));
    if (nb)
        FRAC_HIP(c, hipMemcpyAsync(block_sse, Q.d_block.ptr, nb * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    FRAC_HIP(c, hipStreamSynchronize(c->stream));
    *sse = *Q.h_total.ptr;
    return FRAC_OK;
}

// what one stream's decode and comparison give
struct StreamError {
    uint64_t sse = 0, pixels = 0, blocks = 0;
    uint32_t items = 0; // the stream's leaves or records
    int iterations = 0;
    double rms = 0.0;
};

// The stream decoded into the decoder's buffers and compared with the plane the ranges lie on; returns
// synchronised.  block_sse (host memory, or NULL) gets min(blocks, block_cap) block sums.
int decode_error_of(frac_ctx* c, const uint8_t* stream, size_t len, int max_iter, double eps, uint64_t* block_sse,
                    size_t block_cap, StreamError* r)
{
    *r = StreamError{};
    Frc1Info h1{};
    Frq1Info hq{};
    const bool quad = stream && len >= 4 && std::memcmp(stream, "FRQ1", 4) == 0;
    {
        std::string msg;
        if (!quad && !(stream && len >= 4 && std::memcmp(stream, "FRC1", 4) == 0))
            return c->fail(FRAC_E_INVALID, "decode_error: neither an FRC1 nor an FRQ1 stream");
        if ((quad ? frq1_parse(stream, len, &hq, msg) : frc1_parse(stream, len, &h1, msg)) != FRAC_OK)
            return c->fail(FRAC_E_INVALID, msg);
    }
    FRAC_TRY(check_ab_knobs(c));
    if (!c->planes_set)
        return c->fail(FRAC_E_STATE, "decode_error: no frame set");
    const uint32_t W = quad ? hq.width : h1.width, H = quad ? hq.height : h1.height;
    const uint32_t g = quad ? hq.max_size : h1.range_size;
    const frac_ctx::PlaneSize& fr = c->same_plane ? c->src : c->tgt;
    if (W != fr.w || H != fr.h)
        return c->fail(FRAC_E_INVALID, "decode_error: the stream's frame is " + std::to_string(W) + "x" +
                                           std::to_string(H) + ", the frame set is " + std::to_string(fr.w) + "x" +
                                           std::to_string(fr.h));
    if (g == 0)
        return c->fail(FRAC_E_INVALID, "decode_error: a range size of zero");
    PlaneIO::Final fin;
    PlaneIO io;
    io.final = &fin;
    if (quad) {
        FRAC_TRY(frq1_decodable(c, hq));
        FRAC_TRY(decode_frq1_parsed(c, hq, stream, 1, max_iter, eps, io, &r->iterations, &r->rms));
    } else {
        FRAC_TRY(decode_frc1_parsed(c, h1, stream, 1, max_iter, eps, io, &r->iterations, &r->rms));
    }
    r->items = quad ? hq.n_leaves : h1.n_ranges;
    const uint32_t bw = W / g, bh = H / g;
    r->blocks = (uint64_t)bw * bh;
    r->pixels = r->blocks * g * g;
    if (!r->blocks) {
        FRAC_HIP(c, hipStreamSynchronize(c->stream));
        return FRAC_OK;
    }
    const size_t nb = block_sse ? (size_t)std::min<uint64_t>(r->blocks, block_cap) : 0;
    return frame_sse_of(c, fin.ptr, fin.pitch, bw, bh, g, block_sse, nb, &r->sse);
}

// what an inter pass and its comparison give
struct InterError {
    uint64_t sse = 0, pixels = 0;
};

// The stream applied at scale 1 to the plane the domains lie on and compared with the plane the ranges lie on,
// over the covered rectangle; returns synchronised.  On the fast route the sums come from the kernel's registers
// and no plane is written; every other stream is applied into the decoder's target buffer and compared there.
int inter_error_of(frac_ctx* c, const uint8_t* stream, size_t len, InterError* r)
{
    *r = InterError{};
    InterStream s;
    FRAC_TRY(inter_open(c, "inter_error", stream, len, 1, &s));
    if (!c->planes_set)
        return c->fail(FRAC_E_STATE, "inter_error: no planes set");
    const uint32_t W = s.width(), H = s.height(), g = s.grid();
    const frac_ctx::PlaneSize& fr = c->same_plane ? c->src : c->tgt;
    if (W != c->src.w || H != c->src.h || W != fr.w || H != fr.h)
        return c->fail(FRAC_E_INVALID, "inter_error: the stream's frame is " + std::to_string(W) + "x" +
                                           std::to_string(H) + ", the planes set are " + std::to_string(c->src.w) +
                                           "x" + std::to_string(c->src.h) + " and " + std::to_string(fr.w) + "x" +
                                           std::to_string(fr.h));
    if (g == 0)
        return c->fail(FRAC_E_INVALID, "inter_error: a range size of zero");
    FRAC_TRY(inter_records(c, stream, &s));
    const uint32_t bw = W / g, bh = H / g;
    r->pixels = (uint64_t)bw * bh * g * g;
    if (!r->pixels) {
        FRAC_HIP(c, hipStreamSynchronize(c->stream));
        return FRAC_OK;
    }
    const PlaneRef frame = target_plane(c);
    auto& Q = c->quality;
    if (s.fast()) { // the ranges tile the frame: the covered rectangle is the frame
        FRAC_HIP(c, Q.d_total.ensure(1));
        FRAC_HIP(c, Q.h_total.ensure());
        FRAC_HIP(c, hipMemsetAsync(Q.d_total.ptr, 0, sizeof(unsigned long long), c->stream));
        InterOut io{};
        io.frame = frame.ptr;
        io.fpitch = frame.stride;
        io.total = Q.d_total.ptr;
        FRAC_TRY((inter_launch_fast<false, true>(c, s, 1, c->d_src.ptr, c->d_sstride, io)));
        FRAC_HIP(c, hipMemcpyAsync(Q.h_total.ptr, Q.d_total.ptr, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                   c->stream));
        FRAC_HIP(c, hipStreamSynchronize(c->stream));
        r->sse = *Q.h_total.ptr;
        return FRAC_OK;
    }
    const uint32_t pitch = plane_pitch(W);
    FRAC_HIP(c, c->d_dec_tgt.ensure((size_t)pitch * (H + 1)));
    FRAC_TRY(inter_launch_general(c, s, 1, c->d_src.ptr, c->d_sstride, c->d_dec_tgt.ptr, pitch));
    return frame_sse_of(c, c->d_dec_tgt.ptr, pitch, bw, bh, g, nullptr, 0, &r->sse);
}

// One probe of the rate readers: the rate state's stream at `split`, packed as frac_quadtree_rate_stream packs
// it into the context's pinned buffer, decoded and compared.  *len = the stream's bytes.  The caller has run
// qtr_reader_checks.
int rate_error_at(frac_ctx* c, uint32_t cbits, uint32_t bbits, double split, int max_iter, double eps, size_t* len,
                  StreamError* r)
{
    const auto& R = c->rate;
    const Frq1Geom g = frq1_geom(R.W, R.H, R.max_size, R.min_size, R.transforms, cbits, bbits);
    const uint64_t bound = frq1_body_bound(g);
    if (bound >= (1ull << 31))
        return c->fail(FRAC_E_INVALID, "FRQ1 pack: the stream could exceed 8 GiB");
    auto& Q = c->quality;
    FRAC_HIP(c, Q.stream.ensure(FRAC_FRQ1_HEADER_BYTES + (size_t)bound * 4));
    FRAC_TRY(frq1_pack_stream(c, g, R.W, R.H, R.max_size, R.min_size, R.transforms, R.classifier ? 1u : 0u, R.d_e.ptr,
                              split, R.d_nodes.ptr, 0, Q.stream.ptr, Q.stream.cap, len));
    if (*len > Q.stream.cap)
        return c->fail(FRAC_E_STATE, "FRQ1 pack: the stream exceeded its bound");
    return decode_error_of(c, Q.stream.ptr, *len, max_iter, eps, nullptr, 0, r);
}

// The rate state's candidates {0.0} ∪ {e(v)}, ascending and distinct, from its sorted keys: what the quality fit
// bisects and frac_quadtree_rate_candidates returns.  The caller has run qtr_reader_checks.
int rate_candidates_of(frac_ctx* c, std::vector<double>* cand)
{
    auto& R = c->rate;
    auto& Q = c->quality;
    Q.skey.resize(R.nkeys);
    if (R.nkeys) {
        FRAC_HIP(c, hipMemcpyAsync(Q.skey.data(), R.d_skey.ptr, (size_t)R.nkeys * sizeof(unsigned long long),
                                   hipMemcpyDeviceToHost, c->stream));
        FRAC_HIP(c, hipStreamSynchronize(c->stream));
    }
    cand->clear();
    cand->reserve((size_t)R.nkeys + 1);
    bool zero = false;
    auto push = [&](double v) {
        if (cand->empty() || cand->back() != v)
            cand->push_back(v);
    };
    for (unsigned long long k : Q.skey) {
        const double v = qtr_val(k);
        if (!zero && !(v < 0.0)) {
            push(0.0);
            zero = true;
        }
        push(v);
    }
    if (!zero)
        push(0.0);
    return FRAC_OK;
}

// what a container's decode and comparison give
struct ColorError {
    uint64_t sse[3] = {0, 0, 0}, pixels = 0;
    int iterations[3] = {0, 0, 0};
    double rms[3] = {0.0, 0.0, 0.0};
};

// what a g × g grid from the origin covers of w
inline uint32_t covered(uint32_t w, uint32_t g) { return w - w % g; }

// The container's planes decoded into d_frc3 and compared in RGB with the reference, which is d_rgb on the
// device or h_rgb on the host (uploaded behind the planes); returns synchronised.
int decode_error_frc3_of(frac_ctx* c, const uint8_t* stream, size_t len, const void* d_rgb, const uint8_t* h_rgb,
                         uint32_t rgb_stride, int max_iter, double eps, ColorError* r)
{
    *r = ColorError{};
    Frc3Decode p;
    FRAC_TRY(frc3_open(c, stream, len, 1, &p));
    if ((!d_rgb && !h_rgb) || rgb_stride < 3ull * p.W)
        return c->fail(FRAC_E_INVALID, "decode_error_frc3: rgb is NULL or its stride below 3·W");
    uint32_t rw = p.W, rh = p.H;
    for (uint32_t k = 0; k < 3; ++k) {
        const uint32_t g = p.info.kind[k] == 1 ? p.h1[k].range_size : p.hq[k].max_size;
        if (g == 0)
            return c->fail(FRAC_E_INVALID, "decode_error_frc3: a range size of zero");
        rw = std::min(rw, k ? 2 * covered(p.cw, g) : covered(p.W, g));
        rh = std::min(rh, k ? 2 * covered(p.ch, g) : covered(p.H, g));
    }
    r->pixels = (uint64_t)rw * rh;
    // the host's rows stay rgb_stride apart, so one copy carries them: up to the rectangle's last pixel
    const size_t ref_bytes = h_rgb && r->pixels ? (size_t)rgb_stride * (rh - 1) + 3 * (size_t)rw : 0;
    FRAC_TRY(frc3_decode_planes(c, stream, &p, 1, max_iter, eps, ref_bytes, r->iterations, r->rms));
    if (!r->pixels) {
        FRAC_HIP(c, hipStreamSynchronize(c->stream));
        return FRAC_OK;
    }
    auto& Q = c->quality;
    FRAC_HIP(c, Q.d_rgb_total.ensure(3));
    FRAC_HIP(c, Q.h_rgb_total.ensure());
    FRAC_HIP(c, hipMemsetAsync(Q.d_rgb_total.ptr, 0, 3 * sizeof(unsigned long long), c->stream));
    if (h_rgb)
        FRAC_HIP(c, hipMemcpyAsync(p.d_tail, h_rgb, ref_bytes, hipMemcpyHostToDevice, c->stream));
    YuvSseArgs a{};
    a.y = p.d_plane[0], a.u = p.d_plane[1], a.v = p.d_plane[2];
    a.ys = p.ys, a.us = a.vs = p.cs;
    a.rgb = h_rgb ? p.d_tail : static_cast<const uint8_t*>(d_rgb);
    a.rs = rgb_stride;
    a.rw = rw, a.rh = rh;
    a.total = Q.d_rgb_total.ptr;
    FRAC_TRY(yuv_rgb_sse_launch(c, a));
    FRAC_HIP(c, hipMemcpyAsync(Q.h_rgb_total.ptr, Q.d_rgb_total.ptr, 3 * sizeof(unsigned long long),
                               hipMemcpyDeviceToHost, c->stream));
    FRAC_HIP(c, hipStreamSynchronize(c->stream));
    for (uint32_t k = 0; k < 3; ++k)
        r->sse[k] = Q.h_rgb_total->sse[k];
    return FRAC_OK;
}

int decode_error_frc3_out(frac_ctx* c, const uint8_t* stream, size_t len, const void* d_rgb, const uint8_t* h_rgb,
                          uint32_t rgb_stride, int max_iter, double eps, uint64_t sse[3], uint64_t* pixels,
                          int iterations[3], double rms[3])
{
    if (!c)
        return FRAC_E_INVALID;
    ColorError r;
    FRAC_TRY(decode_error_frc3_of(c, stream, len, d_rgb, h_rgb, rgb_stride, max_iter, eps, &r));
    for (uint32_t k = 0; k < 3; ++k) {
        if (sse)
            sse[k] = r.sse[k];
        if (iterations)
            iterations[k] = r.iterations[k];
        if (rms)
            rms[k] = r.rms[k];
    }
    if (pixels)
        *pixels = r.pixels;
    return FRAC_OK;
}

} // namespace

extern "C" {

int frac_decode_error_frc3(frac_ctx* c, const uint8_t* stream, size_t len, const uint8_t* rgb, uint32_t rgb_stride,
                           int max_iter, double rms_eps, uint64_t sse[3], uint64_t* pixels, int iterations[3],
                           double rms[3])
{
    return decode_error_frc3_out(c, stream, len, nullptr, rgb, rgb_stride, max_iter, rms_eps, sse, pixels, iterations,
                                 rms);
}

int frac_decode_error_frc3_device(frac_ctx* c, const uint8_t* stream, size_t len, const void* d_rgb,
                                  uint32_t rgb_stride, int max_iter, double rms_eps, uint64_t sse[3], uint64_t* pixels,
                                  int iterations[3], double rms[3])
{
    return decode_error_frc3_out(c, stream, len, d_rgb, nullptr, rgb_stride, max_iter, rms_eps, sse, pixels,
                                 iterations, rms);
}

int frac_quadtree_rate_candidates(frac_ctx* c, double* out, size_t cap, size_t* n_out)
{
    if (!c)
        return FRAC_E_INVALID;
    FRAC_TRY(qtr_reader_checks(c, "quadtree rate candidates", 2, 2));
    std::vector<double> cand;
    FRAC_TRY(rate_candidates_of(c, &cand));
    if (n_out)
        *n_out = cand.size();
    if (out)
        std::memcpy(out, cand.data(), std::min(cand.size(), cap) * sizeof(double));
    return FRAC_OK;
}

int frac_decode_error(frac_ctx* c, const uint8_t* stream, size_t len, int max_iter, double rms_eps, uint64_t* sse,
                      uint64_t* pixels, uint64_t* block_sse, size_t block_cap, size_t* n_blocks, int* iterations,
                      double* rms)
{
    if (!c)
        return FRAC_E_INVALID;
    StreamError r;
    FRAC_TRY(decode_error_of(c, stream, len, max_iter, rms_eps, block_sse, block_cap, &r));
    if (sse)
        *sse = r.sse;
    if (pixels)
        *pixels = r.pixels;
    if (n_blocks)
        *n_blocks = (size_t)r.blocks;
    if (iterations)
        *iterations = r.iterations;
    if (rms)
        *rms = r.rms;
    return FRAC_OK;
}

int frac_inter_error(frac_ctx* c, const uint8_t* stream, size_t len, uint64_t* sse, uint64_t* pixels)
{
    if (!c)
        return FRAC_E_INVALID;
    InterError r;
    FRAC_TRY(inter_error_of(c, stream, len, &r));
    if (sse)
        *sse = r.sse;
    if (pixels)
        *pixels = r.pixels;
    return FRAC_OK;
}

int frac_quadtree_rate_errors(frac_ctx* c, uint32_t cbits, uint32_t bbits, const double* split, size_t n, int max_iter,
                              double rms_eps, uint64_t* sse, uint64_t* bytes, int* iterations)
{
    if (!c)
        return FRAC_E_INVALID;
    FRAC_TRY(qtr_reader_checks(c, "quadtree rate errors", cbits, bbits));
    if (n && !split)
        return c->fail(FRAC_E_INVALID, "quadtree rate errors: split is required");
    for (size_t i = 0; i < n; ++i) {
        StreamError r;
        size_t len = 0;
        FRAC_TRY(rate_error_at(c, cbits, bbits, split[i], max_iter, rms_eps, &len, &r));
        if (sse)
            sse[i] = r.sse;
        if (bytes)
            bytes[i] = len;
        if (iterations)
            iterations[i] = r.iterations;
    }
    return FRAC_OK;
}

int frac_quadtree_rate_quality(frac_ctx* c, uint32_t cbits, uint32_t bbits, uint64_t max_sse, int max_iter,
                               double rms_eps, double* split, uint64_t* bytes, uint32_t* leaves, uint64_t* sse,
                               uint32_t* probes)
{
    if (!c)
        return FRAC_E_INVALID;
    FRAC_TRY(qtr_reader_checks(c, "quadtree rate quality", cbits, bbits));
    std::vector<double> cand;
    FRAC_TRY(rate_candidates_of(c, &cand));
    const size_t m = cand.size();
    struct Probe {
        StreamError r;
        size_t len = 0;
    };
    uint32_t made = 0;
    auto probe = [&](size_t i, Probe* p) {
        ++made;
        return rate_error_at(c, cbits, bbits, cand[i], max_iter, rms_eps, &p->len, &p->r);
    };
    size_t answer = m - 1;
    Probe best;
    FRAC_TRY(probe(m - 1, &best));
    if (best.r.sse > max_sse) {
        Probe p0 = best;
        if (m > 1)
            FRAC_TRY(probe(0, &p0));
        if (p0.r.sse > max_sse)
            return c->fail(FRAC_E_INVALID, "quadtree rate quality: the decoded error at the smallest split distance, " +
                                               std::to_string(p0.r.sse) + ", exceeds " + std::to_string(max_sse));
        size_t lo = 0, hi = m - 1;
        best = p0;
        while (hi - lo > 1) {
            const size_t mid = lo + (hi - lo) / 2;
            Probe p;
            FRAC_TRY(probe(mid, &p));
            if (p.r.sse <= max_sse) {
                lo = mid;
                best = p;
            } else {
                hi = mid;
            }
        }
        answer = lo;
    }
    if (split)
        *split = cand[answer];
    if (bytes)
        *bytes = best.len;
    if (leaves)
        *leaves = best.r.items;
    if (sse)
        *sse = best.r.sse;
    if (probes)
        *probes = made;
    return FRAC_OK;
}

} // extern "C"
