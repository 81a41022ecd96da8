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
// Included by fracenc_api.hip (after fracenc_codec.hip's decoders and fracenc_frq1pack.hip's packer, which the
// entry points chain):
//   frac_decode_error           parse as the decoders do, decode at scale 1 from a zero plane with a PlaneIO that
//                               delivers nothing and reports the final buffer, plane_sse_blocks against the plane
//                               the ranges lie on, on the context's stream (which waits for a pending frame
//                               upload: upload_planes); only the scalars and, when asked, the block sums come back
//   frac_quadtree_rate_errors   per split distance the packer's stream (through a pinned buffer of the context:
//                               the bytes frac_quadtree_rate_stream returns) into the same decode and comparison
//   frac_quadtree_rate_quality  the stated bisection over the rate state's candidates, one such probe each
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
    auto& Q = c->quality;
    const size_t nb = block_sse ? (size_t)std::min<uint64_t>(r->blocks, block_cap) : 0;
    FRAC_HIP(c, Q.d_total.ensure(1));
    FRAC_HIP(c, Q.h_total.ensure());
    if (nb)
        FRAC_HIP(c, Q.d_block.ensure(nb));
    FRAC_HIP(c, hipMemsetAsync(Q.d_total.ptr, 0, sizeof(unsigned long long), c->stream));
    const PlaneRef frame = target_plane(c);
    PlaneSseArgs a{};
    a.a = fin.ptr, a.pitch_a = fin.pitch;
    a.b = frame.ptr, a.pitch_b = frame.stride;
    a.bw = bw, a.bh = bh, a.g = g;
    a.dwords = g % 4 == 0 && fin.pitch % 4 == 0 && frame.stride % 4 == 0 &&
               (reinterpret_cast<uintptr_t>(fin.ptr) | reinterpret_cast<uintptr_t>(frame.ptr)) % 4 == 0;
    const uint64_t units = a.dwords ? (uint64_t)(g / 4) * g : (uint64_t)g * g;
    while (a.lanes_lg < 6 && (1ull << a.lanes_lg) < units)
        ++a.lanes_lg;
    a.block_sse = nb ? Q.d_block.ptr : nullptr;
    a.block_cap = nb;
    a.total = Q.d_total.ptr;
    const uint64_t per_wg = 4ull * (64u >> a.lanes_lg);
    const uint32_t wgs = (uint32_t)std::min<uint64_t>((r->blocks + per_wg - 1) / per_wg, 8192);
    plane_sse_blocks<<<wgs, 256, 0, c->stream>>>(a);
    FRAC_HIP(c, hipGetLastError());
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long));
    FRAC_HIP(c, hipMemcpyAsync(Q.h_total.ptr, Q.d_total.ptr, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                               c->stream));
    if (nb)
        FRAC_HIP(c, hipMemcpyAsync(block_sse, Q.d_block.ptr, nb * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    FRAC_HIP(c, hipStreamSynchronize(c->stream));
    r->sse = *Q.h_total.ptr;
    return FRAC_OK;
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

} // namespace

extern "C" {

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
    auto& R = c->rate;
    auto& Q = c->quality;
    // the candidates {0.0} ∪ {e(v)}, ascending and distinct, from the state's sorted keys
    Q.skey.resize(R.nkeys);
    if (R.nkeys) {
        FRAC_HIP(c, hipMemcpyAsync(Q.skey.data(), R.d_skey.ptr, (size_t)R.nkeys * sizeof(unsigned long long),
                                   hipMemcpyDeviceToHost, c->stream));
        FRAC_HIP(c, hipStreamSynchronize(c->stream));
    }
    std::vector<double> cand;
    cand.reserve((size_t)R.nkeys + 1);
    bool zero = false;
    auto push = [&](double v) {
        if (cand.empty() || cand.back() != v)
            cand.push_back(v);
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
