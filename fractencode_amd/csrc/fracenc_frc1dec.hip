// fracenc_frc1dec.hip — FRC1 streams decoded on the device, at any integer scale.
//
//   frc1dec_records  once per call, one thread per record: the record's bit window out of the packed
//                    stream words (widths are not word-aligned: 20 bits at 64², 26 at 512², up to 64),
//                    the index check (index > n_domains fails the call; index == n_domains is a range
//                    without a domain), the raw record left as one u64 per range
//   frc1dec_step     one Decoder2 iteration for the geometry the packer writes (uniform range grid that
//                    tiles the frame, domain_size == 2·range_size, every range with a domain): threads
//                    mapped to output pixels, a lane produces 4 consecutive pixels of one row and stores
//                    them as one dword; the workgroup's records are staged once in LDS; the doubles are
//                    recomputed from the codes per use (Quantizer::value, two FP64 operations); the
//                    (source − new)² partial sums, decode_check and DecodeState are the fused decoder's
//                    (fracenc_decode.hip)
//   frc1dec_expand   every other stream (another size ratio, margins, domain-less records): the records
//                    as scaled frac_encode_items for decode_apply / decode_fused
// Every coordinate and size is multiplied by `scale`; transform, contrast and brightness are not
// (fractal records are resolution-independent).  fractencode_amd/codec.py unpack_stream is the host
// restatement the tests compare against.
#include "fracenc_common.h"

namespace fracenc {

constexpr uint32_t kFrc1PadWords = 3;  // zeroed dwords after the body: a record's window is 3 dwords
constexpr uint32_t kFrc1TileW = 64, kFrc1TileH = 16; // output pixels per workgroup of frc1dec_step
constexpr uint32_t kFrc1TileRecs = kFrc1TileW * kFrc1TileH; // records a tile can touch (1×1 ranges)

// What the header fixes, by value to every kernel.
struct Frc1Layout {
    uint32_t n_ranges, n_domains;
    uint32_t rcols, dcols; // range / domain grid columns (createUniformGrid)
    uint32_t range_size, domain_size, domain_stride;
    uint32_t index_bits, t_bits, c_bits, b_bits, record_bits;
    // Quantizer::value(q) = fl(fma(q, step, min)) + step/2; step == 0: the degenerate field, always min
    double c_step, c_min, b_step, b_min;
};

struct Frc1Fields {
    uint32_t idx, t, qc, qb;
};

__device__ inline uint32_t frc1_take(unsigned long long& r, uint32_t bits)
{
    const uint32_t v = (uint32_t)(r & ((1ull << bits) - 1ull)); // bits <= 32
    r >>= bits;
    return v;
}

__device__ inline Frc1Fields frc1_fields(unsigned long long r, const Frc1Layout& L)
{
    Frc1Fields f;
    f.idx = frc1_take(r, L.index_bits);
    f.t = frc1_take(r, L.t_bits);
    f.qc = frc1_take(r, L.c_bits);
    f.qb = frc1_take(r, L.b_bits);
    return f;
}

// codec.Quantizer.value: the first rounding fused as the built reference contracts it
__device__ inline double frc1_value(uint32_t q, double step, double mn)
{
    return step > 0.0 ? __fma_rn((double)q, step, mn) + step * 0.5 : mn;
}

// status[0]: records whose index exceeds n_domains; status[1]: records without a domain
__global__ void __launch_bounds__(256) frc1dec_records(const uint32_t* __restrict__ words, Frc1Layout L,
                                                       unsigned long long* __restrict__ rec,
                                                       uint32_t* __restrict__ status)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.n_ranges)
        return;
    const uint64_t bit = i * L.record_bits, w = bit >> 5;
    const uint32_t sh = (uint32_t)(bit & 31u);
    // stream bits [bit, bit + 64) lie in dwords w .. w + 2 (the buffer is padded by kFrc1PadWords)
    const unsigned long long lo = (unsigned long long)words[w] | ((unsigned long long)words[w + 1] << 32);
    unsigned long long r = lo >> sh;
    if (sh)
        r |= (unsigned long long)words[w + 2] << (64u - sh);
    if (L.record_bits < 64)
        r &= (1ull << L.record_bits) - 1ull;
    const uint32_t idx = (uint32_t)(r & ((1ull << L.index_bits) - 1ull));
    if (idx > L.n_domains)
        atomicAdd(&status[0], 1u);
    else if (idx == L.n_domains)
        atomicAdd(&status[1], 1u);
    rec[i] = r;
}

__global__ void __launch_bounds__(256) frc1dec_expand(const unsigned long long* __restrict__ rec, Frc1Layout L,
                                                      uint32_t scale, frac_encode_item* __restrict__ items)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.n_ranges)
        return;
    const Frc1Fields f = frc1_fields(rec[i], L);
    const bool has = f.idx < L.n_domains;
    const uint32_t dcols = L.dcols ? L.dcols : 1u;
    frac_encode_item e;
    e.x = (uint32_t)(i % L.rcols) * L.range_size * scale;
    e.y = (uint32_t)(i / L.rcols) * L.range_size * scale;
    e.w = e.h = L.range_size * scale;
    e.match.score.distance = 0.0;
    e.match.score.contrast = has ? frc1_value(f.qc, L.c_step, L.c_min) : 0.0;
    e.match.score.brightness = has ? frc1_value(f.qb, L.b_step, L.b_min) : 0.0;
    e.match.score.transform = has ? (int32_t)f.t : 0;
    e.match.score._pad = 0;
    e.match.x = has ? (f.idx % dcols) * L.domain_stride * scale : 0u;
    e.match.y = has ? (f.idx / dcols) * L.domain_stride * scale : 0u;
    e.match.sw = e.match.sh = has ? L.domain_size * scale : 0u;
    items[i] = e;
}

// The linear part of the transform LUT (fracenc_common.h lut) as plane-offset steps, modulo 2^32: one step
// of the local x is a4·stride + a0, one of the local y a5·stride + a1.  kFrc1Lin holds a0, a1, a4, a5 (+1,
// two bits each) of transform t in byte t.
constexpr unsigned long long frc1_lin_codes()
{
    unsigned long long k = 0;
    for (int t = 0; t < 8; ++t) {
        const Aff a = lut(t);
        k |= (unsigned long long)((a.a0 + 1) | ((a.a1 + 1) << 2) | ((a.a4 + 1) << 4) | ((a.a5 + 1) << 6)) << (8 * t);
    }
    return k;
}
constexpr unsigned long long kFrc1Lin = frc1_lin_codes();
__device__ inline uint32_t frc1_step_x(uint32_t t, uint32_t stride)
{
    const uint32_t c = (uint32_t)(kFrc1Lin >> (8 * t));
    return (((c >> 4) & 3u) - 1u) * stride + ((c & 3u) - 1u);
}
__device__ inline uint32_t frc1_step_y(uint32_t t, uint32_t stride)
{
    const uint32_t c = (uint32_t)(kFrc1Lin >> (8 * t));
    return (((c >> 6) & 3u) - 1u) * stride + (((c >> 2) & 3u) - 1u);
}

struct Frc1StepArgs {
    const uint8_t* src;
    uint8_t* tgt;
    uint32_t stride;            // plane row stride, a multiple of 64 (inter_frc1: the reference's pitch, any value)
    uint32_t w, h;              // scaled plane: rcols·R × rrows·R
    uint32_t R;                 // scaled range side; the domain patch is 2R square
    uint32_t rrows;             // range grid rows
    uint32_t scale;
    const unsigned long long* rec; // [n_ranges] validated records, each with a domain
};

// grid: (⌈w / 64⌉, ⌈h / 16⌉); thread t: row t / 16 of the tile, pixels 4·(t % 16) .. + 3
__global__ void __launch_bounds__(256) frc1dec_step(Frc1StepArgs a, Frc1Layout L, const DecodeState* __restrict__ st,
                                                    unsigned long long* __restrict__ partial)
{
    if (st->done)
        return;
    __shared__ uint4 srec[kFrc1TileRecs]; // {plane offset of the domain's tap of local (0, 0), transform, q_contrast, q_brightness}
    __shared__ unsigned long long part[4];
    const uint32_t R = a.R, tx0 = blockIdx.x * kFrc1TileW, ty0 = blockIdx.y * kFrc1TileH;
    // the tile's ranges: columns rx0..rx1, rows ry0..ry1 of the range grid (tx0 < w and ty0 < h by the grid)
    const uint32_t rx0 = tx0 / R, ry0 = ty0 / R;
    const uint32_t rx1 = min((tx0 + kFrc1TileW - 1) / R, L.rcols - 1), ry1 = min((ty0 + kFrc1TileH - 1) / R, a.rrows - 1);
    const uint32_t nc = rx1 - rx0 + 1, nrec = nc * (ry1 - ry0 + 1); // <= kFrc1TileRecs
    for (uint32_t k = threadIdx.x; k < nrec; k += 256) {
        const uint32_t ry = ry0 + k / nc, rx = rx0 + k % nc;
        const Frc1Fields f = frc1_fields(a.rec[(size_t)ry * L.rcols + rx], L);
        const uint32_t ox = (f.idx % L.dcols) * L.domain_stride * a.scale;
        const uint32_t oy = (f.idx / L.dcols) * L.domain_stride * a.scale; // both <= 65535
        // sample_sum_dev's first tap of local (sx, sy) is plane offset row·stride + px with
        //   px = ox + a0·sx + a1·sy + (a2 + a3)(S − 1),  row = oy + a4·sx + a5·sy + (a6 + a7)(S − 1)
        // = base + sx·(a4·stride + a0) + sy·(a5·stride + a1); every plane offset is below 2^32 (65535 rows
        // of at most 65536 bytes), so base and the steps are kept modulo 2^32
        const Aff t = lut((int)f.t);
        const uint32_t S1 = 2 * R - 1;
        const uint32_t base = (oy + (uint32_t)(t.a6 + t.a7) * S1) * a.stride + ox + (uint32_t)(t.a2 + t.a3) * S1;
        srec[k] = make_uint4(base, f.t, f.qc, f.qb);
    }
    __syncthreads();
    const uint32_t y = ty0 + (threadIdx.x >> 4), x0 = tx0 + (threadIdx.x & 15u) * 4u;
    uint32_t acc = 0;
    if (y < a.h && x0 < a.w) {
        const uint32_t ry = y / R, ly = y - ry * R;
        uint32_t rx = x0 / R, lx = x0 - rx * R;
        const uint4* row = srec + (ry - ry0) * nc;
        uint4 q = row[rx - rx0];
        double s = frc1_value(q.z, L.c_step, L.c_min), o = frc1_value(q.w, L.b_step, L.b_min);
        // the taps of local (sx, sy) = (2·lx, 2·ly): p, p + d1, p + d2, p + d1 + d2 with p = base + sx·d1 + sy·d2.
        // sx and sy are even and at most S − 2, so sample_sum_dev's edge clamp (at S − 1) never applies.
        uint32_t d1 = frc1_step_x(q.y, a.stride), d2 = frc1_step_y(q.y, a.stride);
        uint32_t p = q.x + 2 * lx * d1 + 2 * ly * d2;
        const size_t off = (size_t)y * a.stride + x0; // dword-aligned: stride % 64 == 0, x0 % 4 == 0
        const uint32_t old = *reinterpret_cast<const uint32_t*>(a.src + off);
        uint32_t out = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            if (x0 + j < a.w) {
                const int sum = (int)a.src[p] + (int)a.src[p + d1] + (int)a.src[p + d2] + (int)a.src[p + d1 + d2];
                const double v = __fma_rn(s, (double)sum / 4.0, o);
                const uint32_t nv = v < 0.0 ? 0u : v > 255 ? 255u : (uint32_t)(uint8_t)v;
                const int d = (int)((old >> (8 * j)) & 255u) - (int)nv;
                acc += (uint32_t)(d * d);
                out |= nv << (8 * j);
                p += 2 * d1;
                if (++lx == R && j < 3 && x0 + j + 1 < a.w) { // the next pixel starts the next range
                    lx = 0;
                    q = row[++rx - rx0];
                    s = frc1_value(q.z, L.c_step, L.c_min);
                    o = frc1_value(q.w, L.b_step, L.b_min);
                    d1 = frc1_step_x(q.y, a.stride);
                    d2 = frc1_step_y(q.y, a.stride);
                    p = q.x + 2 * ly * d2;
                }
            }
        }
        *reinterpret_cast<uint32_t*>(a.tgt + off) = out; // bytes past w lie in the row padding
    }
    unsigned long long sum = acc;
#pragma unroll
    for (int k = 32; k > 0; k >>= 1)
        sum += __shfl_xor(sum, k, 64);
    if ((threadIdx.x & 63u) == 0)
        part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0)
        atomicAdd(&partial[(blockIdx.y * gridDim.x + blockIdx.x) & (kDecodeSlots - 1)],
                  part[0] + part[1] + part[2] + part[3]);
}

} // namespace fracenc
