// fracenc_inter.hip — inter-coded frames: an FRC1 / FRQ1 stream applied once to a reference plane.
//
// A record means "range = s·(domain of the reference) + o": one Frac::copy per record that has a domain, read from
// the reference and written to another plane.  There is no iteration, so no DecodeState, no partial slots and no
// read of the old target; the two planes are the caller's memory, each with a pitch of its own.
//
//   inter_frc1<kWrite, kSse>  frc1dec_step's pixel mapping (a workgroup owns 64×16 output pixels, a lane four
//   inter_frq1<kWrite, kSse>  consecutive pixels of a row) for the streams of those kernels' fast geometry: ranges
//                     or leaves tile the frame, the domain side is twice the range side, every range has a domain.
//                     FRC1 stages the workgroup's records in LDS, FRQ1 finds its leaf through the cell map
//                     (frq1_place).  The taps' plane offsets are built with the reference's pitch, modulo 2^32 as
//                     in the step kernels: that holds because the host refuses a plane whose byte span
//                     (rows − 1)·pitch + width exceeds 2^32, so every offset inside a plane is below 2^32 whatever
//                     the pitch.  The store's offset is 64-bit.
//                     kWrite: the four pixels go to the destination, as one dword where the destination's base
//                     and pitch are 4-aligned (InterOut::dwords, the host's choice for the whole launch) and the
//                     dword ends inside the row; as bytes otherwise.  Nothing past column w − 1 is written: the
//                     destination's rows have no padding of ours.
//                     kSse: (new − frame)² of the lane's pixels in u32 (at most 4·255²), reduced as
//                     yuv_rgb_sse reduces (shuffles over the wave, four waves through LDS: at most 1024·255² <
//                     2^27), then at most one u64 atomic per workgroup and none for a zero sum.  The frame is a
//                     plane of the context (pitch a multiple of 64, so the lane's dword lies inside the row's
//                     allocation).  With kWrite false nothing is stored.
//   inter_apply       every other stream (another size ratio, margins, domain-less records, the stepwise flag):
//                     decode_apply with a pitch per plane, over frc1dec_expand's / frq1dec_expand's scaled items.
//                     The host fills the destination from the reference first; an item without a domain returns.
#include "fracenc_common.h"

namespace fracenc {

// where an inter pass writes and what it compares with
struct InterOut {
    uint8_t* dst;              // kWrite: the destination plane
    uint32_t dpitch;
    uint32_t dwords;           // 1: dst and dpitch are 4-aligned, whole dwords are stored as one
    const uint8_t* frame;      // kSse: the frame, a plane of the context
    uint32_t fpitch;
    unsigned long long* total; // kSse: the sum is added here
};

// Frac::copy's value of one pixel: the four taps at p, p + d1, p + d2, p + d1 + d2 of the reference
__device__ inline uint32_t inter_pixel(const uint8_t* __restrict__ ref, uint32_t p, uint32_t d1, uint32_t d2, double s,
                                       double o)
{
    const int sum = (int)ref[p] + (int)ref[p + d1] + (int)ref[p + d2] + (int)ref[p + d1 + d2];
    const double v = __fma_rn(s, (double)sum / 4.0, o);
    return v < 0.0 ? 0u : v > 255 ? 255u : (uint32_t)(uint8_t)v;
}

// the lane's pixels x0 .. x0 + 3 of row y (those below w), packed in `out`: stored and / or compared
template <bool kWrite, bool kSse>
__device__ inline uint32_t inter_finish(const InterOut& io, uint32_t x0, uint32_t y, uint32_t w, uint32_t out)
{
    if (kWrite) {
        uint8_t* row = io.dst + (size_t)y * io.dpitch + x0;
        if (io.dwords && x0 + 4u <= w) {
            *reinterpret_cast<uint32_t*>(row) = out;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (x0 + j < w)
                    row[j] = (uint8_t)(out >> (8 * j));
        }
    }
    uint32_t acc = 0;
    if (kSse) {
        const uint32_t want = *reinterpret_cast<const uint32_t*>(io.frame + (size_t)y * io.fpitch + x0);
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if (x0 + j < w) {
                const int d = (int)((out >> (8 * j)) & 255u) - (int)((want >> (8 * j)) & 255u);
                acc += (uint32_t)(d * d);
            }
    }
    return acc;
}

// the workgroup's sum of the lanes' acc into io.total; every lane of the workgroup arrives
__device__ inline void inter_reduce(const InterOut& io, uint32_t acc)
{
    __shared__ uint32_t part[4];
#pragma unroll
    for (int k = 32; k > 0; k >>= 1)
        acc += __shfl_xor(acc, k, 64);
    if ((threadIdx.x & 63u) == 0)
        part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t sum = part[0] + part[1] + part[2] + part[3];
        if (sum)
            atomicAdd(io.total, (unsigned long long)sum);
    }
}

// grid: (⌈w / 64⌉, ⌈h / 16⌉); thread t: row t / 16 of the tile, pixels 4·(t % 16) .. + 3.
// a: frc1dec_step's arguments with src = the reference, stride = its pitch; a.tgt is not used.
template <bool kWrite, bool kSse>
__global__ void __launch_bounds__(256) inter_frc1(Frc1StepArgs a, Frc1Layout L, InterOut io)
{
    __shared__ uint4 srec[kFrc1TileRecs]; // as frc1dec_step's: {offset of the tap of local (0, 0), transform, codes}
    const uint32_t R = a.R, tx0 = blockIdx.x * kFrc1TileW, ty0 = blockIdx.y * kFrc1TileH;
    const uint32_t rx0 = tx0 / R, ry0 = ty0 / R;
    const uint32_t rx1 = min((tx0 + kFrc1TileW - 1) / R, L.rcols - 1), ry1 = min((ty0 + kFrc1TileH - 1) / R, a.rrows - 1);
    const uint32_t nc = rx1 - rx0 + 1, nrec = nc * (ry1 - ry0 + 1); // <= kFrc1TileRecs
    for (uint32_t k = threadIdx.x; k < nrec; k += 256) {
        const uint32_t ry = ry0 + k / nc, rx = rx0 + k % nc;
        const Frc1Fields f = frc1_fields(a.rec[(size_t)ry * L.rcols + rx], L);
        const uint32_t ox = (f.idx % L.dcols) * L.domain_stride * a.scale;
        const uint32_t oy = (f.idx / L.dcols) * L.domain_stride * a.scale; // both <= 65535
        // frc1dec_step's base with the reference's pitch: every tap lies inside the domain patch, whose offsets
        // are below the plane's span <= 2^32, so base and the steps are kept modulo 2^32
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
        uint32_t d1 = frc1_step_x(q.y, a.stride), d2 = frc1_step_y(q.y, a.stride);
        uint32_t p = q.x + 2 * lx * d1 + 2 * ly * d2;
        uint32_t out = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            if (x0 + j < a.w) {
                out |= inter_pixel(a.src, p, d1, d2, s, o) << (8 * j);
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
        acc = inter_finish<kWrite, kSse>(io, x0, y, a.w, out);
    }
    if (kSse)
        inter_reduce(io, acc);
}

// The same for a quadtree stream.  a: frq1dec_step's arguments with src = the reference, stride = its pitch
// (frq1_place builds the tap offsets from it); a.tgt is not used.
template <bool kWrite, bool kSse>
__global__ void __launch_bounds__(256) inter_frq1(Frq1StepArgs a, Frq1Layout L, InterOut io)
{
    const uint32_t y = blockIdx.y * kFrc1TileH + (threadIdx.x >> 4);
    const uint32_t x0 = blockIdx.x * kFrc1TileW + (threadIdx.x & 15u) * 4u;
    uint32_t acc = 0;
    if (y < a.h && x0 < a.w) {
        Frq1Place f = frq1_place(a, L, x0, y);
        uint32_t out = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            if (x0 + j < a.w) {
                out |= inter_pixel(a.src, f.p, f.d1, f.d2, f.s, f.o) << (8 * j);
                f.p += 2 * f.d1;
                if (++f.lx == f.R && j < 3 && x0 + j + 1 < a.w) // the next pixel lies in another leaf
                    f = frq1_place(a, L, x0 + j + 1, y);
            }
        }
        acc = inter_finish<kWrite, kSse>(io, x0, y, a.w, out);
    }
    if (kSse)
        inter_reduce(io, acc);
}

struct InterApplyArgs {
    const uint8_t* ref;
    uint8_t* dst;
    uint32_t rpitch, dpitch;
    const frac_encode_item* items;
    uint32_t n;
};

// one wave per item, as decode_apply: the domain patch read in `ref`, the range written in `dst`
__global__ void __launch_bounds__(256) inter_apply(InterApplyArgs a)
{
    const uint32_t it = blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (it >= a.n)
        return;
    const frac_encode_item e = a.items[it];
    const uint32_t sw = e.match.sw, sh = e.match.sh;
    if (sw == 0 || sh == 0)
        return; // no domain: the range keeps the reference's pixels
    const double s = e.match.score.contrast, o = e.match.score.brightness;
    const int t = e.match.score.transform;
    for (uint32_t q = lane; q < e.w * e.h; q += 64) {
        const uint32_t x = q % e.w, y = q / e.w;
        const uint32_t sx = (x * sw) / e.w, sy = (y * sh) / e.h;
        const double smp = (double)sample_sum_dev(a.ref, a.rpitch, e.match.x, e.match.y, sw, sh, sx, sy, t) / 4.0;
        const double v = __fma_rn(s, smp, o);
        a.dst[(size_t)(e.y + y) * a.dpitch + e.x + x] = v < 0.0 ? 0 : v > 255 ? 255 : (uint8_t)v;
    }
}

} // namespace fracenc
