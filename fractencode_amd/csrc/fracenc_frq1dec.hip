// fracenc_frq1dec.hip — FRQ1 quadtree streams decoded on the device, at any integer scale.
//
//   frq1dec_level   the layout pass, once per call and level: one thread per node of the level.  The node's
//                   rank r among the level's split bits is the exclusive prefix sum of the bitmap's per-dword
//                   popcounts (hipcub::DeviceScan over a popcount iterator, enqueued before the kernel) plus
//                   the popcount of the bits below it in its own dword.  A split node writes its quadrants'
//                   origins at 4r .. 4r + 3 of the next level's node array; a leaf (record i − r of the level)
//                   reads its record's bit window as frc1dec_records does, counts an index above / equal to
//                   its level's domain count into the status pair, writes its 16-byte entry and, for the
//                   fast path, its leaf number into every cell it covers of a map at min_size granularity
//   frq1dec_step    one Decoder2 iteration of a stream whose leaves tile the frame, each with a domain:
//                   frc1dec_step's pixel mapping (a workgroup owns 64×16 output pixels, a lane 4 consecutive
//                   pixels of a row, stored as one dword); a lane finds its leaf through the cell map and
//                   looks it up again when its local x reaches the leaf's scaled side inside the dword.
//                   The leaf entries are read straight from global memory, not staged in LDS: the leaves
//                   under a tile are an irregular set (1 to 256 of them at 16/8/4/2), the lanes of one leaf
//                   read the same 16 bytes (one request), and a tile's entries are contiguous per level, so
//                   they stay in L1/L2 between rows
//   frq1dec_expand  every other stream (margins, domain-less leaves, the stepwise flag): the leaves as scaled
//                   frac_encode_items for decode_apply / decode_fused
// fractencode_amd/codec.py unpack_quadtree_stream is the host restatement the tests compare against.
#include "fracenc_common.h"

#include <hipcub/hipcub.hpp>

namespace fracenc {

struct Frq1Popc {
    __host__ __device__ uint32_t operator()(uint32_t w) const { return (uint32_t)__builtin_popcount(w); }
};

// What the header and the host's walk fix for one level, by value.
struct Frq1Level {
    uint32_t n_nodes;
    uint32_t lg;                  // log2 of the level's side
    uint32_t cols0;               // level 0: columns of its node grid (origins computed); else 0 (node array)
    uint32_t has_bitmap;          // 0: the last level, every node a leaf
    uint32_t bitmap_word, rec_word; // dword offsets of the sections in the body
    uint32_t leaf_base;           // leaf number of the level's first leaf
    uint32_t n_domains, index_bits, t_bits, c_bits, b_bits, record_bits;
    uint32_t mcols, cell_lg;      // the cell map: columns (0: no map) and log2 of the cell side (min_size)
};

// status[0]: leaves whose index exceeds their level's domain count; status[1]: leaves without a domain
__global__ void __launch_bounds__(256) frq1dec_level(const uint32_t* __restrict__ words, Frq1Level L,
                                                     const uint32_t* __restrict__ rank,
                                                     const uint32_t* __restrict__ nodes, uint32_t* __restrict__ next,
                                                     uint4* __restrict__ leaves, uint32_t* __restrict__ map,
                                                     uint32_t* __restrict__ status)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.n_nodes)
        return;
    const uint32_t n = 1u << L.lg;
    uint32_t x, y;
    if (L.cols0) {
        x = (i % L.cols0) << L.lg;
        y = (i / L.cols0) << L.lg;
    } else {
        const uint32_t xy = nodes[i];
        x = xy & 0xffffu;
        y = xy >> 16;
    }
    uint32_t r = 0;
    if (L.has_bitmap) {
        const uint32_t word = words[L.bitmap_word + (i >> 5)], b = i & 31u;
        r = rank[i >> 5] + (uint32_t)__popc(word & ((1u << b) - 1u));
        if ((word >> b) & 1u) { // split: top-left, top-right, bottom-left, bottom-right
            const uint32_t h = n >> 1;
            next[4 * r + 0] = x | (y << 16);
            next[4 * r + 1] = (x + h) | (y << 16);
            next[4 * r + 2] = x | ((y + h) << 16);
            next[4 * r + 3] = (x + h) | ((y + h) << 16);
            return;
        }
    }
    const uint32_t j = i - r; // the leaf's record within the level
    const uint64_t bit = (uint64_t)j * L.record_bits, w = L.rec_word + (bit >> 5);
    const uint32_t sh = (uint32_t)(bit & 31u);
    // stream bits [bit, bit + 64) lie in dwords w .. w + 2 (the buffer is padded by kFrc1PadWords)
    const unsigned long long lo = (unsigned long long)words[w] | ((unsigned long long)words[w + 1] << 32);
    unsigned long long rec = lo >> sh;
    if (sh)
        rec |= (unsigned long long)words[w + 2] << (64u - sh);
    if (L.record_bits < 64)
        rec &= (1ull << L.record_bits) - 1ull;
    const uint32_t idx = frc1_take(rec, L.index_bits), t = frc1_take(rec, L.t_bits);
    const uint32_t qc = frc1_take(rec, L.c_bits), qb = frc1_take(rec, L.b_bits);
    if (idx > L.n_domains)
        atomicAdd(&status[0], 1u);
    else if (idx == L.n_domains)
        atomicAdd(&status[1], 1u);
    const uint32_t leaf = L.leaf_base + j;
    // (an index above the domain count fails the call: only its low 24 bits are kept here)
    leaves[leaf] = make_uint4(x | (y << 16), (idx & 0xffffffu) | (t << 24) | (L.lg << 28), qc, qb);
    if (L.mcols) {
        const uint32_t cx = x >> L.cell_lg, cy = y >> L.cell_lg, cn = n >> L.cell_lg; // cn <= 8
        for (uint32_t v = 0; v < cn; ++v)
            for (uint32_t u = 0; u < cn; ++u)
                map[(size_t)(cy + v) * L.mcols + cx + u] = leaf;
    }
}

// The rest of the header, by value to the step and expand kernels.
struct Frq1Layout {
    uint32_t n_leaves;
    uint32_t dc1, dc2, dc3, dc4; // domain grid columns of the levels of side 2, 4, 8, 16 (at least 1)
    uint32_t nd1, nd2, nd3, nd4; // their domain counts
    double c_step, c_min, b_step, b_min; // as Frc1Layout's
};

__device__ inline uint32_t frq1_by_lg(uint32_t lg, uint32_t v1, uint32_t v2, uint32_t v3, uint32_t v4)
{
    return lg == 1 ? v1 : lg == 2 ? v2 : lg == 3 ? v3 : v4;
}

__global__ void __launch_bounds__(256) frq1dec_expand(const uint4* __restrict__ leaves, Frq1Layout L, uint32_t scale,
                                                      frac_encode_item* __restrict__ items)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.n_leaves)
        return;
    const uint4 q = leaves[i];
    const uint32_t lg = q.y >> 28, n = 1u << lg, idx = q.y & 0xffffffu;
    const bool has = idx < frq1_by_lg(lg, L.nd1, L.nd2, L.nd3, L.nd4);
    const uint32_t dc = frq1_by_lg(lg, L.dc1, L.dc2, L.dc3, L.dc4);
    frac_encode_item e;
    e.x = (q.x & 0xffffu) * scale;
    e.y = (q.x >> 16) * scale;
    e.w = e.h = n * scale;
    e.match.score.distance = 0.0;
    e.match.score.contrast = has ? frc1_value(q.z, L.c_step, L.c_min) : 0.0;
    e.match.score.brightness = has ? frc1_value(q.w, L.b_step, L.b_min) : 0.0;
    e.match.score.transform = has ? (int32_t)((q.y >> 24) & 15u) : 0;
    e.match.score._pad = 0;
    e.match.x = has ? (idx % dc) * n * scale : 0u;
    e.match.y = has ? (idx / dc) * n * scale : 0u;
    e.match.sw = e.match.sh = has ? 2 * n * scale : 0u;
    items[i] = e;
}

// (a2 + a3) and (a6 + a7) of the transform LUT, one bit each, of transform t in bits 2t and 2t + 1: the
// domain's tap of local (0, 0) lies (a2 + a3)(S − 1) columns and (a6 + a7)(S − 1) rows from its origin
constexpr uint32_t frq1_org_codes()
{
    uint32_t k = 0;
    for (int t = 0; t < 8; ++t) {
        const Aff a = lut(t);
        k |= (uint32_t)((a.a2 + a.a3) | ((a.a6 + a.a7) << 1)) << (2 * t);
    }
    return k;
}
constexpr uint32_t kFrq1Org = frq1_org_codes();

struct Frq1StepArgs {
    const uint8_t* src;
    uint8_t* tgt;
    uint32_t stride; // plane row stride, a multiple of 64 (inter_frq1: the reference's pitch, any value)
    uint32_t w, h;   // scaled plane
    uint32_t scale;
    uint32_t cell;   // scaled side of a map cell: min_size · scale
    uint32_t mcols;  // map columns
    const uint32_t* map;  // [rows · mcols] leaf number per cell
    const uint4* leaves;  // [n_leaves] validated entries, each with a domain
};

// A lane's place in the leaf that holds output pixel (x, y).
struct Frq1Place {
    uint32_t R, lx;  // the leaf's scaled side; the pixel's local column
    uint32_t p;      // plane offset of the first tap of the pixel (modulo 2^32, as frc1dec_step's)
    uint32_t d1, d2; // tap steps per local column / row
    double s, o;
};

__device__ inline Frq1Place frq1_place(const Frq1StepArgs& a, const Frq1Layout& L, uint32_t x, uint32_t y)
{
    const uint4 q = a.leaves[a.map[(size_t)(y / a.cell) * a.mcols + x / a.cell]];
    const uint32_t lg = q.y >> 28, t = (q.y >> 24) & 7u, idx = q.y & 0xffffffu;
    const uint32_t dc = frq1_by_lg(lg, L.dc1, L.dc2, L.dc3, L.dc4);
    Frq1Place f;
    f.R = a.scale << lg;
    f.lx = x - (q.x & 0xffffu) * a.scale;
    const uint32_t ly = y - (q.x >> 16) * a.scale;
    const uint32_t ox = (idx % dc) * f.R, oy = (idx / dc) * f.R; // the level's lattice step is its side; <= 65535
    const uint32_t S1 = 2 * f.R - 1, org = kFrq1Org >> (2 * t);
    // sample_sum_dev's first tap of local (sx, sy) = (2·lx, 2·ly): base + sx·d1 + sy·d2 (frc1dec_step)
    const uint32_t base = (oy + ((org >> 1) & 1u) * S1) * a.stride + ox + (org & 1u) * S1;
    f.d1 = frc1_step_x(t, a.stride);
    f.d2 = frc1_step_y(t, a.stride);
    f.p = base + 2 * f.lx * f.d1 + 2 * ly * f.d2;
    f.s = frc1_value(q.z, L.c_step, L.c_min);
    f.o = frc1_value(q.w, L.b_step, L.b_min);
    return f;
}

// grid: (⌈w / 64⌉, ⌈h / 16⌉); thread t: row t / 16 of the tile, pixels 4·(t % 16) .. + 3
__global__ void __launch_bounds__(256) frq1dec_step(Frq1StepArgs a, Frq1Layout L, const DecodeState* __restrict__ st,
                                                    unsigned long long* __restrict__ partial)
{
    if (st->done)
        return;
    __shared__ unsigned long long part[4];
    const uint32_t y = blockIdx.y * kFrc1TileH + (threadIdx.x >> 4);
    const uint32_t x0 = blockIdx.x * kFrc1TileW + (threadIdx.x & 15u) * 4u;
    uint32_t acc = 0;
    if (y < a.h && x0 < a.w) {
        Frq1Place f = frq1_place(a, L, x0, y);
        const size_t off = (size_t)y * a.stride + x0; // dword-aligned: stride % 64 == 0, x0 % 4 == 0
        const uint32_t old = *reinterpret_cast<const uint32_t*>(a.src + off);
        uint32_t out = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            if (x0 + j < a.w) {
                const int sum = (int)a.src[f.p] + (int)a.src[f.p + f.d1] + (int)a.src[f.p + f.d2] +
                                (int)a.src[f.p + f.d1 + f.d2];
                const double v = __fma_rn(f.s, (double)sum / 4.0, f.o);
                const uint32_t nv = v < 0.0 ? 0u : v > 255 ? 255u : (uint32_t)(uint8_t)v;
                const int d = (int)((old >> (8 * j)) & 255u) - (int)nv;
                acc += (uint32_t)(d * d);
                out |= nv << (8 * j);
                f.p += 2 * f.d1;
                if (++f.lx == f.R && j < 3 && x0 + j + 1 < a.w) // the next pixel lies in another leaf
                    f = frq1_place(a, L, x0 + j + 1, y);
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
