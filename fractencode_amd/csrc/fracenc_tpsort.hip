// fracenc_tpsort.hip — the tiled SEA form's sort (fracenc_tp.hip): a stable least-significant-digit sort of
// (uint32 key, uint32 value) pairs with 8-bit digits, both of the form's sides — the domains and the ranges —
// in the same launches.  The keys are (bucket << 16) | Σ, 16 to 19 bits: two passes, three with buckets.
//
// Per pass, over fixed chunks of kTpSortChunk consecutive items (one workgroup per chunk; side 0's chunks come
// first in the grid, then side 1's):
//   tp_sort_count    the chunk's 256-bin digit histogram, to table[side][digit][chunk]: every word of the
//                    table is written by exactly one workgroup, so nothing is zeroed beforehand;
//   tp_sort_offsets  the exclusive scan of each side's table in digit-major, chunk-minor order, in two parts:
//                    here one wave per digit scans the digit's row over the chunks in place and writes the
//                    row's sum to total[side][digit]; the 256 sums are scanned by every scatter workgroup.
//                    total[digit's scan] + table[digit][chunk] is where the chunk's first item with that
//                    digit goes;
//   tp_sort_scatter  each wave ranks its 64-item rounds by digit with a ballot match (equal digits keep their
//                    order) on top of per-wave counters in LDS, the counters become wave bases over the
//                    chunk's offsets, and every item is written at its base + rank.
// Ordering comes from the kernel boundaries alone: no workgroup waits for another, no look-back, no fill.
// The passes alternate between the caller's two buffer pairs; tp_sort_pairs says where the result lies.
#include "fracenc_common.h"

namespace fracenc {

constexpr uint32_t kTpSortChunk = 2048;   // items per workgroup
constexpr uint32_t kTpSortThreads = 256;  // four waves, kTpSortChunk / 256 rounds of 64 items each
constexpr uint32_t kTpSortRounds = kTpSortChunk / kTpSortThreads;
static_assert(kTpSortChunk % kTpSortThreads == 0 && kTpSortThreads == 256, "one thread per digit, whole rounds");

struct TpSortSide {
    const uint32_t* kin;
    const uint32_t* vin;
    uint32_t* kout;
    uint32_t* vout;
    uint32_t n;
    uint32_t nchunks; // ⌈n / kTpSortChunk⌉
    uint32_t* table;  // [256][nchunks]
    uint32_t* total;  // [256] items per digit (tp_sort_offsets)
};

struct TpSortArgs {
    TpSortSide a, b;
    uint32_t shift; // the pass's digit: (key >> shift) & 255
};

// chunks of a side, and the words of both sides' tables (side 0's, side 1's, then the two sides' 256 digit
// totals): 64-bit, for any n < 2^32
constexpr size_t tp_sort_chunks(size_t n) { return (n + kTpSortChunk - 1) / kTpSortChunk; }
constexpr size_t tp_sort_table_words(size_t na, size_t nb)
{
    return 256 * (tp_sort_chunks(na) + tp_sort_chunks(nb)) + 2 * 256;
}
static_assert(tp_sort_chunks(0) == 0 && tp_sort_chunks(1) == 1 && tp_sort_chunks(kTpSortChunk) == 1 &&
              tp_sort_chunks(kTpSortChunk + 1) == 2 && tp_sort_chunks(0xffffffffull) == (1ull << 32) / kTpSortChunk);
static_assert(tp_sort_table_words(0, 0) == 512 && tp_sort_table_words(1, kTpSortChunk) == 1024 &&
              tp_sort_table_words(0xffffffffull, 0xffffffffull) == 512 * ((1ull << 32) / kTpSortChunk) + 512);
// a table index stays below 2^32: 256 · ⌈(2^32 − 1) / chunk⌉ = 2^40 / chunk
static_assert(256ull * tp_sort_chunks(0xffffffffull) <= 0xffffffffull, "table indices are 32-bit");

// the side a workgroup belongs to (selected field by field: the arguments stay in the kernel's argument block)
__device__ __forceinline__ TpSortSide tp_sort_side(const TpSortArgs& s, bool second)
{
    TpSortSide r;
    r.kin = second ? s.b.kin : s.a.kin;
    r.vin = second ? s.b.vin : s.a.vin;
    r.kout = second ? s.b.kout : s.a.kout;
    r.vout = second ? s.b.vout : s.a.vout;
    r.n = second ? s.b.n : s.a.n;
    r.nchunks = second ? s.b.nchunks : s.a.nchunks;
    r.table = second ? s.b.table : s.a.table;
    r.total = second ? s.b.total : s.a.total;
    return r;
}

__global__ void __launch_bounds__(kTpSortThreads) tp_sort_count(TpSortArgs s)
{
    __shared__ uint32_t hist[256];
    const bool second = blockIdx.x >= s.a.nchunks;
    const TpSortSide sd = tp_sort_side(s, second);
    const uint32_t chunk = blockIdx.x - (second ? s.a.nchunks : 0u);
    const uint32_t base = chunk * kTpSortChunk, rem = sd.n - base; // (chunk < nchunks: rem ≥ 1)
    hist[threadIdx.x] = 0u;
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < kTpSortRounds; ++j) {
        const uint32_t off = j * kTpSortThreads + threadIdx.x;
        if (off < rem)
            atomicAdd(&hist[(sd.kin[base + off] >> s.shift) & 255u], 1u);
    }
    __syncthreads();
    sd.table[threadIdx.x * sd.nchunks + chunk] = hist[threadIdx.x];
}

// inclusive scan of x across the wave
__device__ __forceinline__ uint32_t tp_sort_wave_scan(uint32_t x, uint32_t lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)x, o, 64);
        if (lane >= (uint32_t)o)
            x += up;
    }
    return x;
}

// One wave per (side, digit): the digit's row of the table, its counts chunk by chunk, becomes their exclusive
// scan in place, and the row's sum goes to total[digit].  The scan across the digits, 256 values, is left to
// every scatter workgroup: a scan of the whole table in one workgroup per side was this sort's longest kernel.
__global__ void __launch_bounds__(kTpSortThreads) tp_sort_offsets(TpSortArgs s)
{
    constexpr uint32_t kPerSide = 256 / (kTpSortThreads / 64); // workgroups per side
    const bool second = blockIdx.x >= kPerSide;
    const uint32_t nchunks = second ? s.b.nchunks : s.a.nchunks;
    if (nchunks == 0)
        return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t digit = (blockIdx.x - (second ? kPerSide : 0u)) * (kTpSortThreads / 64) + (threadIdx.x >> 6);
    uint32_t* row = (second ? s.b.table : s.a.table) + digit * nchunks;
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < nchunks; c0 += 64u) { // (wave-uniform bounds)
        const bool in = c0 + lane < nchunks;
        const uint32_t v = in ? row[c0 + lane] : 0u;
        const uint32_t inc = tp_sort_wave_scan(v, lane);
        if (in)
            row[c0 + lane] = carry + inc - v;
        carry += (uint32_t)__shfl((int)inc, 63, 64);
    }
    if (lane == 0)
        (second ? s.b.total : s.a.total)[digit] = carry;
}

__global__ void __launch_bounds__(kTpSortThreads) tp_sort_scatter(TpSortArgs s)
{
    constexpr uint32_t kWaves = kTpSortThreads / 64;
    __shared__ uint32_t cnt[kWaves][256]; // per wave and digit: items so far, then the wave's base
    __shared__ uint32_t wtot[kWaves];     // items of each wave's 64 digits
    const bool second = blockIdx.x >= s.a.nchunks;
    const TpSortSide sd = tp_sort_side(s, second);
    const uint32_t chunk = blockIdx.x - (second ? s.a.nchunks : 0u);
    const uint32_t base = chunk * kTpSortChunk, rem = sd.n - base;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (uint32_t k = 0; k < kWaves; ++k)
        cnt[k][threadIdx.x] = 0u;
    // thread = digit: where this chunk's items with the digit begin — the digits' totals scanned across the
    // workgroup (the wave's part here, the waves before it after the barrier) plus the digit's row offset
    const uint32_t dtot = sd.total[threadIdx.x];
    const uint32_t dinc = tp_sort_wave_scan(dtot, lane);
    uint32_t dbase = dinc - dtot + sd.table[threadIdx.x * sd.nchunks + chunk];
    if (lane == 63u)
        wtot[wv] = dinc;
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k + 1 < kWaves; ++k)
        dbase += k < wv ? wtot[k] : 0u;
    // wave wv holds items [wv·R·64, (wv + 1)·R·64) of the chunk, round j its next 64: item order is
    // (wave, round, lane) order, which the ranks below keep
    uint32_t key[kTpSortRounds], val[kTpSortRounds], rank[kTpSortRounds];
#pragma unroll
    for (uint32_t j = 0; j < kTpSortRounds; ++j) {
        const uint32_t off = (wv * kTpSortRounds + j) * 64u + lane;
        const bool valid = off < rem;
        key[j] = valid ? sd.kin[base + off] : 0u;
        val[j] = valid ? sd.vin[base + off] : 0u;
    }
#pragma unroll
    for (uint32_t j = 0; j < kTpSortRounds; ++j) {
        const uint32_t off = (wv * kTpSortRounds + j) * 64u + lane;
        const bool valid = off < rem;
        const uint32_t d = (key[j] >> s.shift) & 255u;
        unsigned long long peers = __builtin_amdgcn_ballot_w64(valid); // the valid lanes with this lane's digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __builtin_amdgcn_ballot_w64(bit);
            peers &= bit ? m : ~m;
        }
        const uint32_t before = (uint32_t)__popcll(peers & below);
        const uint32_t pre = cnt[wv][d]; // every peer reads the count, then the first of them raises it
        __builtin_amdgcn_wave_barrier();
        if (valid && before == 0u)
            cnt[wv][d] = pre + (uint32_t)__popcll(peers);
        __builtin_amdgcn_wave_barrier();
        rank[j] = pre + before;
    }
    __syncthreads();
    { // thread = digit: the waves' counts become their bases over the chunk's offset
        uint32_t g = dbase;
#pragma unroll
        for (uint32_t k = 0; k < kWaves; ++k) {
            const uint32_t t = cnt[k][threadIdx.x];
            cnt[k][threadIdx.x] = g;
            g += t;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < kTpSortRounds; ++j) {
        const uint32_t off = (wv * kTpSortRounds + j) * 64u + lane;
        if (off < rem) {
            const uint32_t pos = cnt[wv][(key[j] >> s.shift) & 255u] + rank[j];
            sd.kout[pos] = key[j];
            sd.vout[pos] = val[j];
        }
    }
}

// One side's buffers: the pairs to sort in key / val; key2 / val2 the other pair of the same size.
struct TpSortBufs {
    uint32_t* key;
    uint32_t* val;
    uint32_t* key2;
    uint32_t* val2;
    uint32_t n;
};

// passes of a sort on the low `bits` key bits, and whether its result lies in the second pair (an odd count)
constexpr uint32_t tp_sort_passes(uint32_t bits) { return (bits + 7u) / 8u; }
constexpr bool tp_sort_in_second(uint32_t bits) { return (tp_sort_passes(bits) & 1u) != 0; }

// Sorts both sides on the low `bits` key bits, 3 launches per pass on `stream`; `table` holds
// tp_sort_table_words(a.n, b.n) words.  A side with n = 0 takes no part.  The result lies in key2 / val2 when
// tp_sort_in_second(bits), else in key / val.
inline hipError_t tp_sort_pairs(uint32_t* table, const TpSortBufs& a, const TpSortBufs& b, uint32_t bits,
                                hipStream_t stream)
{
    const uint32_t ca = (uint32_t)tp_sort_chunks(a.n), cb = (uint32_t)tp_sort_chunks(b.n);
    if (ca + cb == 0)
        return hipSuccess;
    TpSortArgs s;
    s.a.n = a.n;
    s.a.nchunks = ca;
    s.a.table = table;
    s.b.n = b.n;
    s.b.nchunks = cb;
    s.b.table = table + (size_t)256 * ca;
    s.a.total = table + (size_t)256 * (ca + cb);
    s.b.total = s.a.total + 256;
    const uint32_t passes = tp_sort_passes(bits);
    for (uint32_t p = 0; p < passes; ++p) {
        const bool fwd = (p & 1u) == 0;
        s.a.kin = fwd ? a.key : a.key2;
        s.a.vin = fwd ? a.val : a.val2;
        s.a.kout = fwd ? a.key2 : a.key;
        s.a.vout = fwd ? a.val2 : a.val;
        s.b.kin = fwd ? b.key : b.key2;
        s.b.vin = fwd ? b.val : b.val2;
        s.b.kout = fwd ? b.key2 : b.key;
        s.b.vout = fwd ? b.val2 : b.val;
        s.shift = 8u * p;
        tp_sort_count<<<ca + cb, kTpSortThreads, 0, stream>>>(s);
        tp_sort_offsets<<<2 * 256 / (kTpSortThreads / 64), kTpSortThreads, 0, stream>>>(s);
        tp_sort_scatter<<<ca + cb, kTpSortThreads, 0, stream>>>(s);
    }
    return hipGetLastError();
}

} // namespace fracenc
