// fracenc_tp.hip — the SEA engine's tiled form for n = 8, T = 4 (FRAC_FORM_SEA_MFMA):
// the successive-elimination bound of fracenc_sea.hip applied per tile pair, with the
// exhaustive engine's Fourier MFMA kernel doing the arithmetic.
//
//   * domains of each classifier bucket sorted by ΣD4 into 32-domain tiles (tile_pos), each
//     tile with its [min, max] ΣD4; ranges of each bucket sorted by ΣR into 32-range blocks,
//     groups of 8 blocks per workgroup as in the exhaustive search;
//   * seed: the Fourier search over one tile per group (the tile nearest its middle block's
//     ΣR), tp_seed_windows turning each range's maximum into U_r, the least exact error over
//     that tile (any real candidate's error bounds the range's minimum from above);
//   * then, in the same launch: per group the tiles whose ΣD4 interval meets [min ΣR − D, max ΣR + D],
//     D² = n²·(max(U, H) + 1/2) over the group's ranges: outside it (ΣR − ΣD)²/n² alone
//     exceeds the bound, so no candidate there can win, tie or hit (fracenc_sea.hip);
//   * search_dft<…, CHUNKED> over each group's window in 4-tile chunks.  The tiles are in ΣD4
//     order, not domain order, so every chunk attaining a lane's maximum counts: the wave that
//     holds a block sees all of its window's chunks and keeps, per lane, the maximum, how many
//     chunks attain it and the first kTpRecList of them, one 16-byte record per lane
//     (DftArgs::rec, nblocks·64 records: sized by the layout, not by the windows).  resolve_dft
//     re-derives the least selection key over the listed chunks, or over the whole window when
//     more attain the maximum than are listed: ties still go to the earliest domain, then the
//     later transform.  The seed search is the same kernel over a one-tile window and writes
//     the same records, which tp_seed_windows reads before the windowed search replaces them.
// Both sides are sorted by fracenc_tpsort.hip, in the same launches on the run's stream.
// Nothing is sized from the windows; the host still waits once per run, for the totals
// (frac_stats, and AUTO's budget test), which tp_plan sums into its pinned block.  (Queueing the windowed
// search before that wait, behind a device-side budget test, measured no gain: DESIGN §7.9.)
// Records are identical to the exhaustive search's; the cost is data-dependent.
#include "fracenc_common.h"

namespace fracenc {

constexpr int kTpMaxBuckets = 8;
// The route reads the planes once, in tp_keys, before the sort: the pixel pass forms every pool row
// (and −ΣD4²) in pool order and copies every range's 64 pixels in range order (rpix), all contiguous stores, with
// the sort keys from the same registers.  After the sort tp_prep permutes: one whole 128-byte pool row per tile
// row and one 64-byte rpix row per slot are its only gathers (dft_domain_build_pair_at<…, ROWS>,
// dft_range_prep_pair_at<…, RPIX>), a tile is one wave, and everything it stores is contiguous per wave.
// DESIGN §7.10, each measured alone against its absence:
// kTpFastSearch: the windowed search runs the exhaustive search's tuned variant (the guarded constant-folded
//   epilogue, the unrolled chunk, wave-uniform buffer_load … lds stages), its per-tile thresholds written by
//   tp_prep with the tile guards; false: the exact epilogue, as the seed search
// kTpLongestFirst: the windowed search's workgroups take the groups by window size, longest first (tp_plan's
//   order); false: in ΣR order, which leaves the longest windows to the middle of the launch
// (A third, tp_prep storing neither the pool nor −ΣD4² — only the fp32 fallback reads them on this route — took
// 0.0035 ms off prep, within the lines' spread, and was taken out.)
constexpr bool kTpFastSearch = true;
constexpr bool kTpLongestFirst = true;

struct TpBuckets {
    uint32_t nb;
    uint32_t tile_first[kTpMaxBuckets], tile_count[kTpMaxBuckets];
    uint32_t dom_begin[kTpMaxBuckets], dom_count[kTpMaxBuckets];   // sorted domain entries
    uint32_t blk_first[kTpMaxBuckets], blk_count[kTpMaxBuckets];
    uint32_t rng_begin[kTpMaxBuckets], rng_count[kTpMaxBuckets];   // sorted ranges
};

__device__ inline uint32_t byte_sum4(uint32_t w)
{
    const uint32_t t = (w & 0x00ff00ffu) + ((w >> 8) & 0x00ff00ffu);
    return (t & 0xffffu) + (t >> 16);
}

// tp_keys: the route's pixel pass, before the sort, in pool and range order — the only kernel of the route that
// reads the planes — with the run's resets, in one launch as dft_prep arranges them.  Blocks [0, dblocks) take the
// domains, the rest the ranges; every thread also takes a grid-stride share of the best_key reset, and thread 0
// clears the fallback count (launch_all leaves both to this kernel).
struct TpKeyArgs {
    const uint8_t* src;
    uint32_t sstride;
    const frac_grid_item* doms;
    const uint32_t* porig;
    uint32_t P;
    const uint32_t* bucket_end;
    uint32_t nb;
    uint32_t* dkey;
    uint32_t* dpos;
    uint32_t* pool;   // [P][32] packed u16 pairs of D4 (tp_prep's gather; fallback_grid)
    int32_t* negsd2;  // [P] (fallback_grid)
    uint32_t dblocks; // blocks of the domain half
    const uint8_t* tgt;
    uint32_t tstride;
    const frac_grid_item* ranges;
    const int32_t* rbucket_idx;
    uint32_t nr;
    uint32_t* rkey;
    uint32_t* rord;
    uint8_t* rpix;    // [nr][64] the ranges' pixels, row-major, in range order (tp_prep's gather)
    unsigned long long* best_key; // nr entries set to ~0 (no candidate yet)
    uint32_t* fb_count;
};

// Domain half: two lanes per pool position, the first phase of dft_domain_build_pair_at — lane h of a position
// loads the plane rows of D4 rows 4h … 4h + 3 and forms the 2×2 sums (pair_sums), that half of the pool row.
// The sort key (bucket << 16) | ΣD4 comes from the same registers: ΣD4, the sum of the row's cells, is the
// domain's pixel sum (≤ 256·255 < 2^16); so does −ΣD4².  A wave's 32 rows are 4 KiB of the pool, contiguous:
// staged through LDS, each of its four store instructions covers 1 KiB of whole lines (straight from the
// registers an instruction would store 16 bytes at a 64-byte stride).
constexpr uint32_t kTpRowQuads = 9; // LDS uint4 per staged row: 8 + 1 of padding (rows stay 16-byte aligned)

__device__ __forceinline__ void tp_domain_rows_at(uint32_t tid2, const TpKeyArgs& a)
{
    __shared__ uint4 rows[128 * kTpRowQuads]; // 256 threads = 128 rows
    const uint32_t p = tid2 >> 1, hh = tid2 & 1u, lane = threadIdx.x & 63u;
    const uint32_t p0 = (tid2 - lane) >> 1; // the wave's first position
    if (p0 >= a.P) // whole waves leave together
        return;
    uint32_t w[16] = {}; // words 16hh … 16hh + 15 of the row: D4 rows 4hh … 4hh + 3, two cells per word
    if (p < a.P) {
        const frac_grid_item d = a.doms[a.porig[p]];
        const uint8_t* base = a.src + (size_t)(d.y + 8 * hh) * a.sstride + d.x;
        if ((((uintptr_t)base | a.sstride) & 7u) == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                // 16 bytes per row: two 8-byte loads (domain origins are 8-byte aligned, not 16)
                const uint2* r0 = reinterpret_cast<const uint2*>(base + (size_t)(2 * i) * a.sstride);
                const uint2* r1 = reinterpret_cast<const uint2*>(base + (size_t)(2 * i + 1) * a.sstride);
                const uint2 a0 = r0[0], a1 = r0[1], b0 = r1[0], b1 = r1[1];
                w[4 * i + 0] = pair_sums(a0.x, b0.x);
                w[4 * i + 1] = pair_sums(a0.y, b0.y);
                w[4 * i + 2] = pair_sums(a1.x, b1.x);
                w[4 * i + 3] = pair_sums(a1.y, b1.y);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const uint8_t* q = base + (size_t)(2 * (k / 4)) * a.sstride + 4 * (k % 4);
                const uint32_t w0 = q[0] | (q[1] << 8) | (q[2] << 16) | ((uint32_t)q[3] << 24);
                const uint8_t* q1 = q + a.sstride;
                const uint32_t w1 = q1[0] | (q1[1] << 8) | (q1[2] << 16) | ((uint32_t)q1[3] << 24);
                w[k] = pair_sums(w0, w1);
            }
        }
    }
    uint32_t sd = 0;
    int sq = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int lo = (int)(w[k] & 0xffffu), hi = (int)(w[k] >> 16);
        sd += (uint32_t)(lo + hi);
        sq += lo * lo + hi * hi;
    }
    uint4* lrow = rows + ((threadIdx.x >> 1) & 127u) * kTpRowQuads + 4 * hh;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        lrow[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    sd += (uint32_t)__shfl_xor((int)sd, 1, 64);
    sq += __shfl_xor(sq, 1, 64);
    if (p < a.P && hh == 0) {
        uint32_t b = 0;
        while (b + 1 < a.nb && p >= a.bucket_end[b])
            ++b;
        a.dkey[p] = (b << 16) | sd;
        a.dpos[p] = p;
        a.negsd2[p] = -sq;
    }
    // the wave's LDS writes above precede its reads below in program order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint4* wrows = rows + ((threadIdx.x >> 6) & 3u) * 32u * kTpRowQuads;
    uint4* out = reinterpret_cast<uint4*>(a.pool + (size_t)p0 * 32);
    const uint32_t nq = min(32u, a.P - p0) * 8u; // the wave's rows in uint4 (the last wave's may be fewer)
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        const uint32_t q = i * 64u + lane;
        if (q < nq)
            out[q] = wrows[(q >> 3) * kTpRowQuads + (q & 7u)];
    }
}

// Range half: two lanes per range, lane h its rows 4h … 4h + 3, as dft_range_prep_pair_at loads them.  The sort
// key is (bucket << 16) | ΣR (ΣR = 4Σr ≤ 65280 < 2^16); the 64 raw pixels go to rpix[r], row-major, a lane pair's
// two 16-byte stores each completing a 64-byte row and a wave's rows contiguous.
__device__ __forceinline__ void tp_range_rows_at(uint32_t gid2, const TpKeyArgs& a)
{
    const uint32_t r = gid2 >> 1, hh = gid2 & 1u;
    if (r >= a.nr) // lane pairs leave together
        return;
    const frac_grid_item rg = a.ranges[r];
    const uint8_t* base = a.tgt + (size_t)(rg.y + 4 * hh) * a.tstride + rg.x;
    uint2 w[4];
    if ((((uintptr_t)base | a.tstride) & 7u) == 0) {
        // one 8-byte load per row (range origins on the 8-pixel grid)
#pragma unroll
        for (int y = 0; y < 4; ++y)
            w[y] = *reinterpret_cast<const uint2*>(base + (size_t)y * a.tstride);
    } else {
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const uint8_t* q = base + (size_t)y * a.tstride;
            w[y] = make_uint2(q[0] | (q[1] << 8) | (q[2] << 16) | ((uint32_t)q[3] << 24),
                              q[4] | (q[5] << 8) | (q[6] << 16) | ((uint32_t)q[7] << 24));
        }
    }
    uint32_t s = 0;
#pragma unroll
    for (int y = 0; y < 4; ++y)
        s += byte_sum4(w[y].x) + byte_sum4(w[y].y);
    uint4* out = reinterpret_cast<uint4*>(a.rpix + (size_t)r * 64 + 32 * hh);
    out[0] = make_uint4(w[0].x, w[0].y, w[1].x, w[1].y);
    out[1] = make_uint4(w[2].x, w[2].y, w[3].x, w[3].y);
    s += (uint32_t)__shfl_xor((int)s, 1, 64);
    if (hh == 0) {
        a.rkey[r] = ((uint32_t)a.rbucket_idx[r] << 16) | (4u * s);
        a.rord[r] = r;
    }
}

__global__ void __launch_bounds__(256) tp_keys(TpKeyArgs a)
{
    const uint32_t gt = blockIdx.x * blockDim.x + threadIdx.x;
    for (uint32_t i = gt; i < a.nr; i += gridDim.x * blockDim.x)
        a.best_key[i] = ~0ull;
    if (gt == 0)
        *a.fb_count = 0u;
    if (blockIdx.x < a.dblocks)
        tp_domain_rows_at(gt, a);
    else
        tp_range_rows_at((blockIdx.x - a.dblocks) * blockDim.x + threadIdx.x, a);
}

// tile rows from the sorted domain order (−1: a padding row, which tp_prep fills as dft_prep does); per tile
// [min, max] ΣD4 of its valid rows
__device__ __forceinline__ void tp_build_tiles_at(uint32_t gid, const TpBuckets& bk,
                                                  const uint32_t* __restrict__ skey,
                                                  const uint32_t* __restrict__ spos, uint32_t ntiles,
                                                  int32_t* __restrict__ tile_pos, uint2* __restrict__ tile_sd)
{
    if (gid >= ntiles * 32u)
        return;
    const uint32_t tile = gid >> 5, row = gid & 31u;
    uint32_t b = 0;
    while (b + 1 < bk.nb && tile >= bk.tile_first[b] + bk.tile_count[b])
        ++b;
    const uint32_t k = (tile - bk.tile_first[b]) * 32u + row;
    const bool valid = k < bk.dom_count[b];
    const uint32_t p = valid ? spos[bk.dom_begin[b] + k] : 0u;
    tile_pos[gid] = valid ? (int32_t)p : -1;
    if (row == 0) {
        const uint32_t last = min(k + 31u, bk.dom_count[b] - 1u);
        tile_sd[tile] = valid ? make_uint2(skey[bk.dom_begin[b] + k] & 0xffffu,
                                           skey[bk.dom_begin[b] + last] & 0xffffu)
                              : make_uint2(0xffffffffu, 0u);
    }
}

// range slots from the sorted range order; per block [min, max] ΣR of its valid slots
__device__ __forceinline__ void tp_build_slots_at(uint32_t gid, const TpBuckets& bk,
                                                  const uint32_t* __restrict__ rkey,
                                                  const uint32_t* __restrict__ rord, uint32_t nblocks,
                                                  int32_t* __restrict__ slot_range,
                                                  uint32_t* __restrict__ range_slot, uint2* __restrict__ blk_sr,
                                                  uint32_t* __restrict__ blk_u)
{
    if (gid >= nblocks * 32u)
        return;
    const uint32_t blk = gid >> 5, col = gid & 31u;
    uint32_t b = 0;
    while (b + 1 < bk.nb && blk >= bk.blk_first[b] + bk.blk_count[b])
        ++b;
    const uint32_t k = (blk - bk.blk_first[b]) * 32u + col;
    const bool valid = k < bk.rng_count[b];
    const uint32_t r = valid ? rord[bk.rng_begin[b] + k] : 0u;
    slot_range[gid] = valid ? (int32_t)r : -1;
    if (valid)
        range_slot[r] = gid;
    if (col == 0) {
        const uint32_t last = min(k + 31u, bk.rng_count[b] - 1u);
        blk_sr[blk] = make_uint2(rkey[bk.rng_begin[b] + k] & 0xffffu, rkey[bk.rng_begin[b] + last] & 0xffffu);
        blk_u[blk] = 0u;
    }
}

// tp_build: the tiles and the slots in one launch after both sorts; blocks [0, tblocks) take the tiles
struct TpBuildArgs {
    TpBuckets bk;
    const uint32_t* skey; // sorted domain keys and positions
    const uint32_t* spos;
    uint32_t ntiles;
    int32_t* tile_pos;
    uint2* tile_sd;
    uint32_t tblocks;     // blocks of the tile half
    const uint32_t* rkey; // sorted range keys and indices
    const uint32_t* rord;
    uint32_t nblocks;
    int32_t* slot_range;
    uint32_t* range_slot;
    uint2* blk_sr;
    uint32_t* blk_u;
};

__global__ void __launch_bounds__(256) tp_build(TpBuildArgs a)
{
    if (blockIdx.x < a.tblocks)
        tp_build_tiles_at(blockIdx.x * blockDim.x + threadIdx.x, a.bk, a.skey, a.spos, a.ntiles, a.tile_pos, a.tile_sd);
    else
        tp_build_slots_at((blockIdx.x - a.tblocks) * blockDim.x + threadIdx.x, a.bk, a.rkey, a.rord, a.nblocks,
                          a.slot_range, a.range_slot, a.blk_sr, a.blk_u);
}

// seed work: per group the one tile of its bucket nearest the ΣR of its middle block
__device__ __forceinline__ void tp_seed_work_at(uint32_t gi, const uint4* __restrict__ groups, uint32_t ngroups,
                                                const uint2* __restrict__ blk_sr, const uint2* __restrict__ tile_sd,
                                                uint4* __restrict__ work)
{
    if (gi >= ngroups)
        return;
    const uint4 gr = groups[gi];
    const uint2 s = blk_sr[gr.x + gr.y / 2];
    const uint32_t SR = (s.x + s.y) / 2;
    uint32_t lo = 0, hi = gr.w - 1; // first tile whose max ΣD4 reaches SR (else the last)
    while (lo < hi) {
        const uint32_t m = (lo + hi) / 2;
        if (tile_sd[gr.z + m].y < SR)
            lo = m + 1;
        else
            hi = m;
    }
    work[gi] = make_uint4(gr.x, gr.y, gr.z + lo, gr.z + lo + 1);
}

// tp_prep: everything the seed search reads, in one launch after tp_build.  Blocks [0, dblocks) build the domain
// tiles, one wave per tile and two lanes per tile row, from the pool rows tp_keys wrote (dft_domain_build_pair_at,
// ROWS): fragments, constants, the tile-order pool copy, the padding rows, and — a wave reduction — the tile's
// guard terms and its fast-epilogue threshold trmax[tile] (null: not written).  The four entries of padding after
// trmax[ntiles], which a chunk's one scalar load may touch, are written here too, by the first workgroup.  The next
// rblocks build the range blocks, two lanes per slot, from rpix (dft_range_prep_pair_at, RPIX), and the trailing
// blocks the seed work, which reads only what tp_build wrote.
struct TpSeedWorkArgs {
    const uint4* groups = nullptr;
    uint32_t ngroups = 0; // 0: no seed work in this launch
    const uint2* blk_sr = nullptr;
    const uint2* tile_sd = nullptr;
    uint4* work = nullptr;
};

__global__ void __launch_bounds__(256) tp_prep(MfmaDomainPrepArgs d, DftDomainBuildArgs s, uint2* __restrict__ tguard,
                                               int32_t* __restrict__ trmax, uint32_t dblocks, MfmaRangePrepArgs r,
                                               uint32_t* __restrict__ rguard, uint32_t rblocks, TpSeedWorkArgs w)
{
    // one stage for whichever half the workgroup runs (the domain rows are the larger)
    static_assert(128 * kDbRowWords * 4 >= 128 * kDrRowBytes, "the range half's pixels fit the domain half's rows");
    __shared__ uint32_t stage[128 * kDbRowWords];
    if (blockIdx.x < dblocks) {
        if (trmax && blockIdx.x == 0 && threadIdx.x < 4u)
            trmax[d.ntiles + threadIdx.x] = -1; // (padding: masked out by dft_guard_bits)
        dft_domain_build_pair_at<true>(blockIdx.x * blockDim.x + threadIdx.x, d, s, tguard, trmax,
                                                        stage);
    } else if (blockIdx.x < dblocks + rblocks) {
        dft_range_prep_pair_at<true>((blockIdx.x - dblocks) * blockDim.x + threadIdx.x, r, rguard,
                                                         stage);
    } else {
        tp_seed_work_at((blockIdx.x - dblocks - rblocks) * blockDim.x + threadIdx.x, w.groups, w.ngroups, w.blk_sr,
                        w.tile_sd, w.work);
    }
}

// per block: the seed search's maximum y over the seed tile gives each slot U = 16Σa² − y, the
// least exact error over that tile (exact regime; else no bound); the block's bound is the
// greatest U over its slots (a 32-lane reduction, one writer per block)
// (every lane of the block's 32-lane row returns the bound)
__device__ __forceinline__ uint32_t tp_seed_reduce_row(uint32_t blk, uint32_t col, bool live,
                                                       const uint4* __restrict__ rec,
                                                       const int32_t* __restrict__ slot_range,
                                                       const uint32_t* __restrict__ rconst)
{
    uint32_t u = 0u;
    if (live && slot_range[blk * 32u + col] >= 0) {
        const size_t e = (size_t)blk * 64u + col; // the slot's two row halves (search_dft CHUNKED)
        const float y = fmaxf(__uint_as_float(rec[e].x), __uint_as_float(rec[e + 32].x));
        const int64_t sa16 = (int64_t)rconst[blk * 32u + col];
        // y = 16Σa² − min S16 is exact while min S16 < 2^24 (fracenc_dft.hip)
        u = y > (float)(sa16 - kExactLimit) ? (uint32_t)(sa16 - (int64_t)y) : 0xffffffffu;
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1)
        u = max(u, (uint32_t)__shfl_xor((int)u, o, 64));
    return u;
}

// per group of ≤ 8 blocks: the tile window
struct TpWindowArgs {
    const uint4* groups;  // [ngroups] {first block, nblocks, tile_first, tile_count} (static)
    uint32_t ngroups;
    const uint2* blk_sr;
    uint32_t* blk_u;      // [nblocks] the seed bound of each block (written here)
    const uint4* rec;     // the seed search's records, one per block and lane
    const int32_t* slot_range;
    const uint32_t* rconst;
    const uint2* tile_sd;
    int64_t hitH;         // −1: no hits
    uint4* work;          // [ngroups] {first block, nblocks, t0, t1}
    uint32_t* pairs;      // [ngroups] block × tile pairs searched (frac_stats.matrix_flops)
    TpBuckets bk;
    unsigned long long* evals; // [ngroups] (range, domain) pairs in the window (frac_stats.evaluated_mappings)
    unsigned long long* sevals; // [ngroups] (range, domain) pairs of the seed tile, read from work (tp_prep)
};

// one group's window from its blocks' seed bounds (su), with the sums the totals are made of; one thread
__device__ __forceinline__ void tp_seed_window_at(const TpWindowArgs& a, uint32_t gi, const uint4& gr, const uint32_t* su)
{
    const uint32_t seed = a.work[gi].z; // the seed search's tile, before the window replaces it
    uint32_t srlo = 0xffffffffu, srhi = 0, u = 0;
    for (uint32_t k = 0; k < gr.y; ++k) {
        const uint2 s = a.blk_sr[gr.x + k];
        srlo = min(srlo, s.x);
        srhi = max(srhi, s.y);
        u = max(u, su[k]);
    }
    uint32_t t0 = gr.z, t1 = gr.z + gr.w; // the whole bucket when no bound is known
    if (u != 0xffffffffu && gr.w) {
        const double bound = fmax((double)u, (double)a.hitH) + 0.5;
        // (ΣR − ΣD)² / 64 ≤ bound  ⇔  |ΣR − ΣD| ≤ √(64·bound); +1 keeps the rounding conservative
        const int64_t D = (int64_t)sqrt(64.0 * bound) + 1;
        const int64_t lo = (int64_t)srlo - D, hi = (int64_t)srhi + D;
        uint32_t a0 = 0, a1 = gr.w; // first tile with max ΣD4 ≥ lo
        while (a0 < a1) {
            const uint32_t m = (a0 + a1) / 2;
            if ((int64_t)a.tile_sd[gr.z + m].y < lo)
                a0 = m + 1;
            else
                a1 = m;
        }
        uint32_t b0 = a0, b1 = gr.w; // first tile with min ΣD4 > hi
        while (b0 < b1) {
            const uint32_t m = (b0 + b1) / 2;
            if ((int64_t)a.tile_sd[gr.z + m].x <= hi)
                b0 = m + 1;
            else
                b1 = m;
        }
        t0 = gr.z + a0;
        t1 = gr.z + max(a0, b0);
    }
    a.work[gi] = make_uint4(gr.x, gr.y, t0, t1);
    a.pairs[gi] = gr.y * (t1 - t0);
    // the (range, domain) pairs among them: the bucket's last block and last tile are partly padding
    uint32_t b = 0;
    while (b + 1 < a.bk.nb && !(a.bk.tile_count[b] && a.bk.tile_first[b] == gr.z))
        ++b;
    const uint32_t slots = min(gr.y * 32u, a.bk.rng_count[b] - (gr.x - a.bk.blk_first[b]) * 32u);
    const uint32_t r0 = (t0 - gr.z) * 32u, r1 = min((t1 - gr.z) * 32u, a.bk.dom_count[b]);
    a.evals[gi] = (unsigned long long)slots * (r1 > r0 ? r1 - r0 : 0u);
    const uint32_t s0 = (seed - gr.z) * 32u;
    a.sevals[gi] = (unsigned long long)slots * (min(s0 + 32u, a.bk.dom_count[b]) - s0);
}

// tp_seed_windows: one workgroup per group.  Each 32-lane row reduces the seed search's records of one block of
// the group to its bound (tp_seed_reduce_row) and writes blk_u; one thread then sets the group's window.
__global__ void __launch_bounds__(256) tp_seed_windows(TpWindowArgs a)
{
    __shared__ uint32_t su[kDftBlocksPerWG];
    const uint32_t gi = blockIdx.x;
    const uint4 gr = a.groups[gi];
    {
        const uint32_t k = threadIdx.x >> 5, col = threadIdx.x & 31u;
        const bool live = k < gr.y;
        const uint32_t bu = tp_seed_reduce_row(gr.x + k, col, live, a.rec, a.slot_range, a.rconst);
        if (live && col == 0) {
            a.blk_u[gr.x + k] = bu;
            su[k] = bu;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0)
        tp_seed_window_at(a, gi, gr, su);
}

// tp_plan: the totals the host needs, in one workgroup: tot[0..8) = {0, 0, Σ pairs (u64), Σ evals (u64), Σ seed
// evals (u64)} over the groups, written straight into the host's pinned block (read after the stream
// synchronisation).  The first two words once held the chunk and entry-link counts; nothing is sized from the
// windows now, and no scan is left.  (Summing them in tp_seed_windows' last workgroup instead — a device-scope
// fence and a counter per group — saved the launch and measured 0.02 ms slower at C3: DESIGN §7.7.)
// order (kTpLongestFirst; null: none): the groups by pairs[g] descending in kTpOrderClasses classes of equal width
// up to the largest, by group index within a class — a stable counting sort, so the order is deterministic and
// equal windows keep the identity.  The windowed search's workgroup n takes group order[n]: the hardware hands
// workgroups to the first free place, which with the longest first is the list-scheduling rule (§7.10).
// Thread t counts the classes of its own run of ⌈ngroups / 256⌉ consecutive groups in its own column of cnt
// (class-major, so the flattened [class][thread] order is the output order), the columns are scanned in place —
// thread t taking kTpOrderClasses consecutive counters, padded against bank conflicts — and each thread places
// its groups from its counters.
constexpr uint32_t kTpPlanThreads = 256;
constexpr uint32_t kTpOrderClasses = 32;

__global__ void __launch_bounds__(kTpPlanThreads) tp_plan(uint32_t ngroups, const uint32_t* __restrict__ pairs,
                                                          const unsigned long long* __restrict__ evals,
                                                          const unsigned long long* __restrict__ sevals,
                                                          uint32_t* __restrict__ tot, uint32_t* __restrict__ order)
{
    constexpr uint32_t NT = kTpPlanThreads, NC = kTpOrderClasses, NW = NT / 64;
    __shared__ unsigned long long part[3][NW];
    __shared__ uint32_t pmax[NW], wsum[NW];
    __shared__ uint32_t cnt[NC * NT + NC * NT / 32];
    unsigned long long s = 0, v = 0, q = 0;
    uint32_t pm = 0;
    for (uint32_t g = threadIdx.x; g < ngroups; g += NT) {
        const uint32_t pg = pairs[g];
        s += pg;
        pm = max(pm, pg);
        v += evals[g];
        q += sevals[g];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        v += __shfl_xor(v, o, 64);
        q += __shfl_xor(q, o, 64);
        pm = max(pm, (uint32_t)__shfl_xor((int)pm, o, 64));
    }
    if ((threadIdx.x & 63u) == 0) {
        part[0][threadIdx.x >> 6] = s;
        part[1][threadIdx.x >> 6] = v;
        part[2][threadIdx.x >> 6] = q;
        pmax[threadIdx.x >> 6] = pm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0, e = 0, se = 0;
        for (uint32_t k = 0; k < NW; ++k) {
            t += part[0][k];
            e += part[1][k];
            se += part[2][k];
        }
        tot[0] = 0u;
        tot[1] = 0u;
        tot[2] = (uint32_t)t;
        tot[3] = (uint32_t)(t >> 32);
        tot[4] = (uint32_t)e;
        tot[5] = (uint32_t)(e >> 32);
        tot[6] = (uint32_t)se;
        tot[7] = (uint32_t)(se >> 32);
    }
    if (!order)
        return;
    for (uint32_t k = 0; k < NW; ++k)
        pm = max(pm, pmax[k]);
    // class 0 holds the largest windows, class NC − 1 the empty ones
    auto cls = [&](uint32_t pg) { return NC - 1u - (uint32_t)(((uint64_t)pg * NC) / ((uint64_t)pm + 1u)); };
    auto at = [](uint32_t i) { return i + (i >> 5); }; // one word of padding per 32
    const uint32_t per = (ngroups + NT - 1) / NT;
    const uint32_t g0 = min(threadIdx.x * per, ngroups), g1 = min(g0 + per, ngroups);
    for (uint32_t c = 0; c < NC; ++c)
        cnt[at(c * NT + threadIdx.x)] = 0u;
    for (uint32_t g = g0; g < g1; ++g)
        ++cnt[at(cls(pairs[g]) * NT + threadIdx.x)];
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t k = 0; k < NC; ++k)
        mine += cnt[at(threadIdx.x * NC + k)];
    uint32_t inc = mine; // the inclusive scan over the workgroup's threads
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)inc, o, 64);
        inc += (threadIdx.x & 63u) >= (uint32_t)o ? up : 0u;
    }
    if ((threadIdx.x & 63u) == 63u)
        wsum[threadIdx.x >> 6] = inc;
    __syncthreads();
    uint32_t run = inc - mine;
    for (uint32_t k = 0; k < (threadIdx.x >> 6); ++k)
        run += wsum[k];
    for (uint32_t k = 0; k < NC; ++k) {
        const uint32_t i = at(threadIdx.x * NC + k), n = cnt[i];
        cnt[i] = run;
        run += n;
    }
    __syncthreads();
    for (uint32_t g = g0; g < g1; ++g)
        order[cnt[at(cls(pairs[g]) * NT + threadIdx.x)]++] = g;
}

} // namespace fracenc
