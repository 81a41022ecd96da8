// fracenc_dft.hip — rotation-group (C4) Fourier form of the MFMA search, n = 8, T = 4.
//
// The reference's four transforms (Id, R90, R180, R270; transformmatcher.h:41-45) act on
// the n×n decimated grid as g^t for the single permutation g = fwd(1): fwd(t) = g^t
// (checked at compile time below).  The 64 pixels split into 16 orbits {q, gq, g²q, g³q}
// and with a = r − 128 (range), b = D4 − 512 (domain), per orbit o, k = 0..3:
//
//   Z_t = Σ_p a(p)·b(g^t p) = Σ_o Σ_k a_{o,k}·b_{o,k+t}           (cyclic correlation)
//
// Per orbit let s = x0 + x2, u = x1 + x3, α = a0 − a2, β = a1 − a3, γ = b0 − b2, δ = b1 − b3.
// The length-4 DFT of the correlation gives, with
//   U = Σ(s_a s_b + u_a u_b),  U' = Σ(s_a u_b + u_a s_b),  Pr = Σ(αγ + βδ),  Pi = Σ(βγ − αδ):
//
//   2Z_0 = U + Pr,  2Z_2 = U − Pr,  2Z_1 = U' − Pi,  2Z_3 = U' + Pi
//
// so  2·max_t Z_t = max(U + |Pr|, U' + |Pi|)  and, with S16 = Σ(4r − D4)² = 16Σa² − 8Z + Σb²,
// the statistic whose maximum over domains the search wants is
//
//   y = 8·max_t Z_t − Σb²  =  16Σa² − min_t S16.
//
// The six-MFMA form (the only one: 6 MFMA 32x32x16 per 32 domains × 32 ranges, against the direct
// form's T·n²/16 = 16).  The DFT has two real bins and one complex bin.  The real bins are
//   P = Σ(s_a + u_a)(s_b + u_b) = U + U',   M = Σ(s_a − u_a)(s_b − u_b) = U − U'      (K = 16 each)
// and M is accumulated onto P inside the MFMA, once with +(s_a − u_a) and once with −(s_a − u_a):
// 2U = P + M and 2U' = P − M cost no VALU.  The complex bin Pr + iPi = Σ(α + iβ)(γ − iδ) takes
// Gauss's three products, the last two accumulated onto the first inside the MFMA:
//   k1 = Σγ(α + β),   Pr = k1 + Σ(γ − δ)(−β),   Pi = k1 + Σ(−δ − γ)α,
// with the range operands doubled, so the accumulators hold 2Pr and 2Pi.  Fragments (K = 16 orbits):
//   domain tile   [s_b + u_b | s_b − u_b | γ | γ − δ | −δ − γ]                          (kDftKS = 5)
//   range block   [s_a + u_a | s_a − u_a | u_a − s_a | 2(α + β) | −2β | 2α]             (kDftNBF = 6)
// The search tracks h = y/2 = 4·max_t Z_t − Σb²/2 per lane: the tile's row constant is −Σb²/2 — exact
// in f32 (Σb² ≤ 2^24, so a half-integer of magnitude ≤ 2^23) —
//   h = max(2U + |2Pr|, 2U' + |2Pi|) − Σb²/2                      (dft_tile_max6, 4.5 VALU a candidate)
// and what leaves the search is y = 2h (a power-of-two scale: exact).
//
// Exactness (f16 operands, f32 accumulate; a ∈ [−128, 127], b ∈ [−512, 508]; every value an integer):
//   operands  |s_b ± u_b|, |γ − δ|, |δ + γ| ≤ 2048, |γ| ≤ 1020;  |s_a ± u_a| ≤ 512, |2(α + β)| ≤ 1020,
//             |2α|, |2β| ≤ 510 — integers of magnitude ≤ 2048 are exact in f16;
//   2U, 2U'   with A0 = s_a + u_a, A2 = s_a − u_a (B0, B2 on the domain side), |A0| + |A2| =
//             2·max(|s_a|, |u_a|) ≤ 512 and |B0|, |B2| ≤ 2048: every partial sum of P ± M, in any
//             accumulation order, is bounded by Σ_o(|A0·B0| + |A2·B2|) ≤ 16·512·2048 = 2^24: exact;
//   2Pr, 2Pi  partial sums ≤ 2·(16·510·1020 + 16·255·2040) = 33,292,800 < 2^25, all even: exact;
//   2U + |2Pr| = 4·max(Z_0, Z_2) and 2U' + |2Pi| = 4·max(Z_1, Z_3), of magnitude ≤ 2^24: exact;
//   h         one rounding of exact operands, exact whenever |y| ≤ 2^24, which holds for every candidate in
//             the exact regime S16 < 2^24 (y = 16Σa² − S16, 16Σa² ≤ 2^24).  Candidates with S16 ≥ 2^24
//             may round, but rounding is monotone: their y ≤ 16Σa² − 2^24 (exactly representable) stays
//             ≤ it, so they never beat or tie an exact-regime candidate, and a range whose maximum reaches
//             that bound goes to the fp32 fallback (App. A.3), as with the direct engine.
// The guarded fast path (kDftFast6, dft_tile_max6g) starts the P GEMM from C = −Σb²/2, so both
// accumulators built on P carry the constant: u' = 2U − Σb²/2, v' = 2U' − Σb²/2, and
//   h = max(u' + |2Pr|, v' + |2Pi|)              — 2 v_add + 1 v_max3 per candidate instead of 4.5 VALU.
// Every partial sum of u', v' (C included, any accumulation order) is a half-integer of magnitude
// ≤ Σb²/2 + Σ_o(|A0||B0| + |A2||B2|) ≤ Σb²/2 + R6·D6, with R6 = Σ_o(|s_a + u_a| + |s_a − u_a|) per range
// and D6 = max_o max(|s_b + u_b|, |s_b − u_b|) per domain; f32 holds every half-integer below 2^23, so
// the partial sums are exact whenever
//   2·R6·D6 + Σb² < 2^24.
// The guard is taken per (range block, domain tile) from the block's max R6 (rguard) and the tile's max 2·D6
// and max Σb² (tguard, folded into one threshold on R6: trmax); a tile pair that fails it runs the exact
// epilogue.  2Pr, 2Pi are exact as above, and u' + |2Pr| = 4·max(Z_0, Z_2) − Σb²/2 is one rounding of exact
// operands — the argument for h (exact in the exact regime, monotone beyond it) holds unchanged.
// An 8-MFMA form (U, U', Pr, Pi as K = 32 GEMMs) and a five-MFMA form (P ± M on the VALU) preceded this one;
// they were measured in DESIGN §7.2 and profiles/r01 – r03 and are gone from the sources.
//
// The per-lane maximum of y and the chunk (4 tiles) it appeared in feed resolve_dft, which re-derives the exact
// (domain, transform) inside the chunk with integer arithmetic.  resolve_dft reads, per slot: the search's own
// merge over its work items (slotbest; the exhaustive route, SORTED = false) or, on the SEA tiled form
// (SORTED = true), the two records search_dft<…, CHUNKED> left for the slot's row halves.
#include "fracenc_common.h"

namespace fracenc {

template <int N>
struct Orbits4 {
    int p[N * N / 4][4]; // p[o][k] = g^k(q_o)
};

template <int N>
constexpr Orbits4<N> make_orbits4()
{
    Orbits4<N> r{};
    bool seen[N * N] = {};
    int o = 0;
    for (int q = 0; q < N * N; ++q) {
        if (seen[q])
            continue;
        int p = q;
        for (int k = 0; k < 4; ++k) {
            r.p[o][k] = p;
            seen[p] = true;
            p = fwd_index<N>(1, p);
        }
        ++o;
    }
    return r;
}

template <int N>
constexpr bool orbits4_valid()
{
    // fwd(t) = g^t for t = 0..3, g^4 = id, and every orbit has exactly four pixels
    for (int q = 0; q < N * N; ++q) {
        int p = q;
        for (int t = 0; t < 4; ++t) {
            if (fwd_index<N>(t, q) != p)
                return false;
            p = fwd_index<N>(1, p);
        }
        if (p != q)
            return false;
    }
    const Orbits4<N> r = make_orbits4<N>();
    int count[N * N] = {};
    for (int o = 0; o < N * N / 4; ++o)
        for (int k = 0; k < 4; ++k)
            ++count[r.p[o][k]];
    for (int q = 0; q < N * N; ++q)
        if (count[q] != 1)
            return false;
    return true;
}

static_assert(orbits4_valid<8>(), "the reference's rotations must be the powers of Rotate_90 with 4-orbits");

// T = 8 on the Fourier path: Flip_Rotate_k = Flip ∘ Rotate_k and Flip ∘ Rotate_k ∘ Flip = Rotate_{−k}
template <int N>
constexpr bool flips_valid()
{
    for (int k = 0; k < 4; ++k)
        for (int p = 0; p < N * N; ++p) {
            if (fwd_index<N>(4 + k, p) != fwd_index<N>(4, fwd_index<N>(k, p)))
                return false;
            if (fwd_index<N>(4, fwd_index<N>(k, fwd_index<N>(4, p))) != fwd_index<N>((4 - k) & 3, p))
                return false;
        }
    return true;
}
static_assert(flips_valid<8>(), "the flip half of T = 8 is the rotation search of the flipped range");
constexpr Orbits4<8> kOrb8 = make_orbits4<8>();
constexpr float kDftPadY = -1.0e30f; // −Σb² of padding rows: y ≈ −1e30 never wins
constexpr int kDftKS = 5;  // domain fragments per tile
constexpr int kDftNBF = 6; // range fragments per block
// Row constants of a Fourier tile: [2][16] f32 = 8 uint4, padded to kDftCS = 16 uint4 per tile in
// memory and in the LDS stage, so a 4-tile stage's constants are exactly one 1 KiB LDS-DMA piece
constexpr uint32_t kDftCS = 16;

// The two forms of search_dft, by their variant words.  The words keep the values the profiles of rounds 3 – 20
// and the tests name them by; of their bits only kDftFast6 still selects anything, and the tuning build's ablation
// bits (8, 16, 32, 64, 256, 512) are ORed onto them.
//   kDftExactVar  the exact epilogue, row constants in registers (dft_tile_max6), the chunk as a loop, stages by
//                 global_load_lds (stage_tiles): the SEA tiled form's seed search, and the A/B of the guard;
//   kDftFastVar   variant 35, the shipped search: the guarded folded epilogue (dft_tile_max6g), the 4-tile chunk
//                 unrolled (LDS reads at immediate offsets from one base) and stages by buffer_load … lds (the
//                 stage base in an SGPR soffset, per-thread offsets fixed: no VALU per piece).
constexpr int kDftExactVar = 9217;
constexpr int kDftFast6 = 16384;
constexpr int kDftFastVar = 123905;
static_assert((kDftFastVar & kDftFast6) != 0 && (kDftExactVar & kDftFast6) == 0 &&
                  ((kDftFastVar | kDftExactVar) & (8 | 16 | 32 | 64 | 256 | 512)) == 0,
              "the variant words");
template <int VAR>
struct DftForm {
    static constexpr bool FAST6 = (VAR & kDftFast6) != 0;
};

constexpr int64_t kFast6Limit = (1ll << 24) - 1; // 2·R6·D6 + Σb² ≤ this
// the guard of a tile with guard terms {gx = max 2·D6, gy = max Σb²} as one threshold on the block's R6:
// R6·gx + gy ≤ kFast6Limit  ⇔  gy ≤ kFast6Limit and R6 ≤ ⌊(kFast6Limit − gy) / gx⌋  (−1: no block passes)
__device__ inline int32_t dft_fast6_rmax(uint32_t gx, uint32_t gy)
{
    return (int64_t)gy > kFast6Limit ? -1
           : gx == 0                  ? INT32_MAX
                                      : (int32_t)min<int64_t>((kFast6Limit - gy) / gx, INT32_MAX);
}

struct DftArgs {
    MfmaSearchArgs m;
    uint32_t* rguard;      // [nblocks]  max over the block's ranges of R6 = Σ_o(|s_a + u_a| + |s_a − u_a|)
    uint4* rec = nullptr;  // CHUNKED: [nblocks·64] per block and lane the window's maximum and the chunks attaining
                           // it, {bits of max y (+inf = hit), n chunks attaining it, the first's word, the second's}
                           // with a chunk's word tile | tile mask << 28 (fracenc_tp.hip)
    const int32_t* trmax;  // kDftFast6: [ntiles] the largest block R6 whose guard holds against the
                           // tile, (kFast6Limit − max Σb²) / max 2·D6 (−1: none)
    const uint32_t* order = nullptr; // CHUNKED: [workgroups] the work item each workgroup takes (null: its own
                                     // index) — the windows longest first (tp_plan, fracenc_tp.hip)
    unsigned long long* stamps = nullptr; // FRAC_CLOCK_STAMP builds only: [workgroups][kClockStampWords]
    // not CHUNKED: per range slot the maximum over every work item, merged here with one 64-bit atomicMax per
    // (slot, work item): fmap(y) << 32 | (kSlotBestTileMax − chunk) << 6 | the chunk's tiles to re-evaluate << 2 |
    // the lane halves of that chunk attaining y.  The greatest word names the greatest y and, among equal y, the
    // earliest chunk.  The tile mask is 0xf unless the search tracked the tiles attaining y (TMASK); 0 = no work
    // item reached the slot.
    unsigned long long* slotbest = nullptr;
};
constexpr uint32_t kSlotBestTileMax = 0x3ffffffu; // chunk tiles below 2^26 (domains < 2^24: tiles < 2^19)
// per workgroup: s_memtime and s_memrealtime before / after the loop, HW_ID | XCC_ID << 32, and the
// work item's tile range first | end << 32
constexpr uint32_t kClockStampWords = 6;

// ---------------------------------------------------------------------------
// The domain half of the preparation: pool_build and the tile fragments in one pass.  The 2×2 sums come straight
// from the plane (SamplerBilinear's integer sum, image/sampler.h:21-38, as pool_build), two cells per 32-bit
// word — (w & 0x00ff00ff) + ((w >> 8) & 0x00ff00ff) over the word of both rows is the packed u16 pair the pool
// stores — and the same registers feed the tile fragments.
// Outputs: the pool and −ΣD4² (read by fit_winner and fallback_grid; on the tiled form's route, whose fit is
// fused into its resolve, only by fallback_grid — not storing them there measured too little: DESIGN §7.10), the
// pool rows again in tile order, orbit order (resolve_dft); per 32-domain tile the kDftKS A fragments (lane l:
// row l&31, orbit 8(l>>5) + j), −Σb²/2 per row in the [2][16] lane-half layout of the epilogue, and the tile's
// guard terms {max 2·D6, max Σb²} with their threshold on R6.  Every pool position sits in exactly one tile row.
// ---------------------------------------------------------------------------
struct DftDomainBuildArgs {
    const uint8_t* src;
    uint32_t sstride;
    const frac_grid_item* doms;
    const uint32_t* porig;      // pool position → domain index
    uint32_t* pool;             // [P][32] packed u16 pairs of D4
    int32_t* negsd2;            // [P]
    uint32_t* tpool;            // [ntiles*32][32] the same rows in tile order, orbit order (resolve_dft)
};

// pair_sums: fracenc_kernels.hip (pool_build)


// dft_domain_build_pair_at: two lanes per tile row.  Lane h of a row loads
// the plane rows of D4 rows 4h … 4h + 3, writes that half of the pool row, and puts it in LDS; each lane
// then reads the cells of orbits 8h … 8h + 7 back (LDS addresses from the orbit table, no register
// indexing) and builds that lane half of the fragments and of the tile-order copy.  Σb², ΣD4² and the
// guard terms meet in a lane-pair shuffle.  (One thread per row ran, on a small frame, one wave per CU on a
// quarter of the CUs — C2: 16 workgroups; the pair halves the chain and doubles the waves.)
// A tile's 32 rows are one wave's 64 lanes, so the tile guards are a wave reduction.
// ROWS (the SEA tiled form's tp_prep, fracenc_tp.hip): the pool rows and −ΣD4² are already there, written in pool
// order by the pixel pass before the sort (tp_keys), so the lane pair reads the plane not at all: lane h loads its
// 64-byte half of pool[p] — p in ΣD4 order, the route's one gather per domain, a whole 128-byte line per pair —
// and writes neither.  Everything after the load is the same code.  Its row stage is the caller's (lds, 128 rows of
// kDbRowWords words), which tp_prep shares with its range half.
constexpr uint32_t kDbRowWords = 33; // LDS words per row: 32 + 1 of padding (rows in distinct banks)
template <bool ROWS = false>
__device__ __forceinline__ void dft_domain_build_pair_at(uint32_t tid2, const MfmaDomainPrepArgs& a,
                                                         const DftDomainBuildArgs& s, uint2* __restrict__ tguard,
                                                         int32_t* __restrict__ trmax, uint32_t* lds = nullptr)
{
    constexpr int KS = kDftKS;
    uint32_t* rows; // 256 threads = 128 rows
    if constexpr (ROWS) {
        rows = lds;
    } else {
        __shared__ uint32_t own[128 * kDbRowWords];
        rows = own;
    }
    const uint32_t hh = tid2 & 1u;
    if ((tid2 >> 1) >= a.ntiles * 32u) // whole tiles (whole waves) leave together
        return;
    const uint32_t gid = tid2 >> 1;
    const uint32_t tile = gid >> 5, row = gid & 31u;
    uint32_t* lrow = rows + ((threadIdx.x >> 1) & 127u) * kDbRowWords;
    const int p = a.tile_pos[gid];
    uint32_t w[16]; // words 16hh … 16hh + 15 of the row: D4 rows 4hh … 4hh + 3, two cells per word
    int sq = 0;
    if constexpr (ROWS) {
        if (p >= 0) {
            const uint4* pr = reinterpret_cast<const uint4*>(s.pool + (size_t)p * 32 + 16 * hh);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint4 v = pr[k];
                w[4 * k + 0] = v.x;
                w[4 * k + 1] = v.y;
                w[4 * k + 2] = v.z;
                w[4 * k + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k)
                w[k] = 0x02000200u; // padding: b = 0
        }
    } else if (p >= 0) {
        const frac_grid_item d = s.doms[s.porig[p]];
        const uint8_t* base = s.src + (size_t)(d.y + 8 * hh) * s.sstride + d.x;
        if ((((uintptr_t)base | s.sstride) & 7u) == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint2* r0 = reinterpret_cast<const uint2*>(base + (size_t)(2 * i) * s.sstride);
                const uint2* r1 = reinterpret_cast<const uint2*>(base + (size_t)(2 * i + 1) * s.sstride);
                const uint2 a0 = r0[0], a1 = r0[1], b0 = r1[0], b1 = r1[1];
                w[4 * i + 0] = pair_sums(a0.x, b0.x);
                w[4 * i + 1] = pair_sums(a0.y, b0.y);
                w[4 * i + 2] = pair_sums(a1.x, b1.x);
                w[4 * i + 3] = pair_sums(a1.y, b1.y);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const uint8_t* q = base + (size_t)(2 * (k / 4)) * s.sstride + 4 * (k % 4);
                const uint32_t w0 = q[0] | (q[1] << 8) | (q[2] << 16) | ((uint32_t)q[3] << 24);
                const uint8_t* q1 = q + s.sstride;
                const uint32_t w1 = q1[0] | (q1[1] << 8) | (q1[2] << 16) | ((uint32_t)q1[3] << 24);
                w[k] = pair_sums(w0, w1);
            }
        }
        uint4* pw = reinterpret_cast<uint4*>(s.pool + (size_t)p * 32 + 16 * hh);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            pw[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int lo = (int)(w[k] & 0xffffu), hi = (int)(w[k] >> 16);
            sq += lo * lo + hi * hi;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            w[k] = 0x02000200u; // padding: b = 0
    }
#pragma unroll
    for (int k = 0; k < 16; ++k)
        lrow[16 * hh + k] = w[k];
    if constexpr (!ROWS) {
        sq += __shfl_xor(sq, 1, 64);
        if (p >= 0 && hh == 0)
            s.negsd2[p] = -sq;
    }
    // the pair's LDS writes above are one wave's and precede its reads below in program order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint16_t* cells = reinterpret_cast<const uint16_t*>(lrow);
    // orbits 8hh … 8hh + 7: their four cells each (the table's entries, selected by the lane half)
    int cv[8][4];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            cv[j][k] = cells[hh ? kOrb8.p[8 + j][k] : kOrb8.p[j][k]];
    if (p >= 0) {
        // the tile-order copy for resolve_dft, orbit o as (D_{o,0} | D_{o,1} << 16), (D_{o,2} | D_{o,3} << 16)
        uint4* tw = reinterpret_cast<uint4*>(s.tpool + (size_t)gid * 32 + 16 * hh);
#pragma unroll
        for (int v = 0; v < 4; ++v)
            tw[v] = make_uint4((uint32_t)cv[2 * v][0] | ((uint32_t)cv[2 * v][1] << 16),
                               (uint32_t)cv[2 * v][2] | ((uint32_t)cv[2 * v][3] << 16),
                               (uint32_t)cv[2 * v + 1][0] | ((uint32_t)cv[2 * v + 1][1] << 16),
                               (uint32_t)cv[2 * v + 1][2] | ((uint32_t)cv[2 * v + 1][3] << 16));
    }
    int sb2 = 0, dinf = 0;
    _Float16 comp[KS][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int b0 = cv[j][0] - 512, b1 = cv[j][1] - 512, b2 = cv[j][2] - 512, b3 = cv[j][3] - 512;
        sb2 += b0 * b0 + b1 * b1 + b2 * b2 + b3 * b3;
        const int sb = b0 + b2, ub = b1 + b3, gb = b0 - b2, db = b1 - b3;
        dinf = max(dinf, max(abs(sb + ub), abs(sb - ub))); // guard term D6
        comp[0][j] = (_Float16)(sb + ub);
        comp[1][j] = (_Float16)(sb - ub);
        comp[2][j] = (_Float16)gb;
        comp[3][j] = (_Float16)(gb - db);
        comp[4][j] = (_Float16)(-db - gb);
    }
#pragma unroll
    for (int st = 0; st < KS; ++st)
        a.dtiles[((size_t)tile * KS + st) * 64 + row + 32 * hh] = __builtin_bit_cast(uint4, comp[st]);
    sb2 += __shfl_xor(sb2, 1, 64);
    dinf = max(dinf, __shfl_xor(dinf, 1, 64));
    if (hh == 0) {
        const float ny = p >= 0 ? -0.5f * (float)sb2 : kDftPadY; // −Σb²/2: exact (Σb² ≤ 2^24)
        const uint32_t h = (row >> 2) & 1u, i = (row & 3u) + 4u * (row >> 3);
        a.dconst[(size_t)tile * (kDftCS * 4) + h * 16 + i] = __float_as_uint(ny);
    }
    uint32_t gx = p >= 0 ? (uint32_t)(2 * dinf) : 0u, gy = p >= 0 ? (uint32_t)sb2 : 0u;
    // the tile's guard terms over its 32 rows (lanes 2·row + hh of one wave): a wave maximum
#pragma unroll
    for (int o = 32; o > 1; o >>= 1) {
        gx = max(gx, (uint32_t)__shfl_xor((int)gx, o, 64));
        gy = max(gy, (uint32_t)__shfl_xor((int)gy, o, 64));
    }
    if (row == 0 && hh == 0) {
        tguard[tile] = make_uint2(gx, gy);
        if (trmax) // the fast path's guard as one threshold on the block's R6
            trmax[tile] = dft_fast6_rmax(gx, gy);
    }
}

// ---------------------------------------------------------------------------
// The range half: per range block the kDftNBF B fragments (lane l: range slot l&31, orbit 8(l>>5) + j), 16Σa² per
// slot, the block's guard term max R6 and, for resolve_dft, the slot's pixels in orbit order (rorb).
// dft_range_prep_pair_at: two lanes per range slot, as the domain build.  Lane h
// loads rows 4h … 4h + 3 of the range into LDS; each lane then reads the pixels of orbits 8h … 8h + 7 back
// (T = 8's flipped copies read through the Flip permutation: the same table, another address) and builds that
// lane half of the fragments and of the orbit-ordered pixel pairs.  Σa² and R6 meet in a lane-pair shuffle;
// a block's 32 slots are one wave, so its guard stays a wave maximum.
// T = 8: a block at or past flip_from is the flipped copy of its range, a'(q) = a(Flip q).  Flip_Rotate_k =
// Flip ∘ Rotate_k (fwd(4 + k, p) = fwd(4, fwd(k, p)), image/transform.h:32-41) and Flip ∘ g^k ∘ Flip = g^−k, so
// Σ_p a(p)·b(fwd(4 + k, p)) = Σ_q a'(q)·b(g^{−k} q): the copy's rotation t' is transform 4 + (−t' mod 4).
// RPIX (the SEA tiled form's tp_prep): the range's 64 pixels come from MfmaRangePrepArgs::rpix, the range-order copy
// the pixel pass stored before the sort (tp_keys): lane h loads its 32-byte half of rpix[ri], no plane row, and the
// pixel stage is the caller's (lds, 128 slots of kDrRowBytes bytes).
// ---------------------------------------------------------------------------
constexpr uint32_t kDrRowBytes = 68; // LDS bytes per slot: 64 + 4 of padding
template <bool RPIX = false>
__device__ __forceinline__ void dft_range_prep_pair_at(uint32_t gid2, const MfmaRangePrepArgs& a,
                                                       uint32_t* __restrict__ rguard, uint32_t* lds = nullptr)
{
    constexpr int N = 8, NBF = kDftNBF;
    constexpr uint32_t kRow = kDrRowBytes;
    uint8_t* px;
    if constexpr (RPIX) {
        px = reinterpret_cast<uint8_t*>(lds);
    } else {
        __shared__ uint8_t own[128 * kRow];
        px = own;
    }
    const uint32_t gid = gid2 >> 1, hh = gid2 & 1u;
    if (gid >= a.nblocks * 32u) // whole blocks (whole waves) leave together
        return;
    const uint32_t b = gid >> 5, col = gid & 31u;
    uint8_t* lp = px + ((threadIdx.x >> 1) & 127u) * kRow;
    const int ri = a.slot_range[gid];
    uint2 w[4] = {make_uint2(0x80808080u, 0x80808080u), make_uint2(0x80808080u, 0x80808080u),
                  make_uint2(0x80808080u, 0x80808080u), make_uint2(0x80808080u, 0x80808080u)}; // empty: a = 0
    if constexpr (RPIX) {
        if (ri >= 0) {
            const uint4* q = reinterpret_cast<const uint4*>(a.rpix + (size_t)ri * 64 + 32 * hh);
            const uint4 v0 = q[0], v1 = q[1];
            w[0] = make_uint2(v0.x, v0.y);
            w[1] = make_uint2(v0.z, v0.w);
            w[2] = make_uint2(v1.x, v1.y);
            w[3] = make_uint2(v1.z, v1.w);
        }
    } else if (ri >= 0) {
        const frac_grid_item rg = a.ranges[ri];
        const uint8_t* base = a.tgt + (size_t)(rg.y + 4 * hh) * a.tstride + rg.x;
        if ((((uintptr_t)base | a.tstride) & 7u) == 0) {
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
    }
    uint32_t* lw = reinterpret_cast<uint32_t*>(lp);
#pragma unroll
    for (int y = 0; y < 4; ++y) {
        lw[8 * hh + 2 * y] = w[y].x;
        lw[8 * hh + 2 * y + 1] = w[y].y;
    }
    // the pair's LDS writes above are one wave's and precede its reads below in program order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // T = 8: the block's flipped copy, a'(q) = a(Flip q)
    const bool flip = ri >= 0 && b >= a.flip_from;
    int av[8][4]; // orbits 8hh … 8hh + 7, their four pixels − 128
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int q0 = kOrb8.p[j][k], q1 = kOrb8.p[8 + j][k];
            const int q = hh ? q1 : q0, qf = hh ? fwd_index<N>(4, q1) : fwd_index<N>(4, q0);
            av[j][k] = (int)lp[flip ? qf : q] - 128;
        }
    int sa2 = 0, r1 = 0;
    _Float16 comp[NBF][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int a0 = av[j][0], a1 = av[j][1], a2 = av[j][2], a3 = av[j][3];
        sa2 += a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3;
        const int sa = a0 + a2, ua = a1 + a3, al = a0 - a2, be = a1 - a3;
        r1 += abs(sa + ua) + abs(sa - ua); // guard term R6
        comp[0][j] = (_Float16)(sa + ua);
        comp[1][j] = (_Float16)(sa - ua);
        comp[2][j] = (_Float16)(ua - sa);
        comp[3][j] = (_Float16)(2 * (al + be));
        comp[4][j] = (_Float16)(-2 * be);
        comp[5][j] = (_Float16)(2 * al);
    }
    if (ri < 0) { // an empty slot's fragments are zero (its pixels read as 128 above: already so), no guard
        sa2 = 0;
        r1 = 0;
    }
#pragma unroll
    for (int f = 0; f < NBF; ++f)
        a.rfrags[((size_t)b * NBF + f) * 64 + col + 32 * hh] = __builtin_bit_cast(uint4, comp[f]);
    sa2 += __shfl_xor(sa2, 1, 64);
    r1 += __shfl_xor(r1, 1, 64);
    if (hh == 0) {
        a.rconst[gid] = ri >= 0 ? (uint32_t)(16 * sa2) : 0u; // 16Σa² ≤ 2^24
        if (a.slotbest)
            a.slotbest[gid] = 0ull; // the run's reset of the search's merged maxima
    }
    if (a.rorb) {
        // raw pixels r = a + 128, orbit o as the pairs (r_{o,0} | r_{o,1} << 16), (r_{o,2} | r_{o,3} << 16)
        uint4* ro = reinterpret_cast<uint4*>(a.rorb + (size_t)gid * 32 + 16 * hh);
#pragma unroll
        for (int v = 0; v < 4; ++v)
            ro[v] = make_uint4((uint32_t)(av[2 * v][0] + 128) | ((uint32_t)(av[2 * v][1] + 128) << 16),
                               (uint32_t)(av[2 * v][2] + 128) | ((uint32_t)(av[2 * v][3] + 128) << 16),
                               (uint32_t)(av[2 * v + 1][0] + 128) | ((uint32_t)(av[2 * v + 1][1] + 128) << 16),
                               (uint32_t)(av[2 * v + 1][2] + 128) | ((uint32_t)(av[2 * v + 1][3] + 128) << 16));
    }
    // the block's guard: a maximum over its 32 slots (lanes 2·col + hh of one wave), one writer
    uint32_t g1 = (uint32_t)r1;
#pragma unroll
    for (int o = 32; o > 1; o >>= 1)
        g1 = max(g1, (uint32_t)__shfl_xor((int)g1, o, 64));
    if (col == 0 && hh == 0)
        rguard[b] = g1;
}

// ---------------------------------------------------------------------------
// dft_prep: the Fourier path's preparation in one launch.  Blocks [0, dblocks) build the domain
// tiles (dft_domain_build_pair_at), the rest prepare the range blocks (dft_range_prep_pair_at), so the two run
// side by side instead of one after the other.  Every thread also takes a grid-stride share of
// the run's best_key reset, and thread 0 sets the fallback count: the two hipMemsetAsync of
// launch_all, whose launches cost more than their bytes on small frames.
// ---------------------------------------------------------------------------
struct DftPrepInit {
    unsigned long long* best_key = nullptr; // nr entries set to ~0 (no candidate yet)
    uint32_t nr = 0;
    uint32_t* fb_count = nullptr; // set to fbc when not null
    uint32_t fbc = 0;
    uint32_t dblocks = 0; // blocks of the domain build
    const DevPlan* plan = nullptr; // device-planned search: tile / block / range counts from the plan
    uint32_t copies = 1;           // with a plan: range blocks per planned block (T = 8 Fourier: 2)
};

__global__ void __launch_bounds__(256) dft_prep(MfmaDomainPrepArgs d, DftDomainBuildArgs s, uint2* __restrict__ tguard,
                                                int32_t* __restrict__ trmax, MfmaRangePrepArgs r,
                                                uint32_t* __restrict__ rguard, DftPrepInit in)
{
    const uint32_t gt = blockIdx.x * blockDim.x + threadIdx.x;
    if (in.plan) {
        d.ntiles = in.plan->ntiles;
        apply_plan(r, in.copies);
        in.nr = in.plan->nr;
    }
    for (uint32_t i = gt; i < in.nr; i += gridDim.x * blockDim.x)
        in.best_key[i] = ~0ull;
    if (gt == 0 && in.fb_count)
        *in.fb_count = in.fbc;
    if (blockIdx.x < in.dblocks)
        dft_domain_build_pair_at(gt, d, s, tguard, trmax); // two lanes per tile row
    else // two lanes per range slot
        dft_range_prep_pair_at((blockIdx.x - in.dblocks) * blockDim.x + threadIdx.x, r, rguard);
}

// ---------------------------------------------------------------------------
// search_dft<HITS, VAR>: the search_mfma work decomposition with workgroups of kDftBlocksPerWG waves = range blocks
// of one bucket, domain tiles staged through LDS, 4 tiles per double-buffered stage; per lane the chunk maximum of
// h over its 16 rows × the stage's tiles (all four transforms folded in).
// ---------------------------------------------------------------------------
// The exact epilogue, row constants in registers (kDftExactVar).  af: the tile's fragments, bf: the block's (the head
// comment); ny = −Σb²/2:  h = max(2U + |2Pr|, 2U' + |2Pi|) − Σb²/2.
__device__ inline float dft_tile_max6(const half8_t (&af)[kDftKS], const half8_t (&bf)[kDftNBF], const floatx16_t& ny, float m)
{
    const floatx16_t z = {};
    const floatx16_t p = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[0], bf[0], z, 0, 0, 0);  // P
    const floatx16_t k1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[2], bf[3], z, 0, 0, 0); // 2k1
    const floatx16_t u = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[1], bf[1], p, 0, 0, 0);  // P + M = 2U
    const floatx16_t pr = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[3], bf[4], k1, 0, 0, 0); // 2Pr
    const floatx16_t v = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[1], bf[2], p, 0, 0, 0);  // P − M = 2U'
    const floatx16_t pi = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[4], bf[5], k1, 0, 0, 0); // 2Pi
    float y[16];
#pragma unroll
    for (int i = 0; i < 16; ++i)
        y[i] = __builtin_fmaxf(u[i] + __builtin_fabsf(pr[i]), v[i] + __builtin_fabsf(pi[i])) + ny[i];
#pragma unroll
    for (int i = 0; i < 16; i += 2)
        m = __builtin_fmaxf(__builtin_fmaxf(m, y[i]), y[i + 1]);
    return m;
}

__device__ inline floatx16_t lds_row_consts(const uint4* p)
{
    floatx16_t r;
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) {
        const uint4 v = p[c4];
        r[4 * c4 + 0] = __uint_as_float(v.x);
        r[4 * c4 + 1] = __uint_as_float(v.y);
        r[4 * c4 + 2] = __uint_as_float(v.z);
        r[4 * c4 + 3] = __uint_as_float(v.w);
    }
    return r;
}

// One tile pair with the guarded fast path (kDftFast6, kDftFastVar).  Both paths issue
// the same six MFMAs; only P's C operand differs — the tile's −Σb²/2 row constants when the guard
// holds, the stage's zero block when it does not (a wave-uniform choice of address, so one MFMA
// sequence and one register allocation serve both) — and the epilogue: the folded form
// (2 VALU + one v_max3 step per candidate), or the exact one with the constants read after the
// MFMAs.  lc: the tile's row constants ([2][16] lane-half layout), h: the lane half.
template <int ABL = 0>
__device__ inline float dft_tile_max6g(const half8_t (&af)[kDftKS], const half8_t (&bf)[kDftNBF], const uint4* la, uint32_t ic,
                                       uint32_t iz, uint32_t h, bool fast, float m)
{
    if constexpr (ABL == 16) {
        // ABLATION (tuning only, wrong results): the fast epilogue on the fragments' bits, no MFMA
        const floatx16_t c = lds_row_consts(la + (fast ? ic : iz) + h * 4);
        auto bits = [&](const half8_t& x, int i) { return __builtin_bit_cast(uint4, x)[i & 3]; };
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float u = c[i] + __uint_as_float(bits(af[i >> 2], i)), pr = __uint_as_float(bits(bf[i >> 2], i));
            const float v = __uint_as_float(bits(af[(i >> 2) + 1], i)), pi = __uint_as_float(bits(bf[(i >> 2) + 2], i));
            m = __builtin_fmaxf(__builtin_fmaxf(m, u + __builtin_fabsf(pr)), v + __builtin_fabsf(pi));
        }
        return m;
    }
    // one base pointer, a selected index: the compiler keeps the read's underlying LDS object and
    // does not wait for the other stage buffer's pending LDS-DMA (a selected pointer made it)
    const uint4* lc = la + ic;
    const floatx16_t c = lds_row_consts(la + (fast ? ic : iz) + h * 4);
    const floatx16_t z = {};
    const floatx16_t k1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[2], bf[3], z, 0, 0, 0); // 2k1
    const floatx16_t p = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[0], bf[0], c, 0, 0, 0);  // P (− Σb²/2)
    const floatx16_t pr = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[3], bf[4], k1, 0, 0, 0); // 2Pr
    const floatx16_t u = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[1], bf[1], p, 0, 0, 0);  // 2U (− Σb²/2)
    const floatx16_t pi = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[4], bf[5], k1, 0, 0, 0); // 2Pi
    const floatx16_t v = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[1], bf[2], p, 0, 0, 0);  // 2U' (− Σb²/2)
    if constexpr (ABL == 8) // ABLATION (tuning only, wrong results): the MFMAs with a one-value epilogue
        return __builtin_fmaxf(m, (u[0] + pr[0]) + (v[0] + pi[0]));
    if (fast) {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            m = __builtin_fmaxf(__builtin_fmaxf(m, u[i] + __builtin_fabsf(pr[i])), v[i] + __builtin_fabsf(pi[i]));
        return m;
    }
    const floatx16_t ny = lds_row_consts(lc + h * 4);
    float y[16];
#pragma unroll
    for (int i = 0; i < 16; ++i)
        y[i] = __builtin_fmaxf(u[i] + __builtin_fabsf(pr[i]), v[i] + __builtin_fabsf(pi[i])) + ny[i];
#pragma unroll
    for (int i = 0; i < 16; i += 2)
        m = __builtin_fmaxf(__builtin_fmaxf(m, y[i]), y[i + 1]);
    return m;
}

// kDftFast6 guard bits of a 4-tile chunk: bit k set iff the block's R6 ≤ tile t0 + k's threshold
// (one scalar load of four thresholds; trmax is padded by 4 entries), masked to the chunk's ne tiles
__device__ inline uint32_t dft_guard_bits(const int32_t* __restrict__ trmax, uint32_t t0, uint32_t ne, uint32_t r1)
{
    t0 = __builtin_amdgcn_readfirstlane(t0);
    const __attribute__((address_space(4))) int32_t* rp =
        (const __attribute__((address_space(4))) int32_t*)(uintptr_t)(trmax + t0);
    const int32_t g0 = rp[0], g1 = rp[1], g2 = rp[2], g3 = rp[3], ri = (int32_t)r1;
    const uint32_t g = ((ri <= g0) ? 1u : 0u) | ((ri <= g1) ? 2u : 0u) | ((ri <= g2) ? 4u : 0u) | ((ri <= g3) ? 8u : 0u);
    return g & ((1u << ne) - 1u);
}

// One 4-tile chunk [q0, q1) of the stage at la (nt tiles): the lane's maximum of h over it.
// MASK (CHUNKED or TMASK search): masks[0] gets the chunk tiles attaining the lane's maximum, masks[1]
// (HITS) the tiles holding a hit (h ≥ hl), bit k for tile q0 + k.  iz: the stage's zero block (kDftFast6).
template <int VAR, bool MASK = false, bool HITS = false>
__device__ inline float dft_compute_stage(const uint4* __restrict__ la, uint32_t nt, uint32_t lane,
                                          const half8_t (&bf)[kDftNBF], uint32_t tb, uint32_t r1, uint32_t q0,
                                          uint32_t q1, uint32_t* masks, float hl, uint32_t iz,
                                          const int32_t* __restrict__ trmax)
{
    constexpr int KS = kDftKS;
    constexpr bool FAST6 = DftForm<VAR>::FAST6;
    const uint4* lc = la + nt * (uint32_t)KS * 64u;
    const uint32_t h = lane >> 5;
    float cm = -__builtin_inff();
    // the chunk's fast-path guards, loaded up front (wave-uniform scalar loads)
    uint32_t gfast = 0;
    // the tile index is wave-uniform: readfirstlane + the constant address space make the guard
    // loads scalar, which the vmcnt waits of the stage's LDS-DMA do not serialise with
    const uint32_t t0 = __builtin_amdgcn_readfirstlane(tb + q0), ne = __builtin_amdgcn_readfirstlane(min(q1, nt) - q0);
    if constexpr (FAST6)
        gfast = dft_guard_bits(trmax, t0, ne, r1);
    auto tile = [&](uint32_t q) {
        // ABLATION bit 32 (tuning only, wrong results): every tile reuses tile 0's operands
        const uint32_t qq = (VAR & 32) ? 0u : q;
        half8_t af[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s)
            af[s] = __builtin_bit_cast(half8_t, la[(qq * KS + s) * 64 + lane]);
        // the tile's maximum folded onto m
        auto tile_max = [&](float m) {
            if constexpr (FAST6) {
                const bool fast = (gfast >> (q - q0)) & 1u; // wave-uniform
                const uint32_t ic = nt * (uint32_t)KS * 64u + qq * kDftCS;
                return dft_tile_max6g<VAR & (8 | 16)>(af, bf, la, ic, iz, h, fast, m);
            } else {
                return dft_tile_max6(af, bf, lds_row_consts(lc + qq * kDftCS + h * 4), m);
            }
        };
        if constexpr (MASK) { // the tile's own maximum first, then the chunk's tiles attaining it
            const float tm = tile_max(-__builtin_inff());
            const uint32_t bit = 1u << (q - q0);
            masks[0] = tm > cm ? bit : (tm == cm ? masks[0] | bit : masks[0]);
            if constexpr (HITS)
                masks[1] |= tm >= hl ? bit : 0u;
            cm = __builtin_fmaxf(cm, tm);
        } else {
            cm = tile_max(cm);
        }
    };
    const uint32_t qe = min(q1, nt);
    if constexpr (FAST6) { // the chunk unrolled
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            if (q0 + k < qe)
                tile(q0 + k);
    } else {
        for (uint32_t q = q0; q < qe; ++q)
            tile(q);
    }
    return cm;
}

constexpr uint32_t kDftBlocksPerWG = 8; // waves (range blocks) sharing one LDS domain stage
// chunks a CHUNKED record lists by word (K of DESIGN §7.7); its count of attaining chunks is exact, so
// the resolve tells "all listed" from "more than listed"
constexpr uint32_t kTpRecList = 2;

// stage_tiles by buffer_load … lds in whole-wave pieces (1 KiB each): the stage's nt·kDftKS A-fragment
// pieces and its one constants piece (kDftCS = 16 uint4 per tile: 4 tiles are one piece; a shorter
// last stage reads the next tiles' constants or the allocation's 1 KiB of slack, never used).  The
// loop, the LDS destination (M0) and the source offset (soffset) are wave-uniform: every piece costs
// scalar instructions only, the lane's voffset (lane·16) is fixed.
__device__ inline void stage_tiles_buf(uint4* dst, __amdgpu_buffer_rsrc_t ra, __amdgpu_buffer_rsrc_t rc, uint32_t tb,
                                       uint32_t nt)
{
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr uint32_t KS = kDftKS, WAVES = kDftBlocksPerWG;
    const uint32_t voff = (threadIdx.x & 63u) * 16u;
    const uint32_t tbu = __builtin_amdgcn_readfirstlane(tb), npa = __builtin_amdgcn_readfirstlane(nt * KS);
    for (uint32_t p = wv; p <= npa; p += WAVES) {
        auto* l = (__attribute__((address_space(3))) void*)(dst + p * 64u);
        if (p < npa)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, l, 16, voff, (tbu * KS + p) * 1024u, 0, 0);
        else
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rc, l, 16, voff, tbu * kDftCS * 16u, 0, 0);
    }
}

// CHUNKED (the SEA engine's tiled form, fracenc_tp.hip): tiles are in ΣD4 order, not domain
// order, so every chunk attaining a lane's maximum matters, not only the first.  One workgroup holds a
// group's whole window and wave w its block wk.x + w throughout, so the lane keeps the running maximum,
// the number of chunks attaining it and the words of the first kTpRecList of them in registers, and
// writes one record per lane when the window is done (DftArgs::rec).  resolve_dft
// re-evaluates the listed chunks, or the whole window when more than the list holds attain the maximum.
// TMASK (not CHUNKED, slotbest): each lane also tracks which tiles of its best chunk attain its maximum (or
// hold a hit), and the slot word carries them, so resolve_dft re-evaluates those tiles instead of the whole
// chunk.  Costs the tile-pair epilogue a compare per tile: chosen where the resolve, not the search, dominates.
template <bool HITS, int VAR, bool CHUNKED = false, bool TMASK = false>
__global__ void __launch_bounds__(64 * kDftBlocksPerWG) search_dft(DftArgs d)
{
    constexpr uint32_t WAVES = kDftBlocksPerWG;
    constexpr uint32_t kTilesPerStage = fracenc::kTilesPerStage; // LDS stage = chunk (resolve_dft): unsigned here
    static_assert(kTilesPerStage == 4, "chunk words, tile masks and the guard load assume 4-tile stages");
    static_assert(kTuningBuild || (VAR & (8 | 16 | 32 | 64 | 256 | 512)) == 0,
                  "search_dft ablations exist only in FRAC_TUNING builds");
    static_assert(!(TMASK && CHUNKED), "CHUNKED records carry their own tile masks");
    if (past_plan(d.m))
        return;
    const MfmaSearchArgs& a = d.m;
    constexpr int KS = kDftKS, NBF = kDftNBF;
    constexpr int STAGE = kTilesPerStage * KS * 64 + kTilesPerStage * kDftCS;
    // kDftFast6: each stage buffer ends in 8 zero uint4, the row constants of a tile pair that runs
    // the exact epilogue (written here, published by the first stage barrier, never a DMA target).
    // Inside the stage's own array, so the compiler still tells these reads from the other
    // buffer's pending LDS-DMA (a separate array made it wait vmcnt(0) before every tile)
    constexpr int ZTAIL = DftForm<VAR>::FAST6 ? 8 : 0;
    __shared__ uint4 lds0[STAGE + ZTAIL];
    __shared__ uint4 lds1[STAGE + ZTAIL];
    if constexpr (DftForm<VAR>::FAST6)
        if (threadIdx.x < 2 * ZTAIL)
            (threadIdx.x < ZTAIL ? lds0 : lds1)[STAGE + (threadIdx.x % ZTAIL)] = make_uint4(0u, 0u, 0u, 0u);
    // (everything below is indexed by the work item's blocks and tiles, not by blockIdx.x)
    const uint4 wk = a.work[(CHUNKED && d.order) ? d.order[blockIdx.x] : blockIdx.x];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const bool active = wv < wk.y;
    const uint32_t blk = wk.x + (active ? wv : 0u);
    const uint32_t r1 = __builtin_amdgcn_readfirstlane(d.rguard[blk]);

    half8_t bf[NBF];
#pragma unroll
    for (int f = 0; f < NBF; ++f)
        bf[f] = __builtin_bit_cast(half8_t, a.rfrags[((size_t)blk * NBF + f) * 64 + lane]);
    float hl = 0.0f;
    if constexpr (HITS) { // S16 ≤ H  ⇔  y ≥ 16Σa² − H  (exact integers below 2^24; halved exactly for h)
        hl = (float)((int32_t)a.rconst[blk * 32 + (lane & 31u)] - (int32_t)a.hitH);
        hl *= 0.5f;
    }
    // the search tracks h = y/2; the records and slot words carry y = 2h (exact)
    constexpr float kOut = 2.0f;

    float best = -__builtin_inff();
    uint32_t btile = 0, bmask = 0xfu;
    uint32_t masks[2] = {0u, 0u};
    uint32_t nbest = 0, word1 = 0, word2 = 0; // CHUNKED: chunks attaining `best`, the first two's words
    auto finish_stage = [&](float cm, uint32_t tb) {
        if constexpr (CHUNKED) {
            static_assert(kTpRecList == 2, "the record lists two chunks");
            // the chunk's word carries its tile mask in bits 28..31 of its tile (resolve_dft<true>
            // evaluates only those tiles): the hit tiles when the chunk holds a hit, else the
            // tiles attaining the maximum
            uint32_t msk = masks[0];
            if constexpr (HITS)
                if (cm >= hl) {
                    cm = __builtin_inff();
                    msk = masks[1];
                }
            const uint32_t word = tb | (msk << 28);
            // (a chunk's maximum is finite or +inf, so the first chunk always starts the list)
            const bool gt = cm > best, eq = cm == best;
            word2 = (eq && nbest == 1u) ? word : word2;
            word1 = gt ? word : word1;
            nbest = gt ? 1u : nbest + (eq ? 1u : 0u);
            best = gt ? cm : best;
            masks[0] = masks[1] = 0u;
            return;
        }
        // any hit in the chunk: the first-hit chunk wins. (A per-tile mask here, as the CHUNKED
        // records carry, cost 4% of this kernel in a 30-sample A/B for 0.1 ms less resolve: only TMASK.)
        uint32_t msk = 0xfu;
        if constexpr (TMASK) {
            msk = masks[0];
            if constexpr (HITS)
                msk = cm >= hl ? masks[1] : msk;
            masks[0] = masks[1] = 0u;
        }
        if constexpr (HITS)
            cm = cm >= hl ? __builtin_inff() : cm;
        if (cm > best) {
            best = cm;
            btile = tb;
            bmask = msk;
        }
    };
    const uint32_t nstage = (wk.w - wk.z + kTilesPerStage - 1) / kTilesPerStage;
    auto stage_nt = [&](uint32_t st) { return min((uint32_t)kTilesPerStage, wk.w - (wk.z + st * kTilesPerStage)); };
    // ABLATION bits (tuning only, wrong results): 64 no LDS-DMA and no barrier after the first
    // stages; 256 no LDS-DMA (barriers kept); 512 no barrier (LDS-DMA kept)
    constexpr bool NODMA = (VAR & 64) != 0;
    constexpr bool SKIPDMA = NODMA || (VAR & 256) != 0, SKIPBAR = NODMA || (VAR & 512) != 0;
    auto stage = [&](uint4* dst, uint32_t tb, uint32_t nt) {
        if constexpr (DftForm<VAR>::FAST6) // raw buffers (no range check: the pieces are in bounds)
            stage_tiles_buf(dst, __builtin_amdgcn_make_buffer_rsrc((void*)a.dtiles, 0, 0xffffffffu, 0x00020000),
                            __builtin_amdgcn_make_buffer_rsrc((void*)a.dconst, 0, 0xffffffffu, 0x00020000), tb, nt);
        else
            stage_tiles<KS, 64 * WAVES, kDftCS>(dst, a.dtiles, a.dconst, tb, nt);
    };
#ifdef FRAC_CLOCK_STAMP
    // diagnostic build only (tools/clock_stamp.py, MI355X_MICROARCH.md "DVFS give-back"): the shader
    // clock over this workgroup's loop is Δs_memtime ÷ Δs_memrealtime × 100 MHz
    const unsigned long long ck0 = __builtin_amdgcn_s_memtime(), rt0 = __builtin_amdgcn_s_memrealtime();
#endif
    if (nstage)
        stage(lds0, wk.z, stage_nt(0));
    for (uint32_t st = 0; st < nstage; st += 2) {
        {
            const uint32_t tb = wk.z + st * kTilesPerStage;
            if (!SKIPBAR || st < 2)
                stage_barrier();
            if (st + 1 < nstage && (!SKIPDMA || st == 0))
                stage(lds1, tb + kTilesPerStage, stage_nt(st + 1));
            for (uint32_t c0 = 0; c0 < stage_nt(st); c0 += 4)
                finish_stage(dft_compute_stage<VAR, CHUNKED || TMASK, HITS>(lds0, stage_nt(st), lane, bf, tb, r1, c0, c0 + 4,
                                                                            masks, hl, STAGE, d.trmax),
                             tb + c0);
        }
        if (st + 1 < nstage) {
            const uint32_t tb = wk.z + (st + 1) * kTilesPerStage;
            if (!SKIPBAR || st < 2)
                stage_barrier();
            if (st + 2 < nstage && !SKIPDMA)
                stage(lds0, tb + kTilesPerStage, stage_nt(st + 2));
            for (uint32_t c0 = 0; c0 < stage_nt(st + 1); c0 += 4)
                finish_stage(dft_compute_stage<VAR, CHUNKED || TMASK, HITS>(lds1, stage_nt(st + 1), lane, bf, tb, r1, c0,
                                                                            c0 + 4, masks, hl, STAGE, d.trmax),
                             tb + c0);
        }
    }
#ifdef FRAC_CLOCK_STAMP
    {
        const unsigned long long ck1 = __builtin_amdgcn_s_memtime(), rt1 = __builtin_amdgcn_s_memrealtime();
        // where the workgroup ran: HW_ID (CU, SE, …) and XCC_ID, read by s_getreg (hwreg 4 and 20)
        const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);
        if (threadIdx.x == 0 && d.stamps) { // vector stores from lane 0; nothing in the kernel reads them
            ulonglong2* sp = reinterpret_cast<ulonglong2*>(d.stamps + (size_t)blockIdx.x * kClockStampWords);
            sp[0] = make_ulonglong2(ck0, ck1);
            sp[1] = make_ulonglong2(rt0, rt1);
            sp[2] = make_ulonglong2((unsigned long long)hw | ((unsigned long long)xcc << 32),
                                    (unsigned long long)wk.z | ((unsigned long long)wk.w << 32));
        }
    }
#endif
    if constexpr (CHUNKED) {
        // an empty window leaves {−inf, 0}: resolve_dft gives the slot the default record
        if (active)
            d.rec[(size_t)blk * 64 + lane] = make_uint4(__float_as_uint(best * kOut), nbest, word1, word2);
    }
    if (active && !CHUNKED) {
        // lanes l and l + 32 hold one range slot's two row halves: the greater y, among equal y the earlier
        // chunk, and which halves attain it there (both: resolve_dft evaluates both halves' rows)
        const uint32_t y0 = fmap(best * kOut), t0 = btile;
        const uint32_t y1 = (uint32_t)__shfl_xor((int)y0, 32, 64), t1 = (uint32_t)__shfl_xor((int)t0, 32, 64);
        const uint32_t m1 = TMASK ? (uint32_t)__shfl_xor((int)bmask, 32, 64) : 0xfu;
        const bool first = lane < 32u;
        const uint32_t ym = first ? y0 : y1, tm = first ? t0 : t1; // this half (lane < 32: half 0)
        const uint32_t yo = first ? y1 : y0, to = first ? t1 : t0; // the other half
        if (first) {
            uint32_t tile = tm, hm = 1u, mk = bmask;
            if (yo > ym || (yo == ym && to < tm)) {
                tile = to;
                hm = 2u;
                mk = m1;
            } else if (yo == ym && to == tm) {
                hm = 3u;
                mk |= m1; // both halves' rows are evaluated on every tile of the union
            }
            const unsigned long long w = ((unsigned long long)max(ym, yo) << 32) |
                                         ((kSlotBestTileMax - tile) << 6) | (mk << 2) | hm;
            atomicMax(d.slotbest + (size_t)blk * 32 + lane, w);
        }
    }
}

// ---------------------------------------------------------------------------
// resolve_dft: one wave per range (resolve_mfma's lane map: tile row i = l>>2, pixel
// slice g = l&3).  The greatest entry y over the block's splits and lane halves gives the
// target error S16 = 16Σa² − y (exact regime) or flags the range for the fp32 fallback;
// the chunk(s) holding it are re-evaluated with exact integers for all four transforms,
// keeping the least selection key (first hit in (domain, transform) order, else least
// error with ties to the earliest domain, then the later transform).
// ---------------------------------------------------------------------------
// SORTED (tiles in ΣD4 order, fracenc_tp.hip): rows and tiles are not in domain order, so the
// least key over every matching row of every tile of the chunk is taken (no first-row shortcut).
// One slot's least key and the winner's sums (bestk = kKeyNone: padding slot, or no eligible domain).
// FLIP: the slot holds a T = 8 range's flipped copy (dft_range_prep_pair_at, flip_from), whose rotation t' is the
// reference's transform 4 + (−t' mod 4); the keys carry the reference's transform and a.T.
struct DftResolved {
    unsigned long long bestk = kKeyNone;
    uint32_t bx = 0, bs1 = 0, bs2 = 0, sr1 = 0, sr2 = 0;
};

// What a slot's resolve loads by the slot alone: the search's merged word, 16Σr², the lane's orbits of the range
// and, SORTED, the slot's two records (its row halves: lanes col and col + 32 of its block) and the block's group.
// Issued together; the grouped resolve issues the next item's before it evaluates the current one.
struct DftSlotLoads {
    unsigned long long sb = 0ull;
    uint32_t sa16 = 0;
    uint4 r0 = make_uint4(0u, 0u, 0u, 0u), r1 = r0, rec0 = r0, rec1 = r0;
    uint2 gw = make_uint2(0xffffffffu, 0u);
};

// (slot < nslots: in bounds whether or not the slot holds a range)
template <bool SORTED>
__device__ inline DftSlotLoads dft_slot_loads(const MfmaResolveArgs& a, uint32_t slot, int lane)
{
    DftSlotLoads ld;
    if constexpr (!SORTED)
        ld.sb = a.slotbest[slot];
    ld.sa16 = a.rconst[slot];
    const uint4* rp4 = reinterpret_cast<const uint4*>(a.rorb + (size_t)slot * 32 + (lane & 3) * 8);
    ld.r0 = rp4[0];
    ld.r1 = rp4[1];
    if constexpr (SORTED) {
        const uint32_t blk = slot >> 5, col = slot & 31u;
        ld.rec0 = a.rec[(size_t)blk * 64 + col];
        ld.rec1 = a.rec[(size_t)blk * 64 + col + 32];
        ld.gw = a.blk_group[blk];
    }
    return ld;
}

// ri: the slot's range (slot_range[slot], which the caller holds; < 0: padding); ld: the slot's loads.
// ONE (SORTED): when a single lane holds a key after the evaluation — one row attains the target, the common
// case — that lane's key and sums are read directly instead of through the 64-lane minimum; the same result.
template <bool SORTED, bool ONE = false>
__device__ inline DftResolved resolve_dft_eval(const MfmaResolveArgs& a, uint32_t slot, int ri, int lane, bool flip,
                                               const DftSlotLoads& ld)
{
    constexpr int PG = 16, T = 4; // T: the rotations evaluated per slot
    const uint32_t TK = a.T;      // the transforms of the keys (4, or 8 with the flipped copies)
    DftResolved res;
    const unsigned long long sb = ld.sb;
    const int64_t sa16 = (int64_t)ld.sa16;
    const int i = lane >> 2, g = lane & 3;
    const uint4 r0 = ld.r0, r1 = ld.r1;
    const uint4 rec0 = ld.rec0, rec1 = ld.rec1;
    const uint2 gw = ld.gw;
    if (ri < 0)
        return res;
    // lane (i, g) holds orbits 4g..4g+3 of the range as pixel pairs (dft_range_prep_pair_at) and meets
    // the same orbits of a domain row (tile-order pool, dft_domain_build_pair_at). With fwd(t) = g^t,
    //   X_t = Σ_q r(q)·D4(fwd_t q) = Σ_{o,k} r_{o,k}·D_{o,k+t}:
    // t = 0 pairs (A, B) = (D0|D1, D2|D3), t = 2 the swapped pairs (B, A), t = 1 the rotated
    // pairs (D1|D2, D3|D0) = (alignbit(B, A, 16), alignbit(A, B, 16)) and t = 3 those swapped —
    // two v_alignbit per orbit for all four transforms.
    const uint32_t rp[PG / 2] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
    constexpr uint32_t kOnes = 0x00010001u;
    uint32_t sr2u = 0, sr1 = 0;
#pragma unroll
    for (int q = 0; q < PG / 2; ++q) {
        sr2u = __builtin_amdgcn_udot2(__builtin_bit_cast(ushort2_t, rp[q]), __builtin_bit_cast(ushort2_t, rp[q]), sr2u,
                                      false);
        sr1 = __builtin_amdgcn_udot2(__builtin_bit_cast(ushort2_t, rp[q]), __builtin_bit_cast(ushort2_t, kOnes), sr1,
                                     false);
    }
    // every quad holds the whole range: the sums are wave-uniform (scalar registers from here on)
    sr2u = (uint32_t)__builtin_amdgcn_readfirstlane((int)quad_sum(sr2u));
    sr1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)quad_sum(sr1));
    const int sr2 = (int)sr2u; // Σr² ≤ 64·255²
    // the greatest entry y (vmax) over the block's splits and lane halves, and the chunk(s) holding it
    unsigned long long bestk = kKeyNone;
    uint32_t bx = 0, bs1 = 0, bs2 = 0; // X_t, ΣD4, ΣD4² of bestk's candidate (fit_rstat)
    float vmax = -__builtin_inff();
    bool exact = false, hit = false;
    int64_t target = -1;
    auto set_target = [&]() {
        const bool sentinel = vmax == __builtin_inff();
        exact = sentinel || vmax > (float)(sa16 - kExactLimit);
        target = exact && !sentinel ? sa16 - (int64_t)vmax : -1;
        hit = a.hitH >= 0 && (sentinel || (target >= 0 && target <= a.hitH));
    };
    // re-evaluate chunk `tile0` (4 tiles from there, none at or past tend; SORTED: the tiles in tmask) on the rows
    // of lane half h, keeping the least selection key
    auto eval_chunk = [&](uint32_t tile0, uint32_t h, uint32_t tmask, uint32_t tend) {
        const int row = (i & 3) + 8 * (i >> 2) + 4 * (int)h;
        if (!exact) {
            // fp32 fallback regime: every candidate has S16 ≥ 2^24; any valid domain of the
            // bucket routes the range to fallback_grid through the fit's listing
            const int p = a.tile_pos[tile0 * 32 + row];
            const unsigned long long mask = __ballot(p >= 0 && g == 0);
            if (mask) {
                const int pf = __builtin_amdgcn_readlane(p, __ffsll((long long)mask) - 1);
                bestk = min(bestk, key_miss((uint64_t)kExactLimit, (uint32_t)pf, 0));
            }
            return;
        }
        for (uint32_t tile = tile0; tile < min(tile0 + (uint32_t)kTilesPerStage, tend); ++tile) {
            if (!((tmask >> (tile - tile0)) & 1u))
                continue;
            // the row's pool position (for the key) and its D4 from the tile-order copy are
            // independent loads; ΣD4² is summed here rather than loaded through the position.
            // (Loading the chunk's four tiles up front saved 1 µs at C2 but took 24 more VGPRs:
            // 4 instead of 6 waves per SIMD cost the C4 quadtree's 65k-range level 21 µs.)
            const int p = a.tile_pos[tile * 32 + row];
            const uint4* dp = reinterpret_cast<const uint4*>(a.tpool + ((size_t)tile * 32 + row) * 32 + g * (PG / 2));
            const uint4 d0 = dp[0], d1 = dp[1];
            const uint32_t dv[PG / 2] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
            uint32_t sd2 = 0, sd1 = 0;
#pragma unroll
            for (int q = 0; q < PG / 2; ++q) {
                sd2 = __builtin_amdgcn_udot2(__builtin_bit_cast(ushort2_t, dv[q]), __builtin_bit_cast(ushort2_t, dv[q]),
                                             sd2, false);
                sd1 = __builtin_amdgcn_udot2(__builtin_bit_cast(ushort2_t, dv[q]), __builtin_bit_cast(ushort2_t, kOnes),
                                             sd1, false);
            }
            sd2 = quad_sum(sd2);
            sd1 = quad_sum(sd1);
            const int nsd2 = -(int)sd2; // ΣD4² ≤ 64·1020² < 2^31
            unsigned long long tk = kKeyNone;
            uint32_t tx = 0, ts1 = 0, ts2 = 0;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                uint32_t X = 0;
#pragma unroll
                for (int q = 0; q < PG / 2; ++q) {
                    // pair q of orbit q/2 for transform t (see the lane map above)
                    // t odd: the rotated pairs, rebuilt per transform (a t = 1 copy held across
                    // the loop would take 8 more VGPRs)
                    const int qs = q ^ (t >> 1);
                    const uint32_t dq = (t & 1) ? __builtin_amdgcn_alignbit(dv[qs ^ 1], dv[qs], 16) : dv[qs];
                    X = __builtin_amdgcn_udot2(__builtin_bit_cast(ushort2_t, rp[q]), __builtin_bit_cast(ushort2_t, dq),
                                               X, false);
                }
                X = quad_sum(X);
                // S16 = 16Σr² − 8X + ΣD4² ≤ 64·1020² < 2^31: exact in int32
                const int64_t s16 = p >= 0 ? (int64_t)(16 * sr2 - 8 * (int32_t)X - nsd2) : 0;
                const bool ok = p >= 0 && g == 0 && (hit ? (s16 <= a.hitH) : (s16 == target));
                const uint32_t tr = flip ? 4u + ((4u - (uint32_t)t) & 3u) : (uint32_t)t; // the reference's transform
                if constexpr (SORTED) {
                    // lane-local least key; one wave reduction per range at the end
                    const unsigned long long k =
                        ok ? (hit ? key_hit((uint32_t)p, tr) : key_miss((uint64_t)target, (uint32_t)p, TK - 1 - tr))
                           : kKeyNone;
                    if (k < tk) {
                        tk = k;
                        tx = X;
                    }
                } else {
                    const unsigned long long mask = __ballot(ok);
                    if (mask) {
                        const int first = __ffsll((long long)mask) - 1;
                        const int pf = __builtin_amdgcn_readlane(p, first);
                        const unsigned long long k = hit ? key_hit((uint32_t)pf, tr)
                                                         : key_miss((uint64_t)target, (uint32_t)pf, TK - 1 - tr);
                        const uint32_t xf = (uint32_t)__builtin_amdgcn_readlane((int)X, first);
                        const uint32_t s1f = (uint32_t)__builtin_amdgcn_readlane((int)sd1, first);
                        const uint32_t s2f = (uint32_t)__builtin_amdgcn_readlane((int)sd2, first);
                        if (k < tk) {
                            tk = k;
                            tx = xf;
                            ts1 = s1f;
                            ts2 = s2f;
                        }
                    }
                }
            }
            if constexpr (SORTED) {
                ts1 = sd1;
                ts2 = sd2;
            }
            if (tk != kKeyNone) {
                if (tk < bestk) {
                    bestk = tk;
                    bx = tx;
                    bs1 = ts1;
                    bs2 = ts2;
                }
                if constexpr (!SORTED)
                    break;
            }
        }
    };
    if constexpr (!SORTED) {
        // the search merged its splits itself (search_dft, DftArgs::slotbest): the slot's greatest y, the
        // earliest chunk attaining it, its tiles to evaluate and which lane halves attain it — one load
        if (sb == 0ull)
            return res; // no work item reached the slot: no eligible domain
        vmax = funmap((uint32_t)(sb >> 32));
        if (!(vmax > -1.0e29f))
            return res; // only padding rows: no eligible domain, best_key stays "none"
        set_target();
        const uint32_t tile0 = kSlotBestTileMax - ((uint32_t)sb >> 6), tm = ((uint32_t)sb >> 2) & 0xfu;
        const uint32_t hm = (uint32_t)sb & 3u;
        for (uint32_t h = 0; h < 2; ++h)
            if ((hm >> h) & 1u)
                eval_chunk(tile0, h, tm, a.ntiles);
    } else {
        // the search kept each lane's maximum over its group's window and the chunks attaining it (search_dft
        // CHUNKED): two loads per slot.  A block without a group (a bucket without domains) was
        // never searched and its record is some earlier run's: not read
        if (gw.x == 0xffffffffu)
            return res;
        const float y0 = __uint_as_float(rec0.x), y1 = __uint_as_float(rec1.x);
        vmax = __builtin_fmaxf(y0, y1);
        if (!(vmax > -1.0e29f))
            return res; // an empty window, or only padding rows: no eligible domain, best_key stays "none"
        set_target();
        for (uint32_t h = 0; h < 2; ++h) {
            const uint4 rc = h ? rec1 : rec0;
            if (__uint_as_float(rc.x) != vmax)
                continue;
            if (rc.y <= kTpRecList) {
                // every chunk attaining the maximum is listed; a word carries the chunk's tile mask in bits 28..31
                eval_chunk(rc.z & 0x0fffffffu, h, rc.z >> 28, a.ntiles);
                if (rc.y > 1u)
                    eval_chunk(rc.w & 0x0fffffffu, h, rc.w >> 28, a.ntiles);
            } else {
                // more chunks attain it than the record lists: every chunk of the group's window, whole.  A chunk
                // that does not hold the maximum adds nothing (only rows with S16 = target, or hits, are kept), so
                // this is exact; the window ends at its t1, not the chunk's fourth tile: past it lie tiles the
                // bound excluded, or another bucket's
                const uint4 wk = a.work[gw.x];
                for (uint32_t t = wk.z; t < wk.w; t += (uint32_t)kTilesPerStage)
                    eval_chunk(t, h, 0xfu, wk.w);
            }
        }
    }
    const unsigned long long mine = bestk;
    if constexpr (SORTED) {
        const unsigned long long have = ONE ? __ballot(mine != kKeyNone) : ~0ull;
        if (ONE && (have & (have - 1)) == 0ull) {
            // at most one lane holds a key: it is the least (none: every lane's bestk is "none" already)
            if (have) {
                const int src = __ffsll((long long)have) - 1;
                bestk = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(mine >> 32), src) << 32) |
                        (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)mine, src);
                bx = (uint32_t)__builtin_amdgcn_readlane((int)bx, src);
                bs1 = (uint32_t)__builtin_amdgcn_readlane((int)bs1, src);
                bs2 = (uint32_t)__builtin_amdgcn_readlane((int)bs2, src);
            }
        } else {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long ok2 = ((unsigned long long)lane_xor((uint32_t)(bestk >> 32), lane, o) << 32) |
                                               lane_xor((uint32_t)bestk, lane, o);
                bestk = ok2 < bestk ? ok2 : bestk;
            }
            // the winner's sums: from the lane that evaluated it (keys are unique per (domain, transform)),
            // broadcast through a ballot
            const unsigned long long own = __ballot(mine == bestk && bestk != kKeyNone);
            if (own) {
                const int src = __ffsll((long long)own) - 1;
                bx = (uint32_t)__builtin_amdgcn_readlane((int)bx, src);
                bs1 = (uint32_t)__builtin_amdgcn_readlane((int)bs1, src);
                bs2 = (uint32_t)__builtin_amdgcn_readlane((int)bs2, src);
            }
        }
    }
    res.bestk = bestk;
    res.bx = bx;
    res.bs1 = bs1;
    res.bs2 = bs2;
    res.sr1 = sr1;
    res.sr2 = (uint32_t)sr2;
    return res;
}

// the same with the slot's loads issued here (one slot per wave)
template <bool SORTED>
__device__ inline DftResolved resolve_dft_eval(const MfmaResolveArgs& a, uint32_t slot, int ri, int lane, bool flip)
{
    return resolve_dft_eval<SORTED>(a, slot, ri, lane, flip, dft_slot_loads<SORTED>(a, slot, lane));
}

// range r's record from its resolved winner w (every lane holds the same after resolve_dft_eval); rg: the
// range's item, loaded by the caller at the start of the resolve
__device__ inline void resolve_dft_record(const MfmaResolveArgs& a, uint32_t r, const DftResolved& w, int lane,
                                          const frac_grid_item& rg)
{
    if (a.fused_fit) { // the range's record right here: one launch less per run (C2: 5 µs of a 43 µs frame)
        // the whole wave: the record and the tuple leave as whole stores (fit_rstat_range_wave)
        if (lane == 0)
            a.best_key[r] = w.bestk;
        fit_rstat_range_wave<8>(a.fit, r, w.bestk, make_uint4(w.bx, w.bs1 | (w.sr1 << 16), w.bs2, w.sr2), rg, lane);
        return;
    }
    if (lane == 0) {
        a.best_key[r] = w.bestk;
        if (a.rstat && w.bestk != kKeyNone)
            a.rstat[r] = make_uint4(w.bx, w.bs1 | (w.sr1 << 16), w.bs2, w.sr2);
    }
}

// the slot's range record: its least key (with T = 8's flipped copy, the lesser of the two) and the
// winner's sums for fit_rstat (every lane holds the same after resolve_dft_eval)
template <bool SORTED>
__device__ inline void resolve_dft_slot(const MfmaResolveArgs& a, uint32_t slot, int lane)
{
    const int ri = a.slot_range[slot];
    if (ri < 0)
        return;
    const frac_grid_item rg = a.fused_fit ? a.fit.ranges[ri] : frac_grid_item{};
    DftResolved w = resolve_dft_eval<SORTED>(a, slot, ri, lane, false);
    if (!SORTED && a.flip_slots) {
        const DftResolved f =
            resolve_dft_eval<SORTED>(a, slot + a.flip_slots, a.slot_range[slot + a.flip_slots], lane, true);
        if (f.bestk < w.bestk)
            w = f;
    }
    resolve_dft_record(a, (uint32_t)ri, w, lane, rg);
}

// T = 8 with the flipped copies (MfmaResolveArgs::paired): a two-wave workgroup per slot, wave 0
// resolving the slot and wave 1 its flipped copy at the same time (the one-wave form ran the two
// one after the other); wave 0 keeps the lesser key and writes the record
__device__ inline void resolve_dft_pair(const MfmaResolveArgs& a, uint32_t slot, uint32_t wave, int lane)
{
    __shared__ unsigned long long fkey;
    __shared__ uint32_t fsums[5];
    const int ri = a.slot_range[slot]; // the same for both waves: the barrier below is reached by both or neither
    if (ri < 0)
        return;
    const frac_grid_item rg = (a.fused_fit && wave == 0) ? a.fit.ranges[ri] : frac_grid_item{};
    const uint32_t ws = slot + wave * a.flip_slots;
    const DftResolved w = resolve_dft_eval<false>(a, ws, a.slot_range[ws], lane, wave == 1);
    if (wave == 1 && lane == 0) {
        fkey = w.bestk;
        fsums[0] = w.bx;
        fsums[1] = w.bs1;
        fsums[2] = w.bs2;
        fsums[3] = w.sr1;
        fsums[4] = w.sr2;
    }
    __syncthreads();
    if (wave == 0) {
        DftResolved f;
        f.bestk = fkey;
        f.bx = fsums[0];
        f.bs1 = fsums[1];
        f.bs2 = fsums[2];
        f.sr1 = fsums[3];
        f.sr2 = fsums[4];
        resolve_dft_record(a, (uint32_t)ri, f.bestk < w.bestk ? f : w, lane, rg);
    }
}

// One wave per slot, in slot order (the 32 ranges of a block read the same entry lines, or on the sorted route
// neighbouring records, back to back); launched as one- or four-wave workgroups. A grid of fewer, longer-lived waves striding over the slots measured slower (452 vs
// 372 µs at C3 in the SEA tiled form).
//
// BY_RANGE (the sorted route writing a tuple sink in host memory, launch_tp): one wave per range in range order
// instead (slot = range_slot[r], padding slots never visited, grid ⌈nr / 4⌉), so neighbouring waves write
// neighbouring tuples — the four waves of a workgroup 128 contiguous bytes of the sink — as the exhaustive route's
// slot walk does.  In (bucket, ΣR) order no two tuples written near each other in time share a host line, which cost
// the C3 finish 0.12 ms across PCIe.  Range order still has a price without the entry rows it once
// scattered: a block's 32 slots no longer read their records, constants and orbit copies side by side, 0.035 ms of
// the C3 finish with no sink or a device sink (§7.7), so a run without a host sink keeps the slot order.
// kTpRangeOrder = false keeps the slot order everywhere.  Without a hit threshold both walks run in groups
// (resolve_dft_groups below: ranges r0 … r0 + G − 1 write one contiguous block of the sink), 0.230 → 0.203 ms of the
// C3 finish with a pinned sink and 0.197 → 0.176 with none (§7.14).
constexpr bool kTpRangeOrder = true;

// range r of the sorted route, range order: its slot from the inverse map (tp_build writes one per range)
__device__ inline void resolve_dft_range(const MfmaResolveArgs& a, uint32_t r, int lane)
{
    const uint32_t slot = a.range_slot[r];
    const frac_grid_item rg = a.fused_fit ? a.fit.ranges[r] : frac_grid_item{};
    if (slot >= a.nslots)
        return;
    resolve_dft_record(a, r, resolve_dft_eval<true>(a, slot, (int)r, lane, false), lane, rg);
}

template <bool SORTED = false, bool BY_RANGE = false>
__global__ void __launch_bounds__(256, 8) resolve_dft(MfmaResolveArgs a)
{
    static_assert(SORTED || !BY_RANGE, "the range-order walk is the sorted route's");
    apply_plan(a);
    if constexpr (!SORTED) {
        if (a.paired) { // two-wave workgroups: the slot and its flipped copy at once
            const uint32_t slot = blockIdx.x;
            if (slot < a.nslots)
                resolve_dft_pair(a, slot, __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), threadIdx.x & 63);
            return;
        }
    }
    // the slot is wave-uniform: readfirstlane lets its loads go through the scalar unit
    const uint32_t slot = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if constexpr (BY_RANGE) {
        if (slot < a.nr) // the wave's index is its range
            resolve_dft_range(a, slot, threadIdx.x & 63);
    } else {
        if (slot < a.nslots)
            resolve_dft_slot<SORTED>(a, slot, threadIdx.x & 63);
    }
}

// ---------------------------------------------------------------------------
// resolve_dft_groups: the sorted route's resolve in groups of G consecutive items (ranges with a host sink, slots
// otherwise, as kTpRangeOrder chooses), launched from launch_tp alone.  Only a range's tile evaluation fills a wave
// (16 rows × 4 pixel quarters); its fit — fp64, two divisions — and its stores are per-range work that
// resolve_dft<true> repeats in all 64 lanes.  Here a workgroup works in two phases:
//   1  its waves evaluate the items (resolve_dft_eval<true>, unchanged arithmetic) and lane 0 leaves each item's
//      {key, X, ΣD4 | Σr << 16, ΣD4², Σr², range, state} in LDS; a padding slot, an item past the end, a block
//      without a group, an empty window all deposit and fall through, so every wave reaches the one barrier;
//   2  lane k of wave 0 fits item k (fit_rstat_range_regs) and stores best_key and aux as one 8-byte store each.
//      Range order: the group's records and tuples are the contiguous blocks [64·r0, 64·(r0 + n)) of the records
//      and [32·r0, 32·(r0 + n)) of the sink; they are staged in LDS and leave as whole stores, 16 bytes a lane for
//      the records and 8 for the tuples (the sink is 8-byte aligned and no more), lane l taking piece 64·j + l.
//      A piece of an item whose record is not written here (fp32 regime, past the end) is not stored: no byte
//      outside the block, none of a listed range's.  Slot order: each lane stores its own record and tuple.
// The workgroup's shape was measured (C3, finish ms with a pinned sink / with none; resolve_dft<true> 0.230 / 0.197;
// DESIGN §7.14): one item per wave and 16 waves 0.217 / 0.183, 8 waves 0.213 / 0.186, 4 waves 0.203 / 0.176 — the
// tail of wave 0 holds a workgroup's wave slots, the fewer the better; 4 waves of 8 items each, the next item's
// slot-level loads issued before the current one is evaluated, 0.250 / 0.202: the second set of loads does not fit
// 64 registers (64 bytes of scratch).  Every shape: 64 VGPRs; scratch 0 but for that one.
// ---------------------------------------------------------------------------
constexpr uint32_t kTpGrpWaves = 4u;   // waves per workgroup
constexpr uint32_t kTpGrpPerWave = 1u; // items per wave
constexpr uint32_t kTpGrpItems = kTpGrpWaves * kTpGrpPerWave; // G
constexpr bool kTpGrpOne = true; // the winner read from its lane when one lane holds a key (resolve_dft_eval ONE)
// runs with a hit threshold take the grouped form too (launch_tp); false: they keep resolve_dft<true>, whose waves
// each end with their own first-hit walk instead of waiting at a barrier for the group's longest
constexpr bool kTpGrpHits = false;
static_assert(kTpGrpItems <= 64 && kTpGrpPerWave <= 64, "phase 2 is one wave, a lane per item");

// workgroups for n items, the items of workgroup b, and the 16- or 8-byte pieces of a group's staged block
__host__ __device__ constexpr uint32_t tp_grp_grid(uint32_t n)
{
    return n / kTpGrpItems + (n % kTpGrpItems != 0u ? 1u : 0u);
}
__host__ __device__ constexpr uint32_t tp_grp_count(uint32_t n, uint32_t b)
{
    return b >= tp_grp_grid(n) ? 0u : (n - b * kTpGrpItems < kTpGrpItems ? n - b * kTpGrpItems : kTpGrpItems);
}
constexpr uint32_t kTpGrpPieces = kTpGrpItems * 4u; // a record is four 16-byte pieces, a tuple four 8-byte ones
constexpr uint32_t kTpGrpPasses = (kTpGrpPieces + 63u) / 64u;
static_assert(tp_grp_grid(0u) == 0u && tp_grp_grid(1u) == 1u && tp_grp_grid(kTpGrpItems) == 1u &&
                  tp_grp_grid(kTpGrpItems + 1u) == 2u &&
                  tp_grp_grid(0xffffffffu) == (uint32_t)((0xffffffffull + kTpGrpItems - 1u) / kTpGrpItems),
              "grid size");
static_assert(tp_grp_count(0u, 0u) == 0u && tp_grp_count(1u, 0u) == 1u && tp_grp_count(kTpGrpItems, 0u) == kTpGrpItems &&
                  tp_grp_count(kTpGrpItems, 1u) == 0u && tp_grp_count(kTpGrpItems + 1u, 1u) == 1u &&
                  tp_grp_count(0xffffffffu, tp_grp_grid(0xffffffffu) - 1u) == (0xffffffffu - 1u) % kTpGrpItems + 1u,
              "items of a group");
static_assert((uint64_t)(tp_grp_grid(0xffffffffu) - 1u) * kTpGrpItems +
                      tp_grp_count(0xffffffffu, tp_grp_grid(0xffffffffu) - 1u) == 0xffffffffull,
              "the last group's items end at n: no index of an item wraps");
static_assert(kTpGrpPasses * 64u >= kTpGrpPieces && (kTpGrpPasses - 1u) * 64u < kTpGrpPieces &&
                  sizeof(frac_encode_item) == 64 && sizeof(frac_tuple) == 32 && sizeof(RangeAux) == 8,
              "staged pieces");

template <bool BY_RANGE>
__global__ void __launch_bounds__(kTpGrpWaves * 64, 8) resolve_dft_groups(MfmaResolveArgs a)
{
    constexpr uint32_t G = kTpGrpItems;
    __shared__ uint4 dep[G][2];
    __shared__ uint4 srec[BY_RANGE ? kTpGrpPieces : 1];
    __shared__ uint2 stup[BY_RANGE ? kTpGrpPieces : 1];
    apply_plan(a);
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t base = blockIdx.x * G, cnt = tp_grp_count(BY_RANGE ? a.nr : a.nslots, blockIdx.x);
    // ---- phase 1: this wave's items k = j·waves + wave; lane j first loads item j's slot and range
    uint32_t vslot = 0u;
    int vri = -1;
    if ((uint32_t)lane < kTpGrpPerWave) {
        const uint32_t k = (uint32_t)lane * kTpGrpWaves + wave;
        if (k < cnt) {
            if constexpr (BY_RANGE) {
                vslot = a.range_slot[base + k];
                vri = vslot < a.nslots ? (int)(base + k) : -1;
            } else {
                vslot = base + k;
                vri = a.slot_range[vslot];
            }
        }
    }
    uint32_t slot = (uint32_t)__builtin_amdgcn_readlane((int)vslot, 0);
    int ri = __builtin_amdgcn_readlane(vri, 0);
    DftSlotLoads ld;
    if (ri >= 0)
        ld = dft_slot_loads<true>(a, slot, lane);
#pragma unroll 1
    for (uint32_t j = 0; j < kTpGrpPerWave; ++j) {
        // the next item's slot-level loads go out before this one is evaluated
        uint32_t nslot = 0u;
        int nri = -1;
        DftSlotLoads nld;
        if (j + 1u < kTpGrpPerWave) {
            nslot = (uint32_t)__builtin_amdgcn_readlane((int)vslot, (int)(j + 1u));
            nri = __builtin_amdgcn_readlane(vri, (int)(j + 1u));
            if (nri >= 0)
                nld = dft_slot_loads<true>(a, nslot, lane);
        }
        // (ri < 0 — a padding slot, an item past the end: the default, nothing read)
        const DftResolved w = resolve_dft_eval<true, kTpGrpOne>(a, slot, ri, lane, false, ld);
        if (lane == 0) {
            const uint32_t k = j * kTpGrpWaves + wave;
            dep[k][0] = make_uint4((uint32_t)w.bestk, (uint32_t)(w.bestk >> 32), w.bx, w.bs1 | (w.sr1 << 16));
            dep[k][1] = make_uint4(w.bs2, w.sr2, (uint32_t)ri, ri >= 0 ? 1u : 0u);
        }
        slot = nslot;
        ri = nri;
        ld = nld;
    }
    __syncthreads();
    // ---- phase 2: wave 0, lane k fits item k
    if (wave != 0u)
        return;
    // The fit's arguments are read here from the kernel-argument segment (the one by-value argument lies at its
    // start): loaded at entry with the rest they would be held in scalar registers across the evaluation, which
    // has none to spare, and spilled to vector lanes.
    const MfmaResolveArgs& ka =
        *reinterpret_cast<const MfmaResolveArgs*>((const void*)__builtin_amdgcn_kernarg_segment_ptr());
    const FitArgs& fit = ka.fit;
    FitRegs f;
    f.kind = kFitSkip;
    uint32_t r = 0u;
    if ((uint32_t)lane < G) {
        const uint4 d0 = dep[lane][0], d1 = dep[lane][1];
        if (d1.w) {
            r = d1.z;
            const unsigned long long key = ((unsigned long long)d0.y << 32) | d0.x;
            f = fit_rstat_range_regs<8>(fit, r, key, make_uint4(d0.z, d0.w, d1.x, d1.y), fit.ranges[r]);
            reinterpret_cast<uint2*>(ka.best_key)[r] = make_uint2(d0.x, d0.y);
            reinterpret_cast<uint2*>(fit.aux)[r] = f.aux;
        }
    }
    if constexpr (BY_RANGE) {
        if (f.kind == kFitRecord) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                srec[lane * 4 + q] = f.q[q];
                stup[lane * 4 + q] = fit_tuple_piece(f, q);
            }
        }
        const unsigned long long written = __ballot(f.kind == kFitRecord); // bit k: item k's record leaves here
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");            // (one wave: its LDS writes are done)
        __builtin_amdgcn_wave_barrier();
        uint4* out4 = reinterpret_cast<uint4*>(fit.out + base);
        uint2* tup2 = reinterpret_cast<uint2*>(fit.tuples + base);
#pragma unroll
        for (uint32_t j = 0; j < kTpGrpPasses; ++j) {
            const uint32_t u = 64u * j + (uint32_t)lane; // piece u of the block belongs to item u / 4
            if (u < kTpGrpPieces && ((written >> (u >> 2)) & 1ull)) {
                out4[u] = srec[u];
                tup2[u] = stup[u];
            }
        }
    } else if (f.kind == kFitRecord) {
        uint4* out4 = reinterpret_cast<uint4*>(fit.out + r);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            out4[q] = f.q[q];
        if (fit.tuples) {
            uint2* tup2 = reinterpret_cast<uint2*>(fit.tuples + r);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                tup2[q] = fit_tuple_piece(f, q);
        }
    }
}

} // namespace fracenc
