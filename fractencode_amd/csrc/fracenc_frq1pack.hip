// fracenc_frq1pack.hip — FRQ1 streams laid out, quantized and bit-packed on the device.  Included by
// fracenc_api.hip after fracenc_qtrate.hip (whose tree geometry and keys it reads) and fracenc_stream.hip
// (whose dkey and quantize it reuses, so the arithmetic is the one already pinned to the host packer).
//
// One packer over the level-major full-tree index (level k's N_k = 4^k·N_0 nodes from off[k], FRQ1's canonical
// order) with three front ends that say, per node, whether a partition reaches it and whether it is a leaf there:
//   frq1_state_rate   frac_quadtree_rate_stream: from the rate state's split keys and the split distance,
//                     exactly as qtr_leaf_flags does; a node's record is its own slot of the state
//   frq1_slots +      frac_encode_quadtree_stream: the search's leaves (d_qt_leaves32) scattered into their
//   frq1_state_slots  full-tree slots, the inverse of qtr_ranges (the level-0 item, then one quadrant digit per
//                     level); a node is reached when no ancestor is a leaf, a leaf when it has one itself
//   qrd_state         frac_quadtree_rd_stream (fracenc_qtrd.hip): from the rate state's integer distortions and a
//                     multiplier, the bottom-up pruning's partition; a node's record is its own slot of the state
// All write one 64-bit flag per node, reached in the high word and leaf in the low one, and reduce the leaves'
// contrast and brightness to four order-preserving keys (a wave reduction, one atomic per wave and field).
// Then, for either route:
//   DeviceScan        one exclusive sum over the flags: the high word is the rank among reached nodes (the bit
//                     position in the level's bitmap), the low word the rank among leaves (the record position
//                     in the level's section); N_k and M_k are the differences at off[k]
//   frq1_table        one wave: the section table (bitmap and record offsets per level, the body's size, the leaf
//                     count) into device memory and, with the four keys, into a mapped host result
//   frq1_pack         per reached node: a split ORs its bit into the level's bitmap, a leaf quantizes its record
//                     and ORs its two or three dwords into the level's section (atomicOr into a zeroed body)
// Grids and buffers are sized by what the host knows without a device count: the tree's node counts and
// frq1_body_bound, every section at its level's full node count.  The host synchronises once for the result and
// once more for a copy of exactly the body's bytes; no leaf goes to the host on either route.
namespace {

struct Frq1Geom {
    uint32_t levels, lg0, cols0; // lg0 = log2 max_size, cols0 = level 0's columns
    uint32_t nodes[4], off[5];
    uint32_t nd[4], ib[4], rb[4]; // per level: domains, index bits, record bits
    uint32_t tb, cbits, bbits;
    uint32_t cap_words;           // frq1_body_bound: no kernel writes a body word at or past it
};

// the level of node i of the level-major index
__device__ inline uint32_t frq1_level_of(const Frq1Geom& g, uint32_t i)
{
    uint32_t k = 0;
    while (k + 1 < g.levels && i >= g.off[k + 1])
        ++k;
    return k;
}

// The leaves' bounds as four maxima (of ~key for a minimum), so one zeroed block starts them.  Every lane of the
// wave calls it; a wave without a leaf writes nothing.
__device__ inline void frq1_bounds(bool leaf, double cv, double bv, unsigned long long* __restrict__ mm)
{
    unsigned long long v[4] = {0ull, 0ull, 0ull, 0ull};
    if (leaf) {
        const unsigned long long ck = dkey(cv), bk = dkey(bv);
        v[0] = ~ck, v[1] = ck, v[2] = ~bk, v[3] = bk;
    }
    const bool any = __ballot(leaf) != 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int f = 0; f < 4; ++f)
            v[f] = max(v[f], (unsigned long long)__shfl_xor(v[f], o, 64));
    if ((threadIdx.x & 63u) == 0 && any)
#pragma unroll
        for (int f = 0; f < 4; ++f)
            atomicMax(&mm[f], v[f]);
}

// the rate route: reached and leaf from the split keys (qtr_leaf_flags' rule); flag[total] = 0
__global__ void __launch_bounds__(256) frq1_state_rate(Frq1Geom g, const double* __restrict__ e, double t,
                                                       const frac_qt_leaf* __restrict__ nodes,
                                                       unsigned long long* __restrict__ flag,
                                                       unsigned long long* __restrict__ mm)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, total = g.off[g.levels];
    bool reached = false, leaf = false;
    double cv = 0.0, bv = 0.0;
    if (i < total) {
        const uint32_t k = frq1_level_of(g, i), j = i - g.off[k];
        reached = k == 0 || e[g.off[k - 1] + (j >> 2)] > t;
        leaf = reached && !(k + 1 < g.levels && e[i] > t);
        if (leaf) {
            cv = nodes[i].contrast;
            bv = nodes[i].brightness;
        }
    }
    if (i <= total)
        flag[i] = (unsigned long long)(reached ? 1u : 0u) << 32 | (leaf ? 1u : 0u);
    frq1_bounds(leaf, cv, bv, mm);
}

// the search route: leaf p into the slot of its node (slot[] = all-ones beforehand)
__global__ void __launch_bounds__(256) frq1_slots(Frq1Geom g, const frac_qt_leaf* __restrict__ leaves, uint32_t n,
                                                  uint32_t* __restrict__ slot)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n)
        return;
    const uint32_t x = leaves[p].x, y = leaves[p].y, lg = leaves[p].code >> 28;
    if (lg > g.lg0 || g.lg0 - lg >= g.levels)
        return;
    const uint32_t k = g.lg0 - lg, cx = x >> g.lg0, cy = y >> g.lg0;
    if (cx >= g.cols0)
        return;
    uint32_t j = cy * g.cols0 + cx;
    if (j >= g.nodes[0])
        return;
    for (uint32_t d = 1; d <= k; ++d) {
        const uint32_t s = g.lg0 - d;
        j = 4 * j + (((x >> s) & 1u) | ((y >> s) & 1u) << 1);
    }
    slot[g.off[k] + j] = p;
}

__global__ void __launch_bounds__(256) frq1_state_slots(Frq1Geom g, const uint32_t* __restrict__ slot,
                                                        const frac_qt_leaf* __restrict__ leaves,
                                                        unsigned long long* __restrict__ flag,
                                                        unsigned long long* __restrict__ mm)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, total = g.off[g.levels];
    bool reached = false, leaf = false;
    double cv = 0.0, bv = 0.0;
    if (i < total) {
        const uint32_t k = frq1_level_of(g, i), j = i - g.off[k];
        reached = true;
        for (uint32_t a = 0; a < k; ++a)
            reached = reached && slot[g.off[a] + (j >> (2 * (k - a)))] == ~0u;
        const uint32_t p = slot[i];
        leaf = reached && p != ~0u;
        if (leaf) {
            cv = leaves[p].contrast;
            bv = leaves[p].brightness;
        }
    }
    if (i <= total)
        flag[i] = (unsigned long long)(reached ? 1u : 0u) << 32 | (leaf ? 1u : 0u);
    frq1_bounds(leaf, cv, bv, mm);
}

// the section table (Frq1Table, fracenc_ctx.h) from the ranks at the level boundaries: one thread, the four
// levels unrolled so that the table stays in registers
__global__ void __launch_bounds__(64) frq1_table(Frq1Geom g, const unsigned long long* __restrict__ rank,
                                                 const unsigned long long* __restrict__ mm,
                                                 Frq1Table* __restrict__ tab, Frq1Result* __restrict__ res)
{
    if (blockIdx.x || threadIdx.x)
        return;
    Frq1Table t{};
    uint32_t w = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        if (k >= g.levels)
            break;
        const unsigned long long a = rank[g.off[k]], b = rank[g.off[k + 1]];
        const uint32_t N = (uint32_t)(b >> 32) - (uint32_t)(a >> 32), M = (uint32_t)b - (uint32_t)a;
        t.reach0[k] = (uint32_t)(a >> 32);
        t.leaf0[k] = (uint32_t)a;
        t.bm_word[k] = w;
        if (k + 1 < g.levels)
            w += (N + 31) / 32;
        t.rec_word[k] = w;
        w += (uint32_t)(((unsigned long long)M * g.rb[k] + 31) / 32);
    }
    t.words = w;
    t.leaves = (uint32_t)rank[g.off[g.levels]];
    *tab = t;
    res->t = t;
    for (int f = 0; f < 4; ++f)
        res->mm[f] = mm[f];
}

// per reached node its bit or its record into the zeroed body; slot = nullptr: node i's record is rec[i]
__global__ void __launch_bounds__(256) frq1_pack(Frq1Geom g, const unsigned long long* __restrict__ flag,
                                                 const unsigned long long* __restrict__ rank,
                                                 const Frq1Table* __restrict__ tab,
                                                 const frac_qt_leaf* __restrict__ rec, const uint32_t* __restrict__ slot,
                                                 const unsigned long long* __restrict__ mm, uint32_t* __restrict__ body)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.off[g.levels])
        return;
    const unsigned long long f = flag[i];
    if (!(f >> 32))
        return;
    const uint32_t k = frq1_level_of(g, i);
    const unsigned long long r = rank[i];
    if (!(uint32_t)f) { // reached and no leaf: a split
        const uint32_t q = (uint32_t)(r >> 32) - tab->reach0[k], w = tab->bm_word[k] + (q >> 5);
        if (k + 1 < g.levels && w < g.cap_words)
            atomicOr(&body[w], 1u << (q & 31u));
        return;
    }
    const frac_qt_leaf e = rec[slot ? slot[i] : i];
    const uint32_t d = e.code & FRAC_QT_NO_DOMAIN, ib = g.ib[k], width = g.rb[k];
    unsigned long long v = d == FRAC_QT_NO_DOMAIN ? g.nd[k] : d;
    v |= (unsigned long long)((e.code >> 24) & 15u) << ib;
    v |= quantize(e.contrast, dkey_inv(~mm[0]), dkey_inv(mm[1]), g.cbits) << (ib + g.tb);
    v |= quantize(e.brightness, dkey_inv(~mm[2]), dkey_inv(mm[3]), g.bbits) << (ib + g.tb + g.cbits);
    const unsigned long long bit = (unsigned long long)((uint32_t)r - tab->leaf0[k]) * width;
    const uint32_t sh = (uint32_t)(bit & 31u);
    const unsigned long long w = tab->rec_word[k] + (bit >> 5);
    if (w + (sh + width + 31) / 32 > g.cap_words)
        return;
    atomicOr(&body[w], (uint32_t)(v << sh));
    if (sh + width > 32)
        atomicOr(&body[w + 1], (uint32_t)(v >> (32 - sh)));
    if (sh + width > 64)
        atomicOr(&body[w + 2], (uint32_t)(v >> (64 - sh)));
}

// a bound of the body's dwords the host knows: every level's bitmap and record section at its full node count
uint64_t frq1_body_bound(const Frq1Geom& g)
{
    uint64_t w = 0;
    for (uint32_t k = 0; k < g.levels; ++k)
        w += (k + 1 < g.levels ? ((uint64_t)g.nodes[k] + 31) / 32 : 0) + ((uint64_t)g.nodes[k] * g.rb[k] + 31) / 32;
    return w;
}

// what the packer needs of a frame's tree and a stream's widths (frq1_levels has accepted the sizes)
Frq1Geom frq1_geom(uint32_t W, uint32_t H, uint32_t max_size, uint32_t min_size, uint32_t T, uint32_t cbits,
                   uint32_t bbits)
{
    Frq1Geom g{};
    uint32_t side[4];
    g.levels = frq1_levels(max_size, min_size, side);
    g.lg0 = frq1_bitlen(max_size) - 1;
    const uint64_t n0 = frac_uniform_grid(W, H, max_size, max_size, nullptr, 0);
    g.cols0 = n0 ? (W - max_size) / max_size + 1 : 1u;
    g.tb = std::max(1u, frq1_bitlen(T - 1));
    g.cbits = cbits, g.bbits = bbits;
    for (uint32_t k = 0; k < g.levels; ++k) {
        g.nodes[k] = (uint32_t)(n0 << (2 * k));
        g.off[k + 1] = g.off[k] + g.nodes[k];
        g.nd[k] = (uint32_t)frac_uniform_grid(W, H, 2 * side[k], side[k], nullptr, 0);
        g.ib[k] = std::max(1u, frq1_bitlen(g.nd[k]));
        g.rb[k] = g.ib[k] + g.tb + cbits + bbits;
    }
    return g;
}

// the RD route's front end (fracenc_qtrd.hip): the pruning's partition at `lambda` as flags and bounds
int qrd_state(frac_ctx* c, uint32_t cbits, uint32_t bbits, unsigned long long lambda, unsigned long long* flag,
              unsigned long long* mm);

// The stream of the partition the front end describes: rec = the rate state's nodes (n_rec unused; by the split
// keys rate_e at `split`, or with rd_lambda by the pruning at *rd_lambda) or the search's n_rec leaves.  The
// caller has validated the arguments and set the device.
int frq1_pack_stream(frac_ctx* c, Frq1Geom g, uint32_t W, uint32_t H, uint32_t max_size, uint32_t min_size, uint32_t T,
                     uint32_t stream_flags, const double* rate_e, double split, const frac_qt_leaf* rec, uint32_t n_rec,
                     uint8_t* out, size_t cap, size_t* n_out, const unsigned long long* rd_lambda = nullptr)
{
    auto& P = c->frq1pack;
    const uint32_t total = g.off[g.levels];
    uint32_t leaves = 0, words = 0;
    double mm[4] = {0.0, 0.0, 0.0, 0.0};
    if (total) {
        const uint64_t bound = frq1_body_bound(g);
        if (bound >= (1ull << 31))
            return c->fail(FRAC_E_INVALID, "FRQ1 pack: the stream could exceed 8 GiB");
        g.cap_words = (uint32_t)bound;
        FRAC_HIP(c, P.d_flag.ensure((size_t)total + 1));
        FRAC_HIP(c, P.d_rank.ensure((size_t)total + 1));
        FRAC_HIP(c, P.d_body.ensure(g.cap_words));
        FRAC_HIP(c, P.d_mm.ensure(4));
        FRAC_HIP(c, P.d_tab.ensure(1));
        FRAC_HIP(c, P.h_res.ensure());
        size_t need = 0;
        FRAC_HIP(c, hipcub::DeviceScan::ExclusiveSum(nullptr, need, P.d_flag.ptr, P.d_rank.ptr, (int)total + 1,
                                                     c->stream));
        if (need > P.tmp_bytes) {
            FRAC_HIP(c, P.d_tmp.ensure(need));
            P.tmp_bytes = need;
        }
        void* dres = nullptr;
        FRAC_HIP(c, hipHostGetDevicePointer(&dres, P.h_res.ptr, 0));
        FRAC_HIP(c, hipMemsetAsync(P.d_mm.ptr, 0, 4 * sizeof(unsigned long long), c->stream));
        FRAC_HIP(c, hipMemsetAsync(P.d_body.ptr, 0, (size_t)g.cap_words * sizeof(uint32_t), c->stream));
        const uint32_t blocks = (total + 1 + 255) / 256;
        const uint32_t* slot = nullptr;
        if (rd_lambda) {
            FRAC_TRY(qrd_state(c, g.cbits, g.bbits, *rd_lambda, P.d_flag.ptr, P.d_mm.ptr));
        } else if (rate_e) {
            frq1_state_rate<<<blocks, 256, 0, c->stream>>>(g, rate_e, split, rec, P.d_flag.ptr, P.d_mm.ptr);
        } else {
            FRAC_HIP(c, P.d_slot.ensure(total));
            FRAC_HIP(c, hipMemsetAsync(P.d_slot.ptr, 0xff, (size_t)total * sizeof(uint32_t), c->stream));
            if (n_rec)
                frq1_slots<<<(n_rec + 255) / 256, 256, 0, c->stream>>>(g, rec, n_rec, P.d_slot.ptr);
            frq1_state_slots<<<blocks, 256, 0, c->stream>>>(g, P.d_slot.ptr, rec, P.d_flag.ptr, P.d_mm.ptr);
            slot = P.d_slot.ptr;
        }
        size_t tb = P.tmp_bytes;
        FRAC_HIP(c, hipcub::DeviceScan::ExclusiveSum(P.d_tmp.ptr, tb, P.d_flag.ptr, P.d_rank.ptr, (int)total + 1,
                                                     c->stream));
        frq1_table<<<1, 64, 0, c->stream>>>(g, P.d_rank.ptr, P.d_mm.ptr, P.d_tab.ptr,
                                            reinterpret_cast<Frq1Result*>(dres));
        frq1_pack<<<blocks, 256, 0, c->stream>>>(g, P.d_flag.ptr, P.d_rank.ptr, P.d_tab.ptr, rec, slot, P.d_mm.ptr,
                                                 P.d_body.ptr);
        FRAC_HIP(c, hipGetLastError());
        FRAC_HIP(c, hipStreamSynchronize(c->stream));
        const Frq1Result res = *P.h_res.ptr;
        leaves = res.t.leaves;
        words = res.t.words;
        if (words > g.cap_words)
            return c->fail(FRAC_E_STATE, "FRQ1 pack: the body exceeded its bound");
        if (leaves) {
            mm[0] = dkey_inv(~res.mm[0]), mm[1] = dkey_inv(res.mm[1]);
            mm[2] = dkey_inv(~res.mm[2]), mm[3] = dkey_inv(res.mm[3]);
        }
        for (double v : mm)
            if (!std::isfinite(v))
                return c->fail(FRAC_E_INVALID, "FRQ1 pack: a leaf with a non-finite contrast or brightness");
    }
    const size_t size = FRAC_FRQ1_HEADER_BYTES + (size_t)words * 4;
    *n_out = size;
    if (!out)
        return FRAC_OK;
    uint8_t hdr[FRAC_FRQ1_HEADER_BYTES];
    frq1_header(hdr, W, H, max_size, min_size, T, stream_flags, g.cbits, g.bbits, leaves, mm);
    std::memcpy(out, hdr, std::min<size_t>(cap, FRAC_FRQ1_HEADER_BYTES));
    if (cap > FRAC_FRQ1_HEADER_BYTES && words)
        FRAC_HIP(c, hipMemcpy(out + FRAC_FRQ1_HEADER_BYTES, P.d_body.ptr, std::min(cap, size) - FRAC_FRQ1_HEADER_BYTES,
                              hipMemcpyDeviceToHost));
    return FRAC_OK;
}

} // namespace

extern "C" {

int frac_quadtree_rate_stream(frac_ctx* c, double split, uint32_t cbits, uint32_t bbits, uint8_t* out, size_t cap,
                              size_t* n_out)
{
    if (!c)
        return FRAC_E_INVALID;
    FRAC_TRY(qtr_reader_checks(c, "quadtree rate stream", cbits, bbits));
    if (!n_out)
        return c->fail(FRAC_E_INVALID, "quadtree rate stream: n_out is required");
    const auto& R = c->rate;
    const Frq1Geom g = frq1_geom(R.W, R.H, R.max_size, R.min_size, R.transforms, cbits, bbits);
    return frq1_pack_stream(c, g, R.W, R.H, R.max_size, R.min_size, R.transforms, R.classifier ? 1u : 0u, R.d_e.ptr,
                            split, R.d_nodes.ptr, 0, out, cap, n_out);
}

int frac_encode_quadtree_stream(frac_ctx* c, const frac_quadtree_params* qp, uint32_t cbits, uint32_t bbits,
                                uint8_t* out, size_t cap, size_t* n_out, frac_stats* stats)
{
    if (!c)
        return FRAC_E_INVALID;
    if (!qp || !n_out)
        return c->fail(FRAC_E_INVALID, "quadtree stream: params and n_out are required");
    if (cbits < 2 || cbits > 16 || bbits < 2 || bbits > 16)
        return c->fail(FRAC_E_INVALID, "quadtree stream: contrast/brightness bits must be in [2, 16]");
    uint32_t side[4];
    if (!frq1_levels(qp->max_size, qp->min_size, side))
        return c->fail(FRAC_E_INVALID, "quadtree: sizes must be 2, 4, 8 or 16 with min_size <= max_size");
    // the leaves stay in d_qt_leaves32 (frac_encode_quadtree_leaves' checks, search and statistics)
    size_t n_leaves = 0;
    FRAC_TRY(encode_quadtree_leaves_checked(c, qp, nullptr, 0, &n_leaves, stats, true));
    const uint32_t W = c->src.w, H = c->src.h, T = c->p.transforms;
    const Frq1Geom g = frq1_geom(W, H, qp->max_size, qp->min_size, T, cbits, bbits);
    return frq1_pack_stream(c, g, W, H, qp->max_size, qp->min_size, T, c->p.use_classifier ? 1u : 0u, nullptr, 0.0,
                            c->d_qt_leaves32.ptr, (uint32_t)n_leaves, out, cap, n_out);
}

} // extern "C"
