// fracenc_qtrate.hip — quadtree rate sweep: every split distance's FRQ1 size from one search.  Included by
// fracenc_api.hip (after fracenc_codec.hip, whose FRQ1 helpers it uses).
//
// frac_quadtree_rate_build searches the FULL tree — every node of every level, level k's N_k = 4^k·N_0 nodes
// in the order "for each node of level k − 1 its quadrants TL, TR, BL, BR" — through the level machinery the
// host-planned quadtree path uses (LevelGrid, a device-built range list, frac_run, settle_fallback).  Per
// level, qtr_ranges builds the range list from the node index and qtr_store keeps each node's record as a
// 32-byte leaf (qt_leaf_of) and its split key e(v) = min(d(v), e(parent(v))): under split distance t node v is
// reached and split exactly when e(v) > t, so the partition at any t is a function of the keys.  The keys are
// sorted once (64-bit order-preserving patterns, the level as payload) and prefix-counted per level, after
// which the split counts S_k(t) are one binary search and an FRQ1 stream's size a closed form of them
// (frq1_size_of: fractencode_amd/codec.py's layout).  The readers:
//   frac_quadtree_rate_sizes   qtr_sizes: per caller threshold the search and the closed form
//   frac_quadtree_rate_fit     qtr_fit: the size at every distinct candidate {0.0} ∪ {e(v)}, a minimum over the
//                              fitting ones (no monotonicity assumed); qtr_fit_finish: its size and leaf count
//   frac_quadtree_rate_leaves  qtr_leaf_flags + one scan over the level-major node list (which is FRQ1's
//                              canonical order) + qtr_emit: whole 32-byte stores into the caller's memory
// No reader searches, plans on the host or sizes anything from a device count.
#include <hipcub/hipcub.hpp>

namespace {

// doubles as unsigned 64-bit patterns of the same order (negative values and both zeros included)
__host__ __device__ inline unsigned long long qtr_key(double v)
{
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    return (u >> 63) ? ~u : u | (1ull << 63);
}
__host__ __device__ inline double qtr_val(unsigned long long k)
{
    return __builtin_bit_cast(double, (k >> 63) ? k ^ (1ull << 63) : ~k);
}

// what the kernels need of the tree and of the stream's record widths
struct QtrGeom {
    uint32_t levels, nkeys;
    uint32_t nodes[4], off[5];
    uint32_t rb[4]; // record bits per level
};

// The size of an FRQ1 stream whose partition splits S[k] nodes of level k < levels − 1 (codec.py's layout):
// the header, per level but the last a bitmap over its N_k nodes, per level its M_k = N_k − S_k records, each
// section padded to a dword; N_0 = n0, N_{k+1} = 4·S_k.  *leaves = Σ M_k.
__host__ __device__ inline unsigned long long frq1_size_of(uint32_t levels, uint32_t n0, const uint32_t* rb,
                                                           const uint32_t* S, uint32_t* leaves)
{
    unsigned long long bytes = FRAC_FRQ1_HEADER_BYTES, N = n0, total = 0;
    for (uint32_t k = 0; k < levels; ++k) {
        const bool last = k + 1 == levels;
        if (!last)
            bytes += 4ull * ((N + 31) / 32);
        const unsigned long long Sk = last ? 0ull : S[k], M = N - Sk;
        bytes += 4ull * ((M * rb[k] + 31) / 32);
        total += M;
        N = 4 * Sk;
    }
    if (leaves)
        *leaves = (uint32_t)total;
    return bytes;
}

// level k's range list from the node index: the level-0 item (row-major in a grid of cols0 columns) and one
// quadrant digit per level below it, most significant first
__global__ void __launch_bounds__(256) qtr_ranges(uint32_t k, uint32_t max_size, uint32_t cols0, uint32_t count,
                                                  frac_grid_item* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count)
        return;
    const uint32_t i0 = i >> (2 * k);
    uint32_t x = (i0 % cols0) * max_size, y = (i0 / cols0) * max_size;
    for (uint32_t j = 1; j <= k; ++j) {
        const uint32_t q = (i >> (2 * (k - j))) & 3u, h = max_size >> j;
        x += (q & 1u) * h;
        y += (q >> 1) * h;
    }
    const uint32_t n = max_size >> k;
    out[i] = frac_grid_item{x, y, n, n, -1};
}

// a searched level into the tree: the records as leaves, and (levels that can split) the split keys
__global__ void __launch_bounds__(256) qtr_store(const frac_encode_item* __restrict__ rec, uint32_t count,
                                                 uint32_t dcols, uint32_t level, frac_qt_leaf* __restrict__ nodes,
                                                 double* __restrict__ e, const double* __restrict__ e_parent,
                                                 unsigned long long* __restrict__ key, uint32_t* __restrict__ lvl)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count)
        return;
    const frac_encode_item r = rec[i];
    nodes[i] = qt_leaf_of(r, dcols);
    if (!e)
        return;
    double v = r.match.score.distance;
    if (e_parent) {
        const double p = e_parent[i >> 2];
        v = p < v ? p : v;
    }
    e[i] = v;
    key[i] = qtr_key(v);
    lvl[i] = level;
}

struct QtrLevelIs {
    uint32_t k;
    __host__ __device__ uint32_t operator()(uint32_t l) const { return l == k ? 1u : 0u; }
};

// keys ≤ t in sorted order: the first position whose key exceeds t (the comparison the split makes, in double)
__device__ inline uint32_t qtr_upper(const unsigned long long* __restrict__ skey, uint32_t n, double t)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (qtr_val(skey[mid]) > t)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// the stream size with the first `pos` sorted keys not splitting: S_k = N_k − (level-k keys among them)
__device__ inline unsigned long long qtr_size_at(const QtrGeom& g, const uint32_t* __restrict__ pre, uint32_t pos,
                                                 uint32_t S[4], uint32_t* leaves)
{
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k)
        S[k] = k + 1 < g.levels ? g.nodes[k] - pre[(size_t)k * (g.nkeys + 1) + pos] : 0u;
    return frq1_size_of(g.levels, g.nodes[0], g.rb, S, leaves);
}

__global__ void __launch_bounds__(256) qtr_sizes(QtrGeom g, const unsigned long long* __restrict__ skey,
                                                 const uint32_t* __restrict__ pre, const double* __restrict__ split,
                                                 uint32_t n, unsigned long long* __restrict__ bytes,
                                                 uint32_t* __restrict__ counts)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    uint32_t S[4], leaves;
    bytes[i] = qtr_size_at(g, pre, qtr_upper(skey, g.nkeys, split[i]), S, &leaves);
    counts[5 * i] = leaves;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k)
        counts[5 * i + 1 + k] = S[k];
}

// The size at every distinct candidate: thread i < nkeys takes sorted key i when it is the last of its ties
// (the comparison is strict: equal keys stop splitting together), thread nkeys the candidate 0.0.
// fit[0] = the least fitting candidate's key, fit[1] = the least size (both all-ones beforehand); one atomic
// pair per wave.
__global__ void __launch_bounds__(256) qtr_fit(QtrGeom g, const unsigned long long* __restrict__ skey,
                                               const uint32_t* __restrict__ pre, unsigned long long max_bytes,
                                               unsigned long long* __restrict__ fit)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long best = ~0ull, least = ~0ull;
    if (i <= g.nkeys) {
        unsigned long long key = qtr_key(0.0);
        uint32_t pos = 0;
        bool take = true;
        if (i < g.nkeys) {
            key = skey[i];
            pos = i + 1;
            take = pos == g.nkeys || skey[pos] != key;
        } else {
            pos = qtr_upper(skey, g.nkeys, 0.0);
        }
        if (take) {
            uint32_t S[4];
            least = qtr_size_at(g, pre, pos, S, nullptr);
            if (least <= max_bytes)
                best = key;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long b = (unsigned long long)__shfl_xor((long long)best, o, 64);
        const unsigned long long l = (unsigned long long)__shfl_xor((long long)least, o, 64);
        best = b < best ? b : best;
        least = l < least ? l : least;
    }
    if ((threadIdx.x & 63u) == 0) {
        if (best != ~0ull)
            atomicMin(&fit[0], best);
        atomicMin(&fit[1], least);
    }
}

// the fit's answer into mapped host memory: the candidate, its size and leaf count (one thread)
__global__ void qtr_fit_finish(QtrGeom g, const unsigned long long* __restrict__ skey,
                               const uint32_t* __restrict__ pre, const unsigned long long* __restrict__ fit,
                               frac_ctx::QtRate::Result* __restrict__ res)
{
    if (blockIdx.x || threadIdx.x)
        return;
    res->key = fit[0];
    res->min_bytes = fit[1];
    res->found = fit[0] != ~0ull ? 1u : 0u;
    res->bytes = 0;
    res->leaves = 0;
    if (res->found) {
        uint32_t S[4], leaves;
        res->bytes = qtr_size_at(g, pre, qtr_upper(skey, g.nkeys, qtr_val(fit[0])), S, &leaves);
        res->leaves = leaves;
    }
}

// Node i of the level-major tree is a leaf under t when it is reached (level 0, or its parent's key exceeds t)
// and does not split (the last level, or its own key does not exceed t).  flag[total] = 0, so the exclusive
// scan's last word is the leaf count.
__global__ void __launch_bounds__(256) qtr_leaf_flags(QtrGeom g, const double* __restrict__ e, double t,
                                                      uint32_t* __restrict__ flag)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, total = g.off[g.levels];
    if (i > total)
        return;
    uint32_t f = 0;
    if (i < total) {
        uint32_t k = 0;
        while (k + 1 < g.levels && i >= g.off[k + 1])
            ++k;
        const uint32_t j = i - g.off[k];
        const bool reached = k == 0 || e[g.off[k - 1] + (j >> 2)] > t;
        const bool splits = k + 1 < g.levels && e[i] > t;
        f = reached && !splits ? 1u : 0u;
    }
    flag[i] = f;
}

__global__ void __launch_bounds__(256) qtr_emit(const frac_qt_leaf* __restrict__ nodes,
                                                const uint32_t* __restrict__ flag, const uint32_t* __restrict__ rank,
                                                uint32_t total, frac_qt_leaf* __restrict__ out, uint32_t cap,
                                                frac_ctx::QtRate::Result* __restrict__ res)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0)
        res->leaves = rank[total];
    if (i < total && flag[i] && rank[i] < cap)
        out[rank[i]] = nodes[i];
}

QtrGeom qtr_geom(const frac_ctx* c, uint32_t cbits, uint32_t bbits)
{
    const auto& R = c->rate;
    QtrGeom g{};
    g.levels = R.levels;
    g.nkeys = R.nkeys;
    const uint32_t tb = std::max(1u, frq1_bitlen(R.transforms - 1));
    for (uint32_t k = 0; k < 4; ++k) {
        g.nodes[k] = R.nodes[k];
        g.rb[k] = k < R.levels ? std::max(1u, frq1_bitlen(R.ndoms[k])) + tb + cbits + bbits : 0u;
    }
    for (uint32_t k = 0; k < 5; ++k)
        g.off[k] = R.off[k];
    return g;
}

int qtr_reader_checks(frac_ctx* c, const char* who, uint32_t cbits, uint32_t bbits)
{
    if (!c->rate.ready)
        return c->fail(FRAC_E_STATE, std::string(who) + ": no readable rate state (frac_quadtree_rate_build, and no "
                                                        "setter, frac_run or quadtree encode since)");
    if (cbits < 2 || cbits > 16 || bbits < 2 || bbits > 16)
        return c->fail(FRAC_E_INVALID, std::string(who) + ": contrast/brightness bits must be in [2, 16]");
    FRAC_HIP(c, hipSetDevice(c->device));
    return FRAC_OK;
}

// The leaves a partition of the rate state's tree names, in canonical order, into the caller's memory: `flags`
// launches what writes the [total + 1] leaf flags (the last one 0); then one scan and qtr_emit.  The caller has
// run qtr_reader_checks.
template <class Flags>
int qtr_leaves_by(frac_ctx* c, frac_qt_leaf* out, size_t cap, size_t* n_out, Flags&& flags)
{
    auto& R = c->rate;
    const uint32_t total = R.off[R.levels];
    *n_out = 0;
    if (!total)
        return FRAC_OK;
    // device memory and pinned host memory are written directly; pageable memory through d_out and one copy
    frac_qt_leaf* dst = nullptr;
    if (out && cap) {
        hipPointerAttribute_t at{};
        void* dp = nullptr;
        if (hipPointerGetAttributes(&at, out) == hipSuccess) {
            if (at.type == hipMemoryTypeDevice)
                dst = out;
            else if (at.type == hipMemoryTypeHost && hipHostGetDevicePointer(&dp, out, 0) == hipSuccess && dp)
                dst = reinterpret_cast<frac_qt_leaf*>(dp);
        }
        (void)hipGetLastError(); // pageable memory is not an error
    }
    const bool staged = out && cap && !dst;
    if (staged)
        dst = R.d_out.ptr;
    const uint32_t dcap = !out ? 0u : (uint32_t)std::min<size_t>(staged ? std::min(cap, R.d_out.cap) : cap, 0xffffffffu);
    void* dres = nullptr;
    FRAC_HIP(c, hipHostGetDevicePointer(&dres, R.h_res.ptr, 0));
    const uint32_t blocks = (total + 1 + 255) / 256;
    FRAC_TRY(flags(R.d_flag.ptr)); // [total + 1] leaf flags, the last one 0
    size_t tb = R.tmp_bytes;
    FRAC_HIP(c, hipcub::DeviceScan::ExclusiveSum(R.d_tmp.ptr, tb, R.d_flag.ptr, R.d_rank.ptr, (int)total + 1,
                                                 c->stream));
    qtr_emit<<<blocks, 256, 0, c->stream>>>(R.d_nodes.ptr, R.d_flag.ptr, R.d_rank.ptr, total, dst, dcap,
                                            reinterpret_cast<frac_ctx::QtRate::Result*>(dres));
    FRAC_HIP(c, hipGetLastError());
    FRAC_HIP(c, hipStreamSynchronize(c->stream));
    const uint32_t n_leaves = R.h_res->leaves;
    *n_out = n_leaves;
    if (staged && n_leaves)
        FRAC_HIP(c, hipMemcpy(out, R.d_out.ptr, std::min<size_t>(dcap, n_leaves) * sizeof(frac_qt_leaf),
                              hipMemcpyDeviceToHost));
    return FRAC_OK;
}

} // namespace

extern "C" {

int frac_quadtree_rate_build(frac_ctx* c, uint32_t max_size, uint32_t min_size, frac_stats* stats)
{
    if (!c)
        return FRAC_E_INVALID;
    // the levels' runs write no tuples into a frac_run sink (it is sized for the context's own ranges)
    struct SinkAside {
        frac_ctx* c;
        frac_tuple* saved;
        ~SinkAside() { c->tuple_sink = saved; }
    } aside{c, c->tuple_sink};
    c->tuple_sink = nullptr;
    uint32_t side[4];
    const uint32_t levels = frq1_levels(max_size, min_size, side);
    if (!levels)
        return c->fail(FRAC_E_INVALID, "quadtree rate: sizes must be 2, 4, 8 or 16 with min_size <= max_size");
    if (!c->planes_set)
        return c->fail(FRAC_E_STATE, "quadtree rate: no frame set");
    const uint32_t W = c->src.w, H = c->src.h, T = c->p.transforms;
    if (W > 0xffffu || H > 0xffffu)
        return c->fail(FRAC_E_INVALID, "quadtree rate: a frame side above 65535 does not fit the 16-bit origins");
    if (frac_uniform_grid(W, H, 2 * min_size, min_size, nullptr, 0) >= FRAC_QT_NO_DOMAIN)
        return c->fail(FRAC_E_INVALID, "quadtree rate: the finest level has more domains than a 24-bit index holds");
    FRAC_TRY(check_ab_knobs(c));
    FRAC_HIP(c, hipSetDevice(c->device));
    if (!c->same_plane && (c->tgt.w != W || c->tgt.h != H))
        return c->fail(FRAC_E_INVALID, "quadtree rate: source and target planes must have one size");
    auto& R = c->rate;
    R.ready = false;
    c->rd.q_ready = false; // the RD readers' distortions (fracenc_qtrd.hip) are of the tree searched before
    const uint64_t n0 = frac_uniform_grid(W, H, max_size, max_size, nullptr, 0);
    if ((n0 << (2 * (levels - 1))) * 4 / 3 >= (1ull << 31))
        return c->fail(FRAC_E_INVALID, "quadtree rate: the full tree has 2^31 nodes or more");
    R.W = W, R.H = H, R.max_size = max_size, R.min_size = min_size, R.levels = levels, R.transforms = T;
    R.classifier = c->p.use_classifier != 0;
    for (uint32_t k = 0; k < 4; ++k) {
        R.nodes[k] = k < levels ? (uint32_t)(n0 << (2 * k)) : 0u;
        R.ndoms[k] = k < levels ? (uint32_t)frac_uniform_grid(W, H, 2 * side[k], side[k], nullptr, 0) : 0u;
        R.off[k + 1] = R.off[k] + R.nodes[k];
    }
    R.nkeys = R.off[levels - 1];
    const uint32_t total_nodes = R.off[levels], nkeys = R.nkeys, finest = R.nodes[levels - 1];
    qt_grids_for(c, W, H);
    LevelGrid level{c, c->doms_set};
    frac_stats total{};
    HostTrace tr("quadtree rate");
    // every buffer of the state and of its readers, at the tree's size
    FRAC_HIP(c, R.d_nodes.ensure(total_nodes));
    FRAC_HIP(c, R.d_e.ensure(nkeys));
    FRAC_HIP(c, R.d_key.ensure(nkeys));
    FRAC_HIP(c, R.d_skey.ensure(nkeys));
    FRAC_HIP(c, R.d_lvl.ensure(nkeys));
    FRAC_HIP(c, R.d_slvl.ensure((size_t)nkeys + 1));
    FRAC_HIP(c, R.d_pre.ensure(3 * ((size_t)nkeys + 1)));
    FRAC_HIP(c, R.d_flag.ensure((size_t)total_nodes + 1));
    FRAC_HIP(c, R.d_rank.ensure((size_t)total_nodes + 1));
    FRAC_HIP(c, R.d_out.ensure(finest)); // a partition has at most the finest level's node count of leaves
    FRAC_HIP(c, R.d_fit.ensure(2));
    FRAC_HIP(c, R.h_res.ensure());
    using LevelIter = hipcub::TransformInputIterator<uint32_t, QtrLevelIs, const uint32_t*>;
    {
        size_t need = 0, b = 0;
        if (nkeys) {
            FRAC_HIP(c, hipcub::DeviceRadixSort::SortPairs(nullptr, b, R.d_key.ptr, R.d_skey.ptr, R.d_lvl.ptr,
                                                           R.d_slvl.ptr, (int)nkeys, 0, 64, c->stream));
            need = std::max(need, b);
        }
        FRAC_HIP(c, hipcub::DeviceScan::ExclusiveSum(nullptr, b, LevelIter(R.d_slvl.ptr, QtrLevelIs{0}), R.d_pre.ptr,
                                                     (int)nkeys + 1, c->stream));
        need = std::max(need, b);
        FRAC_HIP(c, hipcub::DeviceScan::ExclusiveSum(nullptr, b, R.d_flag.ptr, R.d_rank.ptr, (int)total_nodes + 1,
                                                     c->stream));
        need = std::max(need, b);
        if (need > R.tmp_bytes) {
            FRAC_HIP(c, R.d_tmp.ensure(need));
            R.tmp_bytes = need;
        }
    }
    FRAC_HIP(c, c->d_ranges.ensure(finest));
    FRAC_HIP(c, c->d_qt_stats.ensure(5));
    if (stats)
        FRAC_HIP(c, hipMemsetAsync(c->d_qt_stats.ptr, 0, 5 * sizeof(unsigned long long), c->stream));
    tr.mark("buffers");
    const uint32_t cols0 = n0 ? (W - max_size) / max_size + 1 : 1u;
    for (uint32_t k = 0; k < levels && n0; ++k) {
        const uint32_t n = side[k], count = R.nodes[k];
        const int lv = __builtin_ctz(n);
        if (c->qt_doms[lv].empty()) {
            c->qt_doms[lv].resize(frac_uniform_grid(W, H, 2 * n, n, nullptr, 0));
            if (!c->qt_doms[lv].empty())
                frac_uniform_grid(W, H, 2 * n, n, c->qt_doms[lv].data(), c->qt_doms[lv].size());
        }
        qtr_ranges<<<(count + 255) / 256, 256, 0, c->stream>>>(k, max_size, cols0, count, c->d_ranges.ptr);
        level.in(lv);
        c->ranges_dev = true;
        c->nr_dev = count;
        c->n_dev = n;
        c->ranges_set = true;
        c->ran = false;
        FRAC_TRY(frac_run(c));
        FRAC_TRY(settle_fallback(c)); // the level's records are complete before qtr_store reads them
        if (stats)
            qt_host_level_stats(c, count, total);
        level.out();
        const bool keyed = k + 1 < levels;
        qtr_store<<<(count + 255) / 256, 256, 0, c->stream>>>(
            c->d_out.ptr, count, W >= 2 * n ? (W - 2 * n) / n + 1 : 0u, k, R.d_nodes.ptr + R.off[k],
            keyed ? R.d_e.ptr + R.off[k] : nullptr, keyed && k ? R.d_e.ptr + R.off[k - 1] : nullptr,
            keyed ? R.d_key.ptr + R.off[k] : nullptr, keyed ? R.d_lvl.ptr + R.off[k] : nullptr);
        FRAC_HIP(c, hipGetLastError());
        if (stats && (c->p.flags & FRAC_FLAG_TIMING)) {
            FRAC_HIP(c, hipStreamSynchronize(c->stream)); // the level's run has completed
            add_run_times(total, last_events(c));
        }
        tr.mark("level");
    }
    c->ranges_dev = false;
    c->ranges.clear();
    c->dirty = true;
    c->ran = false;
    // the order: one sort of the keys with their levels, then per level the count of its keys before each position
    if (nkeys) {
        size_t tb = R.tmp_bytes;
        FRAC_HIP(c, hipcub::DeviceRadixSort::SortPairs(R.d_tmp.ptr, tb, R.d_key.ptr, R.d_skey.ptr, R.d_lvl.ptr,
                                                       R.d_slvl.ptr, (int)nkeys, 0, 64, c->stream));
    }
    FRAC_HIP(c, hipMemsetAsync(R.d_slvl.ptr + nkeys, 0xff, sizeof(uint32_t), c->stream)); // no level's key
    for (uint32_t k = 0; k + 1 < levels; ++k) {
        size_t tb = R.tmp_bytes;
        FRAC_HIP(c, hipcub::DeviceScan::ExclusiveSum(R.d_tmp.ptr, tb, LevelIter(R.d_slvl.ptr, QtrLevelIs{k}),
                                                     R.d_pre.ptr + (size_t)k * (nkeys + 1), (int)nkeys + 1, c->stream));
    }
    FRAC_HIP(c, hipStreamSynchronize(c->stream));
    tr.mark("sort + counts");
    if (stats) {
        FRAC_TRY(qt_host_read_stats(c, total));
        *stats = total;
    }
    R.ready = true;
    return FRAC_OK;
}

int frac_quadtree_rate_sizes(frac_ctx* c, uint32_t cbits, uint32_t bbits, const double* split, size_t n,
                             uint64_t* bytes, uint32_t* leaves, uint32_t* splits)
{
    if (!c)
        return FRAC_E_INVALID;
    FRAC_TRY(qtr_reader_checks(c, "quadtree rate sizes", cbits, bbits));
    if (n && (!split || !bytes))
        return c->fail(FRAC_E_INVALID, "quadtree rate sizes: split and bytes are required");
    if (n > 0x7fffffffu / 5)
        return c->fail(FRAC_E_INVALID, "quadtree rate sizes: too many thresholds");
    if (!n)
        return FRAC_OK;
    auto& R = c->rate;
    FRAC_HIP(c, R.d_split.ensure(n));
    FRAC_HIP(c, R.d_bytes.ensure(n));
    FRAC_HIP(c, R.d_counts.ensure(5 * n));
    FRAC_HIP(c, hipMemcpyAsync(R.d_split.ptr, split, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    qtr_sizes<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(qtr_geom(c, cbits, bbits), R.d_skey.ptr, R.d_pre.ptr,
                                                                 R.d_split.ptr, (uint32_t)n, R.d_bytes.ptr,
                                                                 R.d_counts.ptr);
    FRAC_HIP(c, hipGetLastError());
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long));
    std::vector<uint32_t> counts(5 * n);
    FRAC_HIP(c, hipMemcpyAsync(bytes, R.d_bytes.ptr, n * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    FRAC_HIP(c, hipMemcpyAsync(counts.data(), R.d_counts.ptr, 5 * n * sizeof(uint32_t), hipMemcpyDeviceToHost,
                               c->stream));
    FRAC_HIP(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; ++i) {
        if (leaves)
            leaves[i] = counts[5 * i];
        if (splits)
            std::memcpy(splits + 4 * i, &counts[5 * i + 1], 4 * sizeof(uint32_t));
    }
    return FRAC_OK;
}

int frac_quadtree_rate_fit(frac_ctx* c, uint32_t cbits, uint32_t bbits, uint64_t max_bytes, double* split,
                           uint64_t* bytes, uint32_t* leaves)
{
    if (!c)
        return FRAC_E_INVALID;
    FRAC_TRY(qtr_reader_checks(c, "quadtree rate fit", cbits, bbits));
    auto& R = c->rate;
    const QtrGeom g = qtr_geom(c, cbits, bbits);
    void* dres = nullptr;
    FRAC_HIP(c, hipHostGetDevicePointer(&dres, R.h_res.ptr, 0));
    FRAC_HIP(c, hipMemsetAsync(R.d_fit.ptr, 0xff, 2 * sizeof(unsigned long long), c->stream));
    qtr_fit<<<(R.nkeys + 1 + 255) / 256, 256, 0, c->stream>>>(g, R.d_skey.ptr, R.d_pre.ptr, max_bytes, R.d_fit.ptr);
    qtr_fit_finish<<<1, 64, 0, c->stream>>>(g, R.d_skey.ptr, R.d_pre.ptr, R.d_fit.ptr,
                                            reinterpret_cast<frac_ctx::QtRate::Result*>(dres));
    FRAC_HIP(c, hipGetLastError());
    FRAC_HIP(c, hipStreamSynchronize(c->stream));
    const frac_ctx::QtRate::Result res = *R.h_res.ptr;
    if (!res.found)
        return c->fail(FRAC_E_INVALID, "quadtree rate fit: no split distance fits " + std::to_string(max_bytes) +
                                           " bytes; the smallest size is " + std::to_string(res.min_bytes) + " bytes");
    if (split)
        *split = qtr_val(res.key);
    if (bytes)
        *bytes = res.bytes;
    if (leaves)
        *leaves = res.leaves;
    return FRAC_OK;
}

int frac_quadtree_rate_leaves(frac_ctx* c, double split, frac_qt_leaf* out, size_t cap, size_t* n_out)
{
    if (!c)
        return FRAC_E_INVALID;
    FRAC_TRY(qtr_reader_checks(c, "quadtree rate leaves", 2, 2));
    if (!n_out)
        return c->fail(FRAC_E_INVALID, "quadtree rate leaves: n_out is required");
    return qtr_leaves_by(c, out, cap, n_out, [&](uint32_t* flag) {
        const uint32_t total = c->rate.off[c->rate.levels];
        qtr_leaf_flags<<<(total + 1 + 255) / 256, 256, 0, c->stream>>>(qtr_geom(c, 2, 2), c->rate.d_e.ptr, split, flag);
        return FRAC_OK;
    });
}

int frac_frq1_size(uint32_t W, uint32_t H, uint32_t max_size, uint32_t min_size, uint32_t T, uint32_t cbits,
                   uint32_t bbits, const uint32_t splits[3], uint64_t* bytes)
{
    auto bad = [&](const std::string& why) {
        g_last_error = "frq1_size: " + why;
        return FRAC_E_INVALID;
    };
    if (!bytes)
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
    if (L > 1 && !splits)
        return bad("NULL argument");
    const uint32_t tb = std::max(1u, frq1_bitlen(T - 1));
    uint32_t rb[4] = {0, 0, 0, 0}, S[4] = {0, 0, 0, 0};
    uint64_t N = frac_uniform_grid(W, H, max_size, max_size, nullptr, 0);
    const uint32_t n0 = (uint32_t)N;
    for (uint32_t k = 0; k < L; ++k) {
        rb[k] = std::max(1u, frq1_bitlen(frac_uniform_grid(W, H, 2 * side[k], side[k], nullptr, 0))) + tb + cbits + bbits;
        if (rb[k] > 64)
            return bad("record wider than 64 bits");
        if (k + 1 < L) {
            S[k] = splits[k];
            if (S[k] > N)
                return bad("level " + std::to_string(k) + ": " + std::to_string(S[k]) + " splits of " +
                           std::to_string(N) + " nodes");
            N = 4ull * S[k];
        }
    }
    *bytes = frq1_size_of(L, n0, rb, S, nullptr);
    return FRAC_OK;
}

} // extern "C"
