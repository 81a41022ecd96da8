// fracenc_qtrd.hip — rate–distortion-optimal partitions of the rate state's tree.  Included by fracenc_api.hip
// after fracenc_frq1pack.hip (whose bounds reduction and packer it uses) and fracenc_qtrate.hip (the tree, its
// geometry, the closed-form size and the leaf emitter).
//
// The rule (include/fracenc.h, "rate–distortion-optimal partitions"), all of it in unsigned 64-bit integers: node
// v of level k (side n) has the distortion q(v) = llrint(d(v)·64n²), 16 × its summed squared error; a leaf costs
// its record's bits rb_k and, above the last level, its bitmap bit; a split costs its bitmap bit.  For a
// multiplier Λ, bottom-up: J(v) = q(v) + Λ·rb at the last level; above it leafJ = q(v) + Λ·(rb_k + 1),
// splitJ = Λ + Σ_children J, v splits exactly when splitJ < leafJ, J(v) = the smaller.  Level 0 is reached, a node
// is reached when its parent is reached and splits, a reached node that does not split is a leaf.
//
//   qrd_q       q(v) of every node, once per rate state (the first RD reader after a build launches it)
//   qrd_prune   The pruning, with no J in memory: a level-0 node's subtree has 4^(L−1) ∈ {1, 4, 16, 64} nodes of
//               the last level, contiguous in the level-major index, so a wave holds whole subtrees.  Lane j takes
//               last-level node j and loads its own q and its ancestors' (one address per group of lanes) once;
//               per multiplier the groups of 4, 16 and 64 lanes sum J by xor shuffles, after which every lane of a
//               group holds the sum and takes the group's decision itself — nothing comes back down.  A group's
//               first lane reports the group's node.  Lanes past the last node run every shuffle with zeros; the
//               subtrees are complete, so no group mixes them with nodes.
//                 sizes mode   a chunk of multipliers per block row (blockIdx.y): S_k by ballot and popcount, the
//                              leaves' distortion by a wave sum, one atomic per wave and quantity — into one of
//                              up to 64 copies of the sums, chosen by the block, so that the thousands of waves
//                              of a large tree do not queue on one address; the readers add the copies up
//                 flag modes   one multiplier: the leaf flags frac_quadtree_rate_leaves' scan and emit take, or
//                              the packer's 64-bit reached/leaf flags with the leaves' four bounds
//   qrd_fit_*   frac_quadtree_rd_fit: rounds of 64 probes over the interval (lo, hi] of multipliers; a one-wave
//               step between two prunings picks the first fitting probe as the new hi and its predecessor as the
//               new lo and writes the next round's probes, so the rounds queue without the host; the last step
//               writes the answer into mapped host memory.
namespace {

constexpr uint32_t kQrdChunk = 16;  // multipliers a lane evaluates with its q in registers
constexpr uint32_t kQrdProbes = 64; // the fit's probes per round: one wave steps them
constexpr uint32_t kQrdCopies = 64; // at most this many copies of the per-multiplier sums (block b adds to b mod copies)
constexpr unsigned long long kQrdMaxLambda = 1ull << 32;

using QrdAcc = frac_ctx::QtRd::Acc;
using QrdFit = frac_ctx::QtRd::Fit;

// q(v) = llrint(d·64n²): an exact integer below 2^32 for every record the search makes (the largest is the default
// record's, 1e5·64·256); 0 for a negative or NaN distance.  The cap only keeps the store defined.
__global__ void __launch_bounds__(256) qrd_q(QtrGeom g, uint32_t max_size, const frac_qt_leaf* __restrict__ nodes,
                                             uint32_t* __restrict__ q)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.off[g.levels])
        return;
    uint32_t k = 0;
    while (k + 1 < g.levels && i >= g.off[k + 1])
        ++k;
    const uint32_t n = max_size >> k;
    const double d = nodes[i].distance;
    uint32_t v = 0;
    if (d > 0.0) {
        const double s = d * (64.0 * n * n);
        v = s >= 4294967295.0 ? 0xffffffffu : (uint32_t)llrint(s);
    }
    q[i] = v;
}

enum { QRD_SIZES = 0, QRD_LEAF_FLAGS = 1, QRD_PACK_FLAGS = 2 };

// L = the tree's levels.  lam = the multipliers in device memory (sizes mode), else the one multiplier lam1.
template <int L, int MODE>
__global__ void __launch_bounds__(256) qrd_prune(QtrGeom g, const uint32_t* __restrict__ q,
                                                 const unsigned long long* __restrict__ lam, unsigned long long lam1,
                                                 uint32_t n_lam, QrdAcc* __restrict__ acc, uint32_t copies,
                                                 uint32_t* __restrict__ flag32, unsigned long long* __restrict__ flag64,
                                                 const frac_qt_leaf* __restrict__ nodes,
                                                 unsigned long long* __restrict__ mm)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x; // the last level's node
    const bool valid = t < g.nodes[L - 1];
    // the lane's own node (k = L − 1) and its ancestors: index, q, and whether the lane is its group's first
    uint32_t idx[L], qv[L];
    bool first[L];
#pragma unroll
    for (int k = 0; k < L; ++k) {
        const uint32_t sh = 2 * (L - 1 - k);
        idx[k] = g.off[k] + (t >> sh);
        first[k] = valid && (t & ((1u << sh) - 1u)) == 0;
        qv[k] = valid ? q[idx[k]] : 0u;
    }
    const bool lane0 = (threadIdx.x & 63u) == 0;
    const uint32_t i0 = MODE == QRD_SIZES ? blockIdx.y * kQrdChunk : 0u;
    const uint32_t i1 = MODE == QRD_SIZES ? min(i0 + kQrdChunk, n_lam) : 1u;
    if constexpr (MODE == QRD_SIZES)
        acc += (size_t)(blockIdx.x % copies) * n_lam;
    for (uint32_t i = i0; i < i1; ++i) {
        const unsigned long long lm = MODE == QRD_SIZES ? lam[i] : lam1;
        unsigned long long J = valid ? qv[L - 1] + lm * g.rb[L - 1] : 0ull;
        bool split[L]; // [L − 1] stays false: the last level does not split
        split[L - 1] = false;
        // every lane runs every shuffle: nothing has returned, and a group is all nodes or none
#pragma unroll
        for (int k = L - 2; k >= 0; --k) {
            const int o = 1 << (2 * (L - 2 - k));
            J += (unsigned long long)__shfl_xor((long long)J, o, 64);
            J += (unsigned long long)__shfl_xor((long long)J, 2 * o, 64);
            const unsigned long long sj = lm + J, lj = qv[k] + lm * (g.rb[k] + 1u);
            split[k] = sj < lj; // strict: a tie keeps the leaf
            J = split[k] ? sj : lj;
        }
        bool reached = valid;
        unsigned long long d = 0;
#pragma unroll
        for (int k = 0; k < L; ++k) {
            const bool mine = first[k] && reached; // a reached node, and this lane's to report
            const bool leaf = mine && !split[k];
            if constexpr (MODE == QRD_SIZES) {
                d += leaf ? qv[k] : 0u;
                if (k < L - 1) {
                    const uint32_t s = (uint32_t)__popcll(__ballot(mine && split[k]));
                    if (lane0 && s)
                        atomicAdd(&acc[i].S[k], s);
                }
            } else if constexpr (MODE == QRD_LEAF_FLAGS) {
                if (first[k])
                    flag32[idx[k]] = leaf ? 1u : 0u;
            } else {
                if (first[k])
                    flag64[idx[k]] = (unsigned long long)(reached ? 1u : 0u) << 32 | (leaf ? 1u : 0u);
                frq1_bounds(leaf, leaf ? nodes[idx[k]].contrast : 0.0, leaf ? nodes[idx[k]].brightness : 0.0, mm);
            }
            reached = reached && split[k];
        }
        if constexpr (MODE == QRD_SIZES) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1)
                d += (unsigned long long)__shfl_xor((long long)d, o, 64);
            if (lane0 && d)
                atomicAdd(&acc[i].dist, d);
        }
    }
    if (MODE == QRD_LEAF_FLAGS && t == 0)
        flag32[g.off[L]] = 0u; // the exclusive scan's last word: the leaf count
    if (MODE == QRD_PACK_FLAGS && t == 0)
        flag64[g.off[L]] = 0ull;
}

// per multiplier the closed-form size of its split counts
// the sums of multiplier i over the copies
__device__ inline QrdAcc qrd_sum(const QrdAcc* __restrict__ acc, uint32_t copies, uint32_t n, uint32_t i)
{
    QrdAcc a{0, {0, 0, 0, 0}};
    for (uint32_t c = 0; c < copies; ++c) {
        const QrdAcc b = acc[(size_t)c * n + i];
        a.dist += b.dist;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            a.S[k] += b.S[k];
    }
    return a;
}

__global__ void __launch_bounds__(256) qrd_sizes_finish(QtrGeom g, const QrdAcc* __restrict__ acc, uint32_t copies,
                                                        uint32_t n, unsigned long long* __restrict__ bytes,
                                                        uint32_t* __restrict__ counts,
                                                        unsigned long long* __restrict__ dist)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const QrdAcc a = qrd_sum(acc, copies, n, i);
    uint32_t S[4], leaves;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k)
        S[k] = k + 1 < g.levels ? a.S[k] : 0u;
    bytes[i] = frq1_size_of(g.levels, g.nodes[0], g.rb, S, &leaves);
    counts[5 * i] = leaves;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k)
        counts[5 * i + 1 + k] = S[k];
    dist[i] = a.dist;
}

// Probe i of a round over (lo, hi]: ascending, the last one hi, neighbours at most ceil((hi − lo)/64) apart.
// hi − lo ≤ 2^32 + 1, so the product stays far below 2^64.
__device__ inline unsigned long long qrd_probe(long long lo, unsigned long long hi, uint32_t i)
{
    const unsigned long long w = (unsigned long long)((long long)hi - lo);
    return (unsigned long long)(lo + (long long)((w * (i + 1) + kQrdProbes - 1) / kQrdProbes));
}

// the first round: (−1, 2^32], no sums yet (one wave)
__global__ void __launch_bounds__(64) qrd_fit_init(QrdFit* __restrict__ fit, unsigned long long* __restrict__ lam,
                                                   QrdAcc* __restrict__ acc, uint32_t copies)
{
    const uint32_t i = threadIdx.x;
    if (i == 0)
        *fit = QrdFit{-1, kQrdMaxLambda, 0, 0, 0, 0, 0};
    lam[i] = qrd_probe(-1, kQrdMaxLambda, i);
    for (uint32_t c = 0; c < copies; ++c)
        acc[c * kQrdProbes + i] = QrdAcc{0, {0, 0, 0, 0}};
}

// Between two rounds (one wave, lane i the probe i): the first probe whose stream fits becomes hi, the probe
// before it (which does not fit) or the old lo becomes lo.  hi's stream fits in every round but the first, where
// no fitting probe means that nothing fits: the last probe, 2^32, has the smallest stream there is.  Writes the
// next round's probes and clears the sums; the last round's step passes res, mapped host memory.
__global__ void __launch_bounds__(64) qrd_fit_step(QtrGeom g, unsigned long long max_bytes, QrdFit* __restrict__ fit,
                                                   unsigned long long* __restrict__ lam, QrdAcc* __restrict__ acc,
                                                   uint32_t copies, QrdFit* __restrict__ res)
{
    const uint32_t i = threadIdx.x;
    QrdFit f = *fit;
    const QrdAcc a = qrd_sum(acc, copies, kQrdProbes, i);
    const unsigned long long p = lam[i], dist = a.dist;
    uint32_t S[4], leaves;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k)
        S[k] = k + 1 < g.levels ? a.S[k] : 0u;
    const unsigned long long bytes = frq1_size_of(g.levels, g.nodes[0], g.rb, S, &leaves);
    const unsigned long long fits = __ballot(bytes <= max_bytes);
    if (fits) { // (wave-uniform: every lane shuffles)
        const int w = __ffsll((long long)fits) - 1;
        const long long below = __shfl((long long)p, w ? w - 1 : 0, 64);
        f.lo = w ? below : f.lo;
        f.hi = (unsigned long long)__shfl((long long)p, w, 64);
        f.bytes = (unsigned long long)__shfl((long long)bytes, w, 64);
        f.dist = (unsigned long long)__shfl((long long)dist, w, 64);
        f.leaves = (uint32_t)__shfl((int)leaves, w, 64);
        f.found = 1u;
    } else {
        f.found = 0u;
        f.min_bytes = (unsigned long long)__shfl((long long)bytes, (int)kQrdProbes - 1, 64);
    }
    lam[i] = qrd_probe(f.lo, f.hi, i);
    for (uint32_t c = 0; c < copies; ++c)
        acc[c * kQrdProbes + i] = QrdAcc{0, {0, 0, 0, 0}};
    if (i == 0) {
        *fit = f;
        if (res)
            *res = f;
    }
}

// the RD readers' checks after qtr_reader_checks, and the state's q(v) on first use
int qrd_ensure_q(frac_ctx* c)
{
    auto& R = c->rate;
    auto& D = c->rd;
    const uint32_t total = R.off[R.levels];
    if (D.q_ready || !total)
        return FRAC_OK;
    FRAC_HIP(c, D.d_q.ensure(total));
    qrd_q<<<(total + 255) / 256, 256, 0, c->stream>>>(qtr_geom(c, 2, 2), R.max_size, R.d_nodes.ptr, D.d_q.ptr);
    FRAC_HIP(c, hipGetLastError());
    D.q_ready = true;
    return FRAC_OK;
}

// the copies of the sums a sizes launch over n multipliers adds into: no more than blocks, and [copies][n] small
uint32_t qrd_copies(const QtrGeom& g, size_t n)
{
    const uint32_t blocks = (g.nodes[g.levels - 1] + 255) / 256;
    return std::max<uint32_t>(1u, std::min<uint32_t>({kQrdCopies, blocks, (uint32_t)(65536 / std::max<size_t>(n, 1))}));
}

template <int MODE>
int qrd_launch(frac_ctx* c, const QtrGeom& g, uint32_t n_lam, const unsigned long long* lam, unsigned long long lam1,
               QrdAcc* acc, uint32_t copies, uint32_t* flag32, unsigned long long* flag64, unsigned long long* mm)
{
    const dim3 grid((g.nodes[g.levels - 1] + 255) / 256, MODE == QRD_SIZES ? (n_lam + kQrdChunk - 1) / kQrdChunk : 1u);
    const uint32_t* q = c->rd.d_q.ptr;
    const frac_qt_leaf* nodes = c->rate.d_nodes.ptr;
    switch (g.levels) {
    case 1:
        qrd_prune<1, MODE><<<grid, 256, 0, c->stream>>>(g, q, lam, lam1, n_lam, acc, copies, flag32, flag64, nodes,
                                                        mm);
        break;
    case 2:
        qrd_prune<2, MODE><<<grid, 256, 0, c->stream>>>(g, q, lam, lam1, n_lam, acc, copies, flag32, flag64, nodes,
                                                        mm);
        break;
    case 3:
        qrd_prune<3, MODE><<<grid, 256, 0, c->stream>>>(g, q, lam, lam1, n_lam, acc, copies, flag32, flag64, nodes,
                                                        mm);
        break;
    default:
        qrd_prune<4, MODE><<<grid, 256, 0, c->stream>>>(g, q, lam, lam1, n_lam, acc, copies, flag32, flag64, nodes,
                                                        mm);
        break;
    }
    FRAC_HIP(c, hipGetLastError());
    return FRAC_OK;
}

// the packer's third front end (declared in fracenc_frq1pack.hip; the tree is not empty there)
int qrd_state(frac_ctx* c, uint32_t cbits, uint32_t bbits, unsigned long long lambda, unsigned long long* flag,
              unsigned long long* mm)
{
    FRAC_TRY(qrd_ensure_q(c));
    return qrd_launch<QRD_PACK_FLAGS>(c, qtr_geom(c, cbits, bbits), 1, nullptr, lambda, nullptr, 1, nullptr, flag, mm);
}

int qrd_lambda_check(frac_ctx* c, const char* who, unsigned long long lambda)
{
    if (lambda > kQrdMaxLambda)
        return c->fail(FRAC_E_INVALID, std::string(who) + ": a multiplier above 2^32");
    return FRAC_OK;
}

} // namespace

extern "C" {

int frac_quadtree_rd_sizes(frac_ctx* c, uint32_t cbits, uint32_t bbits, const uint64_t* lambda, size_t n,
                           uint64_t* bytes, uint32_t* leaves, uint32_t* splits, uint64_t* distortion)
{
    if (!c)
        return FRAC_E_INVALID;
    FRAC_TRY(qtr_reader_checks(c, "quadtree rd sizes", cbits, bbits));
    if (n && (!lambda || !bytes))
        return c->fail(FRAC_E_INVALID, "quadtree rd sizes: lambda and bytes are required");
    if (n > (size_t)65535 * kQrdChunk)
        return c->fail(FRAC_E_INVALID, "quadtree rd sizes: too many multipliers");
    for (size_t i = 0; i < n; ++i)
        FRAC_TRY(qrd_lambda_check(c, "quadtree rd sizes", lambda[i]));
    if (!n)
        return FRAC_OK;
    auto& R = c->rate;
    auto& D = c->rd;
    const QtrGeom g = qtr_geom(c, cbits, bbits);
    if (!R.off[R.levels]) { // no level-0 ranges: the header alone, whatever the multiplier
        for (size_t i = 0; i < n; ++i) {
            bytes[i] = FRAC_FRQ1_HEADER_BYTES;
            if (leaves)
                leaves[i] = 0;
            if (splits)
                std::memset(splits + 4 * i, 0, 4 * sizeof(uint32_t));
            if (distortion)
                distortion[i] = 0;
        }
        return FRAC_OK;
    }
    FRAC_TRY(qrd_ensure_q(c));
    const uint32_t copies = qrd_copies(g, n);
    FRAC_HIP(c, D.d_lam.ensure(n));
    FRAC_HIP(c, D.d_acc.ensure((size_t)copies * n));
    FRAC_HIP(c, D.d_bytes.ensure(n));
    FRAC_HIP(c, D.d_dist.ensure(n));
    FRAC_HIP(c, D.d_counts.ensure(5 * n));
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long));
    FRAC_HIP(c, hipMemcpyAsync(D.d_lam.ptr, lambda, n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    FRAC_HIP(c, hipMemsetAsync(D.d_acc.ptr, 0, (size_t)copies * n * sizeof(QrdAcc), c->stream));
    FRAC_TRY(qrd_launch<QRD_SIZES>(c, g, (uint32_t)n, D.d_lam.ptr, 0, D.d_acc.ptr, copies, nullptr, nullptr, nullptr));
    qrd_sizes_finish<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(g, D.d_acc.ptr, copies, (uint32_t)n,
                                                                        D.d_bytes.ptr, D.d_counts.ptr, D.d_dist.ptr);
    FRAC_HIP(c, hipGetLastError());
    std::vector<uint32_t> counts(5 * n);
    FRAC_HIP(c, hipMemcpyAsync(bytes, D.d_bytes.ptr, n * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (distortion)
        FRAC_HIP(c, hipMemcpyAsync(distortion, D.d_dist.ptr, n * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    FRAC_HIP(c, hipMemcpyAsync(counts.data(), D.d_counts.ptr, 5 * n * sizeof(uint32_t), hipMemcpyDeviceToHost,
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

int frac_quadtree_rd_fit(frac_ctx* c, uint32_t cbits, uint32_t bbits, uint64_t max_bytes, uint64_t* lambda,
                         uint64_t* bytes, uint32_t* leaves, uint64_t* distortion)
{
    if (!c)
        return FRAC_E_INVALID;
    FRAC_TRY(qtr_reader_checks(c, "quadtree rd fit", cbits, bbits));
    auto& R = c->rate;
    auto& D = c->rd;
    QrdFit res{-1, 0, FRAC_FRQ1_HEADER_BYTES, 0, FRAC_FRQ1_HEADER_BYTES, 0, max_bytes >= FRAC_FRQ1_HEADER_BYTES};
    if (R.off[R.levels]) {
        const QtrGeom g = qtr_geom(c, cbits, bbits);
        FRAC_TRY(qrd_ensure_q(c));
        const uint32_t copies = qrd_copies(g, kQrdProbes);
        FRAC_HIP(c, D.d_lam.ensure(kQrdProbes));
        FRAC_HIP(c, D.d_acc.ensure((size_t)copies * kQrdProbes));
        FRAC_HIP(c, D.d_fit.ensure(1));
        FRAC_HIP(c, D.h_fit.ensure());
        void* dres = nullptr;
        FRAC_HIP(c, hipHostGetDevicePointer(&dres, D.h_fit.ptr, 0));
        // the rounds that bring the 2^32 + 1 multipliers of (−1, 2^32] down to one
        uint32_t rounds = 0;
        for (unsigned long long w = kQrdMaxLambda + 1; w > 1; w = (w + kQrdProbes - 1) / kQrdProbes)
            ++rounds;
        qrd_fit_init<<<1, 64, 0, c->stream>>>(D.d_fit.ptr, D.d_lam.ptr, D.d_acc.ptr, copies);
        for (uint32_t r = 0; r < rounds; ++r) {
            FRAC_TRY(qrd_launch<QRD_SIZES>(c, g, kQrdProbes, D.d_lam.ptr, 0, D.d_acc.ptr, copies, nullptr, nullptr,
                                           nullptr));
            qrd_fit_step<<<1, 64, 0, c->stream>>>(g, max_bytes, D.d_fit.ptr, D.d_lam.ptr, D.d_acc.ptr, copies,
                                                  r + 1 == rounds ? reinterpret_cast<QrdFit*>(dres) : nullptr);
        }
        FRAC_HIP(c, hipGetLastError());
        FRAC_HIP(c, hipStreamSynchronize(c->stream));
        res = *D.h_fit.ptr;
    }
    if (!res.found)
        return c->fail(FRAC_E_INVALID, "quadtree rd fit: no multiplier fits " + std::to_string(max_bytes) +
                                           " bytes; the smallest size is " + std::to_string(res.min_bytes) + " bytes");
    if (lambda)
        *lambda = res.hi;
    if (bytes)
        *bytes = res.bytes;
    if (leaves)
        *leaves = res.leaves;
    if (distortion)
        *distortion = res.dist;
    return FRAC_OK;
}

int frac_quadtree_rd_leaves(frac_ctx* c, uint32_t cbits, uint32_t bbits, uint64_t lambda, frac_qt_leaf* out,
                            size_t cap, size_t* n_out)
{
    if (!c)
        return FRAC_E_INVALID;
    FRAC_TRY(qtr_reader_checks(c, "quadtree rd leaves", cbits, bbits));
    FRAC_TRY(qrd_lambda_check(c, "quadtree rd leaves", lambda));
    if (!n_out)
        return c->fail(FRAC_E_INVALID, "quadtree rd leaves: n_out is required");
    return qtr_leaves_by(c, out, cap, n_out, [&](uint32_t* flag) {
        FRAC_TRY(qrd_ensure_q(c));
        return qrd_launch<QRD_LEAF_FLAGS>(c, qtr_geom(c, cbits, bbits), 1, nullptr, lambda, nullptr, 1, flag, nullptr,
                                          nullptr);
    });
}

int frac_quadtree_rd_stream(frac_ctx* c, uint64_t lambda, uint32_t cbits, uint32_t bbits, uint8_t* out, size_t cap,
                            size_t* n_out)
{
    if (!c)
        return FRAC_E_INVALID;
    FRAC_TRY(qtr_reader_checks(c, "quadtree rd stream", cbits, bbits));
    FRAC_TRY(qrd_lambda_check(c, "quadtree rd stream", lambda));
    if (!n_out)
        return c->fail(FRAC_E_INVALID, "quadtree rd stream: n_out is required");
    const auto& R = c->rate;
    const Frq1Geom g = frq1_geom(R.W, R.H, R.max_size, R.min_size, R.transforms, cbits, bbits);
    const unsigned long long lm = lambda;
    return frq1_pack_stream(c, g, R.W, R.H, R.max_size, R.min_size, R.transforms, R.classifier ? 1u : 0u, nullptr, 0.0,
                            R.d_nodes.ptr, 0, out, cap, n_out, &lm);
}

} // extern "C"
