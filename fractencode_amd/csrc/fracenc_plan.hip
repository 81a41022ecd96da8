// fracenc_plan.hip — what a run needs before its launches: validation of the grids, the classifier
// buckets (fracenc_bucket.hip), and prepare(), which plans each engine's work lists and sizes, fills
// and uploads its buffers.  Included by fracenc_api.hip.
namespace {

// Largest S16 whose reference distance fl64((S16/16)/area) is <= thr
// (TransformMatcher::checkDistance, encode/transformmatcher.h:32-34); −1 if none.
int64_t compute_hit_limit(double thr, uint32_t area)
{
    auto pred = [&](int64_t s) { return ((double)s * 0.0625) / (double)area <= thr; };
    if (!pred(0))
        return -1;
    int64_t lo = 0, hi = 1ll << 40;
    if (pred(hi))
        return hi;
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (pred(mid))
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// The classifier keys of a run or a quadtree level from the planes' block sums (bucket_keys_bs) when every
// item is at most 32 rows high (q ≤ 16): the source plane's pyramid, and the target's when it is another plane.
static int plane_block_sums(frac_ctx* c, BlockSums& bs, BlockSums& bt)
{
    FRAC_HIP(c, c->d_bsum_s.ensure(bs_words(c->src.w, c->src.h)));
    launch_block_sums(c->d_src.ptr, c->d_sstride, c->src.w, c->src.h, c->d_bsum_s.ptr, c->stream);
    bs = bs_layout(c->d_bsum_s.ptr, c->src.w, c->src.h);
    bt = bs;
    if (!c->same_plane) {
        FRAC_HIP(c, c->d_bsum_t.ensure(bs_words(c->tgt.w, c->tgt.h)));
        launch_block_sums(c->d_tgt.ptr, c->d_tstride, c->tgt.w, c->tgt.h, c->d_bsum_t.ptr, c->stream);
        bt = bs_layout(c->d_bsum_t.ptr, c->tgt.w, c->tgt.h);
    }
    return FRAC_OK;
}

// Both grids' keys (domains dw × dh, ranges rw × rh): from the planes' block sums when every side is at
// most 32, else by the row kernels
static int launch_grid_keys(frac_ctx* c, const KeySeg& kd, uint32_t dw, uint32_t dh, const KeySeg& kr, uint32_t rw,
                            uint32_t rh)
{
    if (dh <= 32 && dw <= 32 && rh <= 32 && rw <= 32) {
        BlockSums bs, bt;
        FRAC_TRY(plane_block_sums(c, bs, bt));
        launch_bucket_keys_bs(kd, bs, dw, dh, kr, bt, rw, rh, c->stream);
    } else {
        launch_bucket_keys_pair(kd, dh, kr, rh, c->stream);
    }
    return FRAC_OK;
}

// The classifier buckets on the device (fracenc_bucket.hip): d_porig (pool position → domain index),
// d_rord (ranges in bucket order), d_rkey (per range bucket); first[b] / rfirst[b] = the first pool
// position / bucket-sorted range of bucket b (b = 0..kMaxBuckets).  One small synchronous copy.
int device_buckets(frac_ctx* c, int nb, uint32_t* dfirst, uint32_t* rfirst)
{
    const uint32_t nd = (uint32_t)c->doms.size(), nr = (uint32_t)nranges(c);
    if (nb == 1) { // one bucket: the pool is the domain list, the ranges keep their order
        if (nd)
            fill_iota<<<(nd + 255) / 256, 256, 0, c->stream>>>(c->d_porig.ptr, nd);
        if (nr) {
            fill_iota<<<(nr + 255) / 256, 256, 0, c->stream>>>(c->d_rord.ptr, nr);
            FRAC_HIP(c, hipMemsetAsync(c->d_rkey.ptr, 0, nr * sizeof(uint32_t), c->stream));
        }
        for (int b = 0; b <= kMaxBuckets; ++b) {
            dfirst[b] = b == 0 ? 0u : nd;
            rfirst[b] = b == 0 ? 0u : nr;
        }
        return FRAC_OK;
    }
    HostTrace tr("buckets");
    const uint32_t m = std::max(std::max(nd, nr), 1u);
    FRAC_HIP(c, c->d_bk_keys.ensure(m));
    FRAC_HIP(c, c->d_bk_cnt.ensure((size_t)(2 * ((m + kBkTile - 1) / kBkTile) + 2) * kMaxBuckets));
    FRAC_HIP(c, c->d_bk_first.ensure(2 * (kMaxBuckets + 1) + 1));
    tr.mark("alloc");
    uint32_t* first = c->d_bk_first.ptr;
    uint32_t* err = first + 2 * (kMaxBuckets + 1);
    FRAC_HIP(c, hipMemsetAsync(err, 0, sizeof(uint32_t), c->stream));
    const auto [tplane, tstride] = target_plane(c);
    // a stored −1 is classified on the item's own plane (Classifier2::compare, Classifier2.cpp:70-81);
    // the pool order porig and the bucket-sorted ranges rord by the stable bucket sort
    // both grids' keys, in one launch for the usual 2n → n geometry
    const KeySeg kd{c->d_doms.ptr, nd, c->d_src.ptr, c->d_sstride, c->d_bk_keys.ptr, nullptr, err, nullptr};
    const KeySeg kr{c->d_ranges.ptr, nr, tplane, tstride, c->d_rkey.ptr, nullptr, err, nullptr};
    FRAC_TRY(launch_grid_keys(c, kd, c->Sw, c->Sh, kr, c->nw, c->nh));
    const BkSeg sd = bk_seg_of(c->d_bk_keys.ptr, nd, nullptr, c->d_bk_cnt.ptr, first, c->d_porig.ptr);
    const BkSeg sr = bk_seg_of(c->d_rkey.ptr, nr, nullptr, c->d_bk_cnt.ptr + (size_t)sd.tiles * kMaxBuckets,
                               first + kMaxBuckets + 1, c->d_rord.ptr);
    launch_bucket_sorts(sd, sr, c->stream);
    uint32_t h[2 * (kMaxBuckets + 1) + 1];
    tr.mark("enqueue");
    FRAC_HIP(c, hipMemcpyAsync(h, first, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    FRAC_HIP(c, hipStreamSynchronize(c->stream));
    tr.mark("D2H + sync");
    if (h[2 * (kMaxBuckets + 1)])
        return c->fail(FRAC_E_INVALID, "item category outside -1..5");
    for (int b = 0; b <= kMaxBuckets; ++b) {
        dfirst[b] = h[b];
        rfirst[b] = h[kMaxBuckets + 1 + b];
    }
    return FRAC_OK;
}

inline int mfma_variant(frac_ctx* c, int& var);
inline bool mfma_dft_enabled(const frac_ctx* c);
// the SEA tiled form's search_dft: the seed search (one tile per group) keeps the exact epilogue; the windowed
// search runs the exhaustive search's shipped form (variant 35) when kTpFastSearch
constexpr int kTpSeedVar = kDftExactVar;
constexpr bool kTpFast = kTpFastSearch;
constexpr int kTpVar = kTpFast ? kDftFastVar : kTpSeedVar;
// FRAC_ENGINE_AUTO's pruned route (n = 8, T = 4, ratio 2; DESIGN §4.4, measured in §7.4).
// kAutoPruneMinPairs: the fewest block × tile pairs (every window open) at which AUTO tries the bound; below
// it the route's fixed cost — the two sides' sort, about ten small launches, one host turnaround — is too large a
// share of the run to risk on unknown data (FRAC_FLAG_PRUNE ignores it).
// kAutoPruneBudget: the share of those pairs the windows may hold; above it the windowed search with its
// resolve costs what the exhaustive search does, and the run falls back to that.  (It bounds time only: the
// windowed search's records are sized by the layout, not by the windows; DESIGN §7.7.  The table behind it was
// measured with the windowed search's exact epilogue, before kTpVar took the guarded fast one, §7.10.)
// Measured (tools/auto_prune_sweep.py, profiles/r08/auto_prune/): a run forced to fall back costs 0.25 – 0.40 ms
// more than the exhaustive one end to end — 13.5 % at 8.4 M pairs, 8.4 % at 16.7 M (4096², a quarter of the
// ranges), 3.2 % at 66.9 M — so the 10 % line lies between the first two and the minimum sits just under the
// smallest size measured within it; the windowed search with its resolve equals the exhaustive search's time at
// a share of 0.43, rounded down to 3/8.
constexpr uint64_t kAutoPruneMinPairs = 16000000;
constexpr uint64_t kAutoPruneBudgetNum = 3, kAutoPruneBudgetDen = 8;
// FRAC_MFMA_VARIANT on the Fourier path, in a tuning build: 35 (the default: the six-MFMA form with the guarded
// constant-folded epilogue, the chunk unrolled and wave-uniform buffer_load … lds stages, kDftFastVar), 37 (35
// always carrying the winning chunk's tile mask, TMASK), 21 (the exact epilogue, kDftExactVar: the A/B of the
// guard) and 240–243 (ablations of 35).  Every other value (the direct form's schedule knobs) runs the default.
// 35 against 21: 12.09 / 12.02 vs 13.85 / 13.65 ms at C3 in two 8-round interleaved A/Bs on two boxes
// (profiles/r03/session3/r03_ab5.log, r03_ab6.log); the forms retired since — the 8- and five-MFMA forms, two
// blocks per wave, 4- and 16-wave workgroups, 8-tile stages — are measured in DESIGN §7.2.
constexpr int kDftDefaultVariant = 35;
// up to this many domain tiles the product build's search also carries the winning chunk's tile mask
// (search_dft TMASK; the tuning build's variant 37 always does)
constexpr uint32_t kDftTmaskTiles = 1024;
inline int dft_variant(int var)
{
    static const int own[] = {21, 35, 37, 240, 241, 242, 243};
    for (int v : own)
        if (var == v)
            return var;
    return kDftDefaultVariant;
}

// Domain items as the search needs them: one size (Size32u, rectangles allowed), at least 2×2 (the
// sampler reads 2×2 blocks, image/sampler.h:21-38), inside the source plane once one is set.
// frac_set_domains runs it, so a reference-side engine rejects a bad grid in its constructor
// (EncodingEngine2.cpp:22-29 catches there), and prepare() again against the current plane.
int check_domains(frac_ctx* c, const frac_grid_item* d, size_t nd)
{
    if (!nd)
        return FRAC_OK;
    const uint32_t Sw = d[0].w, Sh = d[0].h;
    if (Sw < 2 || Sh < 2)
        return c->fail(FRAC_E_INVALID, "domain sides must be at least 2");
    if ((uint64_t)nd >= (1u << 24))
        return c->fail(FRAC_E_INVALID, "at most 2^24 - 1 domains");
    for (size_t i = 0; i < nd; ++i) {
        if (d[i].w != Sw || d[i].h != Sh)
            return c->fail(FRAC_E_INVALID, "all domains must be of one size");
        if (c->planes_set && ((uint64_t)d[i].x + d[i].w > c->src.w || (uint64_t)d[i].y + d[i].h > c->src.h))
            return c->fail(FRAC_E_INVALID, "domain outside the source plane");
        if (d[i].category < -1 || d[i].category > 5)
            return c->fail(FRAC_E_INVALID, "domain category must be -1..5");
    }
    return FRAC_OK;
}

// Rectangular items: under a rotation a rectangle's samples leave its own patch
// (image/transform.h:96-109 maps x' = y for Rotate_90 with the patch's own sizes), reading the plane
// around it.  The reference reads whatever is there, inside the image; beyond the image it reads out
// of bounds.  Every 2×2 block any transform samples — at the metric points (x·⌊Sw/nw⌋, y·⌊Sh/nh⌋) and
// the fit points ((x·Sw)/nw, (y·Sh)/nh), after the sampler's edge clamp — must lie inside the source
// plane for every domain; else the search is refused.
struct SampleBox {
    int x0 = INT32_MAX, x1 = INT32_MIN, y0 = INT32_MAX, y1 = INT32_MIN;
};
// the pixels (relative to the domain origin) that transform t's 2×2 samples of an Sw×Sh domain read
// for an nw×nh range: the metric points and/or the fit points, after the sampler's edge clamp
SampleBox sample_box(int t, int Sw, int Sh, int nw, int nh, bool metric, bool fit)
{
    // the sampler's own table (fracenc_common.h lut(), which gen_sample reads), so the refusal and
    // the decode check cannot drift from the samples the kernels take
    const Aff L = lut(t);
    const int a[8] = {L.a0, L.a1, L.a2, L.a3, L.a4, L.a5, L.a6, L.a7};
    SampleBox b;
    auto add = [&](int lx, int ly) {
        if (lx == Sw - 1)
            --lx;
        if (ly == Sh - 1)
            --ly;
        const int px = a[0] * lx + a[1] * ly + a[2] * (Sw - 1) + a[3] * (Sh - 1);
        const int py = a[4] * lx + a[5] * ly + a[6] * (Sw - 1) + a[7] * (Sh - 1);
        for (int k = 0; k < 4; ++k) {
            const int qx = px + (k & 1 ? a[0] : 0) + (k & 2 ? a[1] : 0);
            const int qy = py + (k & 1 ? a[4] : 0) + (k & 2 ? a[5] : 0);
            b.x0 = std::min(b.x0, qx);
            b.x1 = std::max(b.x1, qx);
            b.y0 = std::min(b.y0, qy);
            b.y1 = std::max(b.y1, qy);
        }
    };
    for (int y = 0; y < nh; ++y)
        for (int x = 0; x < nw; ++x) {
            if (metric)
                add(x * (Sw / nw), y * (Sh / nh));
            if (fit)
                add((x * Sw) / nw, (y * Sh) / nh);
        }
    return b;
}

bool box_inside(const SampleBox& b, uint32_t x, uint32_t y, uint32_t w, uint32_t h)
{
    return (int64_t)x + b.x0 >= 0 && (int64_t)x + b.x1 < (int64_t)w && (int64_t)y + b.y0 >= 0 &&
           (int64_t)y + b.y1 < (int64_t)h;
}

int check_rect_samples(frac_ctx* c)
{
    SampleBox u;
    for (uint32_t t = 0; t < c->p.transforms; ++t) {
        const SampleBox b = sample_box((int)t, (int)c->Sw, (int)c->Sh, (int)c->nw, (int)c->nh, true, true);
        u.x0 = std::min(u.x0, b.x0);
        u.x1 = std::max(u.x1, b.x1);
        u.y0 = std::min(u.y0, b.y0);
        u.y1 = std::max(u.y1, b.y1);
    }
    for (const auto& d : c->doms)
        if (!box_inside(u, d.x, d.y, c->src.w, c->src.h))
            return c->fail(FRAC_E_INVALID, "a transform of a rectangular domain samples outside the source plane "
                                           "(the reference reads out of bounds there)");
    return FRAC_OK;
}

// prepare(), in its steps.  Geometry validation and the derived fields.
int prepare_geometry(frac_ctx* c)
{
    if (!c->planes_set || !c->doms_set || !c->ranges_set)
        return c->fail(FRAC_E_STATE, "planes, domains and ranges must be set before frac_run");
    const uint32_t T = c->p.transforms;
    // geometry (TransformMatcher::matchTransformType, encode/transformmatcher.h:70-78): n×n ranges
    // and S×S domains, S > n (main.cpp:99 rejects target >= source).  S = 2n with n ∈ {2, 4, 8, 16}
    // is every engine's decimate-then-permute path; any other pair — the CLI default 16→4 among
    // them — runs the sampled form (fracenc_gen.hip): one pool row per (domain, transform).
    // ranges: one size nw × nh (Size32u items, image/partition2.hpp:13-31: rectangles allowed)
    const uint32_t nw = c->ranges_dev ? c->n_dev : c->ranges.empty() ? 8u : c->ranges[0].w;
    const uint32_t nh = c->ranges_dev ? c->n_dev : c->ranges.empty() ? 8u : c->ranges[0].h;
    for (const auto& r : c->ranges) {
        if (c->ranges_dev)
            break; // built on the device from validated parents (frac_encode_quadtree)
        if (r.w != nw || r.h != nh)
            return c->fail(FRAC_E_INVALID, "all ranges must be of one size");
        if ((uint64_t)r.x + r.w > c->tgt.w || (uint64_t)r.y + r.h > c->tgt.h)
            return c->fail(FRAC_E_INVALID, "range outside the target plane");
    }
    if (nw < 2 || nh < 2)
        return c->fail(FRAC_E_INVALID, "range sides must be at least 2");
    if ((uint64_t)nw * nh > (1ull << 26))
        return c->fail(FRAC_E_INVALID, "ranges of more than 2^26 pixels");
    // domains: validated by frac_set_domains (one size, inside the plane); re-checked against the
    // current plane, which may have changed since
    const uint32_t Sw = c->doms.empty() ? 2u * nw : c->doms[0].w;
    const uint32_t Sh = c->doms.empty() ? 2u * nh : c->doms[0].h;
    if (!c->doms_trusted)
        FRAC_TRY(check_domains(c, c->doms.data(), c->doms.size()));
    // RootMeanSquare's different-size branch (image/metrics.h:37-50) needs a domain wider than the
    // range (its FRAC_ASSERT, :39; main.cpp:99 for the CLI's square items)
    if (Sw <= nw)
        return c->fail(FRAC_E_INVALID, "domains must be wider than the ranges (metrics.h:39, main.cpp:99)");
    const bool square = nw == nh && Sw == Sh;
    const int n = square ? (int)nw : 0;
    const bool pow2 = n == 2 || n == 4 || n == 8 || n == 16;
    c->virt = !(pow2 && Sw == 2u * nw);
    c->generic = !pow2;
    c->S = Sw;
    c->nw = nw;
    c->nh = nh;
    c->Sw = Sw;
    c->Sh = Sh;
    if (!square)
        FRAC_TRY(check_rect_samples(c));
    c->Teff = c->virt ? 1u : T;
    c->K2 = (nw * nh + 1) / 2;
    if ((uint64_t)c->doms.size() * (c->virt ? T : 1u) >= (1u << 24))
        return c->fail(FRAC_E_INVALID, "at most 2^24 - 1 domains (domains x transforms in the sampled form)");
    c->n = n;
    c->G = c->virt ? 1u : (n == 16 ? 1u : (n <= 4 ? T : 4u));
    c->NG = c->virt ? 1u : T / c->G;
    return FRAC_OK;
}

// the classifier buckets of a prepare(), as its later steps read them
struct PrepBuckets {
    int nb = 1;
    uint32_t VT = 1;              // engine pool rows per pool position
    std::vector<uint32_t> eb, ee; // per bucket: its engine pool rows [eb, ee)
    std::vector<uint32_t> rbeg;   // per bucket (+ the end): its first bucket-sorted range
    BucketLayout L{};
};

// the domain and range lists on the device, their buckets and the BucketLayout
int prepare_buckets(frac_ctx* c, PrepBuckets& B, HostTrace& tr)
{
    const uint32_t T = c->p.transforms;
    // buckets: category + 1 (0 = category −1) with the classifier, a single bucket without.  Every
    // per-item step runs on the device (device_buckets); the host works from the bucket counts.
    const int nb = c->p.use_classifier ? 7 : 1;
    const size_t nd = c->doms.size(), nr = nranges(c);
    FRAC_HIP(c, c->d_doms.ensure(nd));
    FRAC_HIP(c, c->d_ranges.ensure(nr));
    FRAC_HIP(c, c->d_porig.ensure(nd));
    FRAC_HIP(c, c->d_rord.ensure(nr));
    FRAC_HIP(c, c->d_rkey.ensure(nr));
    if (!c->doms_uploaded) {
        FRAC_TRY(upload(c, c->d_doms, c->doms));
        c->doms_uploaded = true;
    }
    if (!c->ranges_dev)
        FRAC_TRY(upload(c, c->d_ranges, c->ranges));
    uint32_t dfirst[kMaxBuckets + 1], rfirst[kMaxBuckets + 1];
    FRAC_TRY(device_buckets(c, nb, dfirst, rfirst));
    tr.mark("buckets (device)");
    c->npos = (uint32_t)nd;
    c->bucket_begin.assign(dfirst, dfirst + nb);
    c->bucket_end.assign(dfirst + 1, dfirst + nb + 1);
    std::vector<uint32_t> rbeg(rfirst, rfirst + nb + 1);
    // the engines' pool rows per bucket: pool positions, or T rows per position in the sampled form
    const uint32_t VT = c->virt ? T : 1u;
    std::vector<uint32_t> eb(nb), ee(nb);
    BucketLayout L{};
    L.nb = (uint32_t)nb;
    L.VT = VT;
    for (int b = 0; b < nb; ++b) {
        eb[b] = c->bucket_begin[b] * VT;
        ee[b] = c->bucket_end[b] * VT;
        L.dbeg[b] = c->bucket_begin[b];
        L.dcnt[b] = c->bucket_end[b] - c->bucket_begin[b];
        L.rbeg[b] = rbeg[b];
        L.rcnt[b] = rbeg[b + 1] - rbeg[b];
    }
    c->layout = L;
    B = PrepBuckets{nb, VT, std::move(eb), std::move(ee), std::move(rbeg), L};
    return FRAC_OK;
}

// the VALU engine's work list
void plan_valu_work(frac_ctx* c, const PrepBuckets& B)
{
    const int nb = B.nb;
    const BucketLayout& L = B.L;
    const auto &eb = B.eb, &ee = B.ee;
    // range slots: per bucket, padded to whole waves of 64 (the VALU engine's work lists only)
    c->work.clear();
    c->nvslots = 0;
    const bool valu_lists = c->p.engine == FRAC_ENGINE_VALU && !c->generic;
    std::vector<std::pair<uint32_t, int>> blocks; // (slot base, bucket)
    for (int b = 0; valu_lists && b < nb; ++b) {
        c->layout.slot_first[b] = c->nvslots; // used by the VALU slot fill below
        const uint32_t cnt = L.rcnt[b];
        for (uint32_t s0 = 0; s0 < cnt; s0 += 64)
            blocks.emplace_back(c->nvslots + s0, b);
        c->nvslots += (cnt + 63) / 64 * 64;
    }
    size_t total_blocks = 0;
    for (auto& bl : blocks)
        if (ee[bl.second] > eb[bl.second])
            total_blocks += c->NG;
    // domain splits: enough waves to fill 256 CUs several times over, ≥ 32 domains per wave
    const size_t target_waves = 8192;
    for (auto& bl : blocks) {
        const uint32_t b0 = eb[bl.second], b1 = ee[bl.second];
        const uint32_t D = b1 - b0;
        if (D == 0)
            continue;
        size_t splits = total_blocks ? (target_waves + total_blocks - 1) / total_blocks : 1;
        splits = std::min<size_t>(splits, std::max<uint32_t>(1u, D / 32u));
        splits = std::max<size_t>(splits, 1);
        for (uint32_t g = 0; g < c->NG; ++g)
            for (size_t s = 0; s < splits; ++s) {
                const uint32_t pb = b0 + (uint32_t)((uint64_t)D * s / splits);
                const uint32_t pe = b0 + (uint32_t)((uint64_t)D * (s + 1) / splits);
                if (pe > pb)
                    c->work.push_back(make_uint4(bl.first, pb, pe, g));
            }
    }
}

// the run's counts and thresholds, its engine and the SEA engine's form
void select_engine(frac_ctx* c, const PrepBuckets& B)
{
    const uint32_t T = c->p.transforms, nw = c->nw, nh = c->nh, Sw = c->Sw, Sh = c->Sh;
    const int n = c->n, nb = B.nb;
    const BucketLayout& L = B.L;
    c->eligible_pairs = 0;
    for (int b = 0; b < nb; ++b)
        c->eligible_pairs += (uint64_t)L.rcnt[b] * L.dcnt[b];
    c->hitH = compute_hit_limit(c->p.rms_threshold, Sw * Sh); // the domain's area (image/metrics.h:49)
    // every candidate in the reference's fp32 arithmetic (gen_fallback): with a threshold no exact error can
    // meet, and for range sides above kGenMaxN, whose S16 outgrows the search keys' error field — there the
    // exact search could not order the candidates, and S16 ≥ 2^24 is the fp32 regime anyway for almost all
    c->all_fallback = c->hitH >= kExactLimit || nw > kGenMaxN || nh > kGenMaxN;

    // engine.  MFMA: exact for every templated n (n = 16 through search_mfma16's integer epilogue).
    // SEA covers n ≤ 8 (its exact evaluation holds a candidate in one wave's VGPRs): larger ranges run
    // the exhaustive MFMA search, which gives the same records.  Range sizes without a templated
    // engine run gen_search (VALU) whatever the request.
    c->engine = c->generic                                ? FRAC_ENGINE_VALU
                : c->p.engine == FRAC_ENGINE_VALU          ? FRAC_ENGINE_VALU
                : c->p.engine == FRAC_ENGINE_SEA && n <= 8 ? FRAC_ENGINE_SEA
                                                           : FRAC_ENGINE_MFMA;
    // SEA, n = 8, T = 4: the tiled form (FRAC_FLAG_SEA_PER_RANGE keeps the per-range form; in a
    // tuning build also FRAC_SEA_TILED=0)
    {
        const char* st = ab_knob("FRAC_SEA_TILED");
        c->tp = c->engine == FRAC_ENGINE_SEA && !c->virt && n == 8 && T == 4 &&
                !(c->p.flags & FRAC_FLAG_SEA_PER_RANGE) && (st ? atoi(st) != 0 : true);
    }
    // AUTO, n = 8, T = 4, ratio 2 on the Fourier path: the tiled form's windows first (launch_tp budgeted).
    // The size condition follows in prepare(), from the groups.  More buckets than the tiled form holds,
    // a quadtree level (device-planned, or its ranges built on the device) and every other geometry stay
    // on the exhaustive route as they were.
    c->auto_prune = c->p.engine == FRAC_ENGINE_AUTO && c->engine == FRAC_ENGINE_MFMA && !c->virt && n == 8 && T == 4 &&
                    !c->all_fallback && !c->qplan && !c->ranges_dev && mfma_dft_enabled(c) &&
                    !(c->p.flags & FRAC_FLAG_EXHAUSTIVE) && nb <= kTpMaxBuckets;
}

// the tiled SEA form's buckets and groups
int plan_tp_groups(frac_ctx* c, const PrepBuckets& B)
{
    const int nb = B.nb;
    const auto& rbeg = B.rbeg;
    if (nb > kTpMaxBuckets)
        return c->fail(FRAC_E_INVALID, "SEA: too many classifier buckets");
    TpBuckets& bk = c->tp_bk;
    bk = TpBuckets{};
    bk.nb = (uint32_t)nb;
    uint32_t nt = 0, nbk = 0;
    for (int b = 0; b < nb; ++b) {
        bk.dom_begin[b] = c->bucket_begin[b];
        bk.dom_count[b] = c->bucket_end[b] - c->bucket_begin[b];
        bk.tile_first[b] = nt;
        bk.tile_count[b] = (bk.dom_count[b] + 31) / 32;
        nt += bk.tile_count[b];
        bk.rng_begin[b] = rbeg[b];
        bk.rng_count[b] = rbeg[b + 1] - rbeg[b];
        bk.blk_first[b] = nbk;
        bk.blk_count[b] = (bk.rng_count[b] + 31) / 32;
        nbk += bk.blk_count[b];
    }
    if (nt >= (1u << 28)) // chunk words hold the tile in 28 bits (search_dft CHUNKED)
        return c->fail(FRAC_E_INVALID, "SEA: too many domain tiles");
    c->ntiles = nt;
    c->nblocks = nbk;
    c->tp_key_bits = 16;
    while ((1u << (c->tp_key_bits - 16)) < (uint32_t)nb)
        ++c->tp_key_bits;
    c->tp_groups.clear();
    c->tp_full_pairs = c->tp_seed_pairs = 0;
    c->tp_blk_group.assign(nbk, make_uint2(0xffffffffu, 0u));
    for (int b = 0; b < nb; ++b) {
        if (!bk.tile_count[b])
            continue; // no domain: the bucket's ranges keep the default record
        for (uint32_t g0 = 0; g0 < bk.blk_count[b]; g0 += kDftBlocksPerWG) {
            const uint32_t gi = (uint32_t)c->tp_groups.size();
            const uint32_t nbl = std::min(kDftBlocksPerWG, bk.blk_count[b] - g0);
            c->tp_groups.push_back(make_uint4(bk.blk_first[b] + g0, nbl, bk.tile_first[b], bk.tile_count[b]));
            c->tp_full_pairs += (uint64_t)nbl * bk.tile_count[b];
            c->tp_seed_pairs += nbl;
            for (uint32_t k = 0; k < nbl; ++k)
                c->tp_blk_group[bk.blk_first[b] + g0 + k] = make_uint2(gi, k);
        }
    }
    return FRAC_OK;
}

// the MFMA engine's range blocks (32 slots) and domain tiles (32 engine pool rows), per bucket
struct MfmaBuckets {
    std::vector<uint32_t> blk_first, blk_count, tile_first, tile_count;
    uint32_t nblocks = 0; // range blocks of one copy
};

// work items: groups of up to BPW blocks of one bucket × splits of its tiles, plus, when asked for (blk_ptr and
// blk_ent not null: the direct form), the CSR map block → entry bases (work·BPW + wave) its resolve kernels read
// (copies: 2 with T = 8's flipped range blocks on the Fourier path, else 1)
void build_work(const MfmaBuckets& mb, uint32_t copies, uint32_t bpw, size_t target_wgs, std::vector<uint4>& work,
                std::vector<uint32_t>* blk_ptr, std::vector<uint32_t>* blk_ent, bool xcd_order)
{
    const bool csr = blk_ptr && blk_ent;
    const int nb = (int)mb.blk_count.size();
    const auto &blk_first = mb.blk_first, &blk_count = mb.blk_count, &tile_first = mb.tile_first,
               &tile_count = mb.tile_count;
    std::vector<uint32_t> split_of; // domain split of each work item
    // splits per bucket in proportion to its tiles, so every work item covers about
    // (groups × tiles) / target_wgs group-tiles — an equal count per bucket gave the small
    // buckets' items a few tiles each (their fixed cost of loading B fragments dominating) and
    // the large buckets' long ones the tail; Σ groups_b·splits_b ≤ target_wgs + groups
    uint64_t gtiles = 0;
    for (int b = 0; b < nb; ++b)
        if (tile_count[b])
            gtiles += (uint64_t)((blk_count[b] + bpw - 1) / bpw * copies) * tile_count[b];
    // every block of bucket b gets one entry per domain split of b: the CSR map is
    // sized by a count pass, then filled in work order (no per-block lists)
    const uint32_t ncp = copies, nbt = mb.nblocks * ncp; // T = 8 Fourier: flipped copies
    std::vector<uint32_t> nsplit(nb, 0);
    if (csr)
        blk_ptr->assign(nbt + 1, 0);
    for (int b = 0; b < nb; ++b) {
        if (!tile_count[b] || !blk_count[b])
            continue;
        const uint64_t tw = work_target(target_wgs, gtiles);
        size_t splits = gtiles ? (size_t)((tw * tile_count[b] + gtiles - 1) / gtiles) : 1;
        splits = std::max<size_t>(1, std::min<size_t>(splits, std::max<uint32_t>(1u, tile_count[b] / 4u)));
        uint32_t ns = 0;
        for (size_t sp = 0; sp < splits; ++sp)
            ns += (uint64_t)tile_count[b] * (sp + 1) / splits > (uint64_t)tile_count[b] * sp / splits;
        nsplit[b] = (uint32_t)splits;
        if (csr)
            for (uint32_t cp = 0; cp < ncp; ++cp)
                for (uint32_t k = 0; k < blk_count[b]; ++k)
                    (*blk_ptr)[cp * mb.nblocks + blk_first[b] + k + 1] = ns;
    }
    std::vector<uint32_t> cur;
    if (csr) {
        for (uint32_t b = 0; b < nbt; ++b)
            (*blk_ptr)[b + 1] += (*blk_ptr)[b];
        blk_ent->assign((*blk_ptr)[nbt], 0);
        cur.assign(blk_ptr->begin(), blk_ptr->end() - 1);
    }
    work.clear();
    for (uint32_t cp = 0; cp < ncp; ++cp)
        for (int b = 0; b < nb; ++b) {
            if (!nsplit[b])
                continue;
            const size_t splits = nsplit[b];
            const uint32_t bf = cp * mb.nblocks + blk_first[b];
            for (uint32_t g = 0; g < blk_count[b]; g += bpw) {
                const uint32_t nbk = std::min(bpw, blk_count[b] - g);
                for (size_t sp = 0; sp < splits; ++sp) {
                    const uint32_t t0 = tile_first[b] + (uint32_t)((uint64_t)tile_count[b] * sp / splits);
                    const uint32_t t1 = tile_first[b] + (uint32_t)((uint64_t)tile_count[b] * (sp + 1) / splits);
                    if (t1 <= t0)
                        continue;
                    const uint32_t w = (uint32_t)work.size();
                    work.push_back(make_uint4(bf + g, nbk, t0, t1));
                    split_of.push_back((uint32_t)sp);
                    if (csr)
                        for (uint32_t k = 0; k < nbk; ++k)
                            (*blk_ent)[cur[bf + g + k]++] = w * bpw + k;
                }
            }
        }
    if (xcd_order && !work.empty()) {
        // XCD-aware order: workgroup n runs on XCD n % 8 (dispatch round-robin), so the
        // items of one domain split go to the same XCDs and their in-flight workgroups
        // stream the same tiles through that XCD's L2 together
        constexpr uint32_t kXcd = 8;
        std::vector<std::vector<uint32_t>> q(kXcd);
        uint32_t S = 0;
        for (uint32_t sp : split_of)
            S = std::max(S, sp + 1);
        // split s → XCDs x ≡ s (mod S) when S ≤ 8 (round-robin over them), else XCD s mod 8
        std::vector<uint32_t> rr(S, 0);
        for (uint32_t w = 0; w < (uint32_t)work.size(); ++w) {
            const uint32_t sp = split_of[w];
            uint32_t x = sp % kXcd;
            if (S <= kXcd) {
                const uint32_t nx = (kXcd - 1 - sp) / S + 1; // XCDs sp, sp + S, ... below 8
                x = sp + S * (rr[sp]++ % nx);
            }
            q[x].push_back(w);
        }
        std::vector<uint32_t> order;
        order.reserve(work.size());
        std::vector<size_t> head(kXcd, 0);
        while (order.size() < work.size()) {
            bool any = false;
            for (uint32_t x = 0; x < kXcd; ++x)
                if (head[x] < q[x].size()) {
                    order.push_back(q[x][head[x]++]);
                    any = true;
                } else { // an empty queue: keep the slot's XCD busy with another split
                    for (uint32_t y = 0; y < kXcd; ++y)
                        if (head[y] < q[y].size()) {
                            order.push_back(q[y][head[y]++]);
                            any = true;
                            break;
                        }
                }
            if (!any)
                break;
        }
        std::vector<uint32_t> inv(work.size());
        std::vector<uint4> nw(work.size());
        for (uint32_t n = 0; n < (uint32_t)order.size(); ++n) {
            nw[n] = work[order[n]];
            inv[order[n]] = n;
        }
        work.swap(nw);
        if (csr)
            for (uint32_t& e : *blk_ent)
                e = inv[e / bpw] * bpw + e % bpw;
    }
}

// the MFMA engine's blocks, tiles and work lists
int plan_mfma_work(frac_ctx* c, const PrepBuckets& B)
{
    const uint32_t T = c->p.transforms;
    const int n = c->n, nb = B.nb;
    const BucketLayout& L = B.L;
    const auto &eb = B.eb, &ee = B.ee;
    // range blocks of 32 slots per bucket; domain tiles of 32 engine pool rows per bucket (the
    // maps themselves are filled on the device below)
    std::vector<uint32_t> blk_first(nb, 0), blk_count(nb, 0), tile_first(nb, 0), tile_count(nb, 0);
    uint32_t nbk = 0, nt = 0;
    for (int b = 0; b < nb; ++b) {
        blk_first[b] = nbk;
        blk_count[b] = (L.rcnt[b] + 31) / 32;
        nbk += blk_count[b];
        tile_first[b] = nt;
        tile_count[b] = (ee[b] - eb[b] + 31) / 32;
        nt += tile_count[b];
    }
    c->nblocks = nbk;
    c->ntiles = nt;
    const MfmaBuckets mb{blk_first, blk_count, tile_first, tile_count, nbk};
    c->mlayout = L;
    for (int b = 0; b < nb; ++b) {
        c->mlayout.slot_first[b] = 32 * blk_first[b];
        c->mlayout.tile_first[b] = tile_first[b];
    }
    const bool fourier = n == 8 && (T == 4 || T == 8) && !c->virt && mfma_dft_enabled(c);
    c->dft_copies = fourier && T == 8 ? 2u : 1u;
    int var = 0; // (only checked here: a bad FRAC_MFMA_VARIANT fails the preparation, not the first run)
    FRAC_TRY(mfma_variant(c, var));
    if (n == 16) // search_mfma16: mfma16_bpw(T) range blocks per 4-wave workgroup (Teff: 1 when sampled)
        build_work(mb, c->dft_copies, mfma16_bpw(c->Teff), kMfma16TargetWgs, c->m_work, &c->m_blk_ptr, &c->m_blk_ent,
                   false);
    else if (!fourier) // the Fourier search reads only its own list
        build_work(mb, c->dft_copies, 4, 8192, c->m_work, &c->m_blk_ptr, &c->m_blk_ent, false);
    else {
        c->m_work.clear();
        c->m_blk_ptr.assign(c->nblocks + 1, 0);
        c->m_blk_ent.clear();
    }
    c->m8_built = n == 8 && !c->virt && (T == 4 || c->dft_copies == 2);
    if (c->m8_built) {
        // FRAC_DFT_WGS (tuning knob): target workgroup count of the Fourier search
        const char* tw = ab_knob("FRAC_DFT_WGS");
        const size_t wgs = tw ? (size_t)std::max(1, atoi(tw)) : 8192 / kDftBlocksPerWG * 4;
        // FRAC_XCD_ORDER (tuning knob): 0 = work items in (block group, split) order
        const char* xo = ab_knob("FRAC_XCD_ORDER");
        // (no CSR map: the search merges its splits per slot itself, DftArgs::slotbest)
        build_work(mb, c->dft_copies, kDftBlocksPerWG, wgs, c->m8_work, nullptr, nullptr, xo ? atoi(xo) != 0 : true);
    } else {
        c->m8_work.clear();
    }
    return FRAC_OK;
}

// every engine's buffers, maps and the VALU work list
int fill_common(frac_ctx* c, const PrepBuckets& B)
{
    const uint32_t VT = B.VT;
    const size_t nr = nranges(c);
    const BucketLayout& L = B.L;
    const size_t P = (size_t)c->npos * VT; // engine pool rows
    FRAC_HIP(c, c->d_pool.ensure(P * (size_t)c->K2));
    FRAC_HIP(c, c->d_negsd2.ensure(P));
    FRAC_HIP(c, c->d_slot_range.ensure(c->nvslots));
    FRAC_HIP(c, c->d_rbucket.ensure(nr));
    FRAC_HIP(c, c->d_best_key.ensure(nr));
    FRAC_HIP(c, c->d_out.ensure(nr));
    FRAC_HIP(c, c->d_aux.ensure(nr));
    FRAC_HIP(c, c->d_fb_list.ensure(nr));
    FRAC_HIP(c, c->d_fb_count.ensure(1));
    FRAC_TRY(upload(c, c->d_work, c->work));
    if (nr)
        fill_rbucket<<<(unsigned)((nr + 255) / 256), 256, 0, c->stream>>>(L, c->d_rkey.ptr, (uint32_t)nr,
                                                                         c->d_rbucket.ptr);
    if (c->nvslots)
        fill_range_slots<<<(c->nvslots + 255) / 256, 256, 0, c->stream>>>(c->layout, c->d_rord.ptr, c->nvslots,
                                                                          c->d_slot_range.ptr, nullptr);
    if (c->all_fallback && nr)
        fill_iota<<<(unsigned)((nr + 255) / 256), 256, 0, c->stream>>>(c->d_fb_list.ptr, (uint32_t)nr);
    return FRAC_OK;
}

// the SEA engine's buffers and sort scratch
int fill_sea(frac_ctx* c, const PrepBuckets& B)
{
    const size_t P = (size_t)c->npos * B.VT, nr = nranges(c);
    const int n = c->n;
    const auto& ee = B.ee;
    if (c->bucket_end.size() > (size_t)kSeaMaxBuckets)
        return c->fail(FRAC_E_INVALID, "SEA: too many classifier buckets");
    FRAC_HIP(c, c->d_sea_dkey.ensure(P));
    FRAC_HIP(c, c->d_sea_dkey2.ensure(P));
    FRAC_HIP(c, c->d_sea_dpos.ensure(P));
    FRAC_HIP(c, c->d_sea_dpos2.ensure(P));
    if (!c->auto_prune) { // (the per-range form's sorted pool: AUTO's pruned route is the tiled form only)
        FRAC_HIP(c, c->d_sea_ent.ensure(P));
        FRAC_HIP(c, c->d_sea_snegsd2.ensure(P));
        FRAC_HIP(c, c->d_sea_spool.ensure(P * (size_t)(n * n / 2)));
    }
    FRAC_HIP(c, c->d_sea_rkey.ensure(nr));
    FRAC_HIP(c, c->d_sea_rkey2.ensure(nr));
    FRAC_HIP(c, c->d_sea_rord.ensure(nr));
    FRAC_HIP(c, c->d_sea_rord2.ensure(nr));
    FRAC_HIP(c, c->d_sea_bend.ensure(kSeaMaxBuckets));
    FRAC_HIP(c, c->d_sea_count.ensure(1));
    FRAC_TRY(upload(c, c->d_sea_bend, ee));
    size_t t1 = 0, t2 = 0;
    FRAC_HIP(c, sort_pairs_u32(nullptr, t1, c->d_sea_dkey.ptr, c->d_sea_dkey2.ptr, c->d_sea_dpos.ptr,
                               c->d_sea_dpos2.ptr, P, 20, c->stream));
    FRAC_HIP(c, sort_pairs_u32(nullptr, t2, c->d_sea_rkey.ptr, c->d_sea_rkey2.ptr, c->d_sea_rord.ptr,
                               c->d_sea_rord2.ptr, nr, 17, c->stream));
    size_t t3 = 0;
    FRAC_HIP(c, sort_pairs_u32(nullptr, t3, c->d_sea_rkey.ptr, c->d_sea_rkey2.ptr, c->d_sea_rord.ptr,
                               c->d_sea_rord2.ptr, nr, 20, c->stream));
    c->sea_tmp_bytes = std::max<size_t>(std::max(std::max(t1, t2), t3), 1);
    FRAC_HIP(c, c->d_sea_tmp.ensure(c->sea_tmp_bytes));
    return FRAC_OK;
}

// the tiled SEA form's buffers and groups
int fill_tp(frac_ctx* c, const PrepBuckets& B)
{
    const size_t P = (size_t)c->npos * B.VT, nr = nranges(c);
    const size_t ng = c->tp_groups.size(), nbk = c->nblocks, nt = c->ntiles;
    // The tiled form's layout is ΣD4-sorted tiles and ΣR-sorted blocks, rebuilt every run; the MFMA route's is
    // the domain and range order, filled once (fill_mfma).  Under AUTO both stay prepared, so per buffer:
    //   own copy per layout — the maps and lists the MFMA route fills at prepare() and never again: tile_pos,
    //     slot_range / range_slot, the 8-block work list (d_tp_* here; d_tp_rec, the tiled form's one record
    //     per block and lane, where the exhaustive route has its slot words).  Small: 4 bytes per tile row, slot
    //     and range, 16 per record.
    //   shared, rebuilt by whichever search runs — everything a run derives from the frame: the tile fragments
    //     and constants (d_m_dtiles, d_m_dconst), the guards, the tile-order pool copy (d_dft_tpool), the range
    //     fragments, constants and orbit copies (d_m_rfrags, d_m_rconst, d_dft_rorb).  dft_prep
    //     writes every row of each, padding rows included, from its own maps (the exhaustive route needs that
    //     frame after frame anyway), so a fallback reads nothing the abandoned attempt laid out.  The pool and
    //     −ΣD4² are indexed by pool position in both layouts (the tiled form writes them in tp_keys, before its
    //     sort, and reads the rows back by tile; d_tp_rpix, the ranges' pixels in range order, is its own).
    FRAC_HIP(c, c->d_tp_slot_range.ensure(nbk * 32));
    FRAC_HIP(c, c->d_tp_range_slot.ensure(nr));
    FRAC_HIP(c, c->d_tp_tile_pos.ensure(nt * 32));
    FRAC_HIP(c, c->d_m_dtiles.ensure(nt * kDftKS * 64));
    FRAC_HIP(c, c->d_m_dconst.ensure((size_t)nt * kDftCS * 4 + 256)); // Fourier layout + one DMA piece of slack
    FRAC_HIP(c, c->d_m_rfrags.ensure(nbk * kDftNBF * 64));
    FRAC_HIP(c, c->d_m_rconst.ensure(nbk * 32));
    FRAC_HIP(c, c->d_dft_tguard.ensure(nt));
    FRAC_HIP(c, c->d_dft_trmax.ensure(nt + 4)); // + 4: a chunk's thresholds are one scalar load (tp_seed_windows)
    FRAC_HIP(c, c->d_tp_order.ensure(ng));
    FRAC_HIP(c, c->d_dft_tpool.ensure(nt * 32 * 32));
    FRAC_HIP(c, c->d_dft_rguard.ensure(nbk));
    FRAC_HIP(c, c->d_tp_work.ensure(ng));
    FRAC_HIP(c, c->d_tp_rec.ensure(nbk * 64));
    FRAC_HIP(c, c->d_tp_sevals.ensure(ng));
    FRAC_HIP(c, c->d_tp_tile_sd.ensure(nt));
    FRAC_HIP(c, c->d_tp_rpix.ensure(nr * 64));
    FRAC_HIP(c, c->d_tp_blk_sr.ensure(nbk));
    FRAC_HIP(c, c->d_tp_blk_u.ensure(nbk));
    FRAC_HIP(c, c->h_tp_tot.ensure());
    FRAC_HIP(c, c->d_tp_sort_table.ensure(tp_sort_table_words(P, nr)));
    FRAC_HIP(c, c->d_tp_pairs.ensure(ng));
    FRAC_HIP(c, c->d_tp_evals.ensure(ng));
    FRAC_HIP(c, c->d_tp_rbk.ensure(nr));
    FRAC_TRY(upload(c, c->d_tp_groups, c->tp_groups));
    FRAC_TRY(upload(c, c->d_tp_blk_group, c->tp_blk_group));
    if (nr)
        FRAC_HIP(c, hipMemcpyAsync(c->d_tp_rbk.ptr, c->d_rkey.ptr, nr * sizeof(int32_t), hipMemcpyDeviceToDevice,
                                   c->stream));
    return FRAC_OK;
}

// the MFMA engine's buffers, maps and work lists
int fill_mfma(frac_ctx* c)
{
    const int n = c->n;
    const size_t nr = nranges(c);
    const int KS = (n * n + 15) / 16;
    // (T = 8 Fourier: the flipped copies' slots map to the same ranges, second half)
    FRAC_HIP(c, c->d_m_slot_range.ensure((size_t)c->nblocks * 32 * c->dft_copies));
    FRAC_HIP(c, c->d_m_range_slot.ensure(nr));
    FRAC_HIP(c, c->d_m_tile_pos.ensure((size_t)c->ntiles * 32));
    FRAC_HIP(c, c->d_m_rconst.ensure((size_t)c->nblocks * 32 * c->dft_copies));
    // the direct form's [tile][8] uint4 and the Fourier form's [tile][kDftCS] (+ one LDS-DMA piece of slack)
    FRAC_HIP(c, c->d_m_dconst.ensure((size_t)c->ntiles * kDftCS * 4 + 256));
    FRAC_HIP(c, c->d_m_dtiles.ensure((size_t)c->ntiles * KS * 64));
    FRAC_HIP(c, c->d_m_rfrags.ensure((size_t)c->nblocks * std::max(c->Teff * KS, 6u * c->dft_copies) * 64));
    FRAC_HIP(c, c->d_m_entries.ensure(c->m_work.size() * 4 * c->Teff * 64)); // the direct form's (search_dft: none)
    if (c->m8_built) // n = 8, T = 4 or 8 (search_dft); may have no work
        FRAC_TRY(upload(c, c->d_m8_work, c->m8_work));
    if (c->nblocks) {
        fill_range_slots<<<(c->nblocks * 32 + 255) / 256, 256, 0, c->stream>>>(
            c->mlayout, c->d_rord.ptr, c->nblocks * 32, c->d_m_slot_range.ptr, c->d_m_range_slot.ptr);
        if (c->dft_copies == 2)
            FRAC_HIP(c, hipMemcpyAsync(c->d_m_slot_range.ptr + (size_t)c->nblocks * 32, c->d_m_slot_range.ptr,
                                       (size_t)c->nblocks * 32 * sizeof(int32_t), hipMemcpyDeviceToDevice,
                                       c->stream));
    }
    if (c->ntiles)
        fill_tile_pos<<<(c->ntiles * 32 + 255) / 256, 256, 0, c->stream>>>(c->mlayout, c->ntiles * 32,
                                                                          c->d_m_tile_pos.ptr);
    FRAC_TRY(upload(c, c->d_m_work, c->m_work));
    FRAC_TRY(upload(c, c->d_m_blk_ptr, c->m_blk_ptr));
    FRAC_TRY(upload(c, c->d_m_blk_ent, c->m_blk_ent));
    return FRAC_OK;
}

int prepare(frac_ctx* c)
{
    HostTrace tr("prepare");
    FRAC_TRY(prepare_geometry(c));
    tr.mark("validate");
    PrepBuckets B;
    FRAC_TRY(prepare_buckets(c, B, tr));
    plan_valu_work(c, B);
    tr.mark("buckets + valu work");
    select_engine(c, B);
    if (c->tp || c->auto_prune)
        FRAC_TRY(plan_tp_groups(c, B)); // (blocks and tiles per bucket as plan_mfma_work counts them)
    // AUTO prunes from kAutoPruneMinPairs block × tile pairs up (FRAC_FLAG_PRUNE: whenever there is a pair)
    if (c->auto_prune)
        c->auto_prune = c->tp_full_pairs >= ((c->p.flags & FRAC_FLAG_PRUNE) ? 1ull : kAutoPruneMinPairs);
    c->dft_copies = 1;
    if (c->engine == FRAC_ENGINE_MFMA)
        FRAC_TRY(plan_mfma_work(c, B));
    tr.mark("engine work");
    FRAC_TRY(fill_common(c, B));
    if (c->engine == FRAC_ENGINE_SEA || c->auto_prune)
        FRAC_TRY(fill_sea(c, B));
    if (c->tp || c->auto_prune)
        FRAC_TRY(fill_tp(c, B));
    if (c->engine == FRAC_ENGINE_MFMA)
        FRAC_TRY(fill_mfma(c));
    c->h_aux.resize(nranges(c));
    c->dirty = false;
    tr.mark("uploads");
    return FRAC_OK;
}

} // namespace
