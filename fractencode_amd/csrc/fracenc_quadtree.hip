// fracenc_quadtree.hip — quadtree frames: the levels planned on the device (qt_encode_dev, MFMA engine)
// or by prepare() per level (the other engines and the tuning knobs).  Included by fracenc_api.hip.
namespace {

// every level's domain grid (geometry only) stays on the host and the device across frames: the
// level swaps them in (no copy, no upload, no re-validation) and back out afterwards
// the caller's domain-list state comes back afterwards; the range list is consumed (cleared, unset)
struct LevelGrid {
    frac_ctx* c;
    bool doms_set_before;
    int lv = -1;
    void in(int level)
    {
        lv = level;
        std::swap(c->doms, c->qt_doms[lv]);
        std::swap(c->d_doms, c->qt_ddoms[lv]);
        c->doms_set = true;
        c->doms_uploaded = c->qt_dvalid[lv];
        c->doms_trusted = true;
        c->dirty = true;
    }
    void out()
    {
        if (lv < 0)
            return;
        c->qt_dvalid[lv] = c->doms_uploaded;
        std::swap(c->doms, c->qt_doms[lv]);
        std::swap(c->d_doms, c->qt_ddoms[lv]);
        c->doms_uploaded = false;
        c->doms_trusted = false;
        c->dirty = true;
        lv = -1;
    }
    ~LevelGrid()
    {
        out();
        c->ranges_dev = false;
        c->doms_set = doms_set_before;
        c->ranges_set = false;
    }
};

// the cached level grids belong to one frame size: another size starts them afresh
void qt_grids_for(frac_ctx* c, uint32_t W, uint32_t H)
{
    if (c->qt_w == W && c->qt_h == H)
        return;
    for (auto& g : c->qt_doms)
        g.clear();
    for (auto& v : c->qt_dvalid)
        v = false;
    c->qt_w = W;
    c->qt_h = H;
}

// A host-planned level's statistics (after its frac_run, before level.out()): the counters accumulate on the
// device in d_qt_stats (no per-level download or host loop), the rest is the host's
void qt_host_level_stats(frac_ctx* c, uint32_t nr, frac_stats& total)
{
    QtBuckets qb{};
    qb.nb = (uint32_t)c->bucket_begin.size();
    for (uint32_t b = 0; b < qb.nb && b < (uint32_t)kMaxBuckets; ++b) {
        qb.beg[b] = c->bucket_begin[b];
        qb.end[b] = c->bucket_end[b];
    }
    const bool sea_ran = c->engine_ran == FRAC_ENGINE_SEA && c->form_ran == FRAC_FORM_SEA;
    qt_level_stats<<<(nr + 255) / 256, 256, 0, c->stream>>>(
        c->d_aux.ptr, c->d_rkey.ptr, c->d_porig.ptr, nr, (uint64_t)c->doms.size(), c->p.use_classifier ? 1 : 0, qb,
        sea_ran ? c->d_sea_count.ptr : nullptr, c->d_qt_stats.ptr);
    total.total_mappings += (uint64_t)c->doms.size() * nr;
    total.engine = c->engine_ran;
    total.search_form = c->form_ran;
    total.matrix_flops += c->flops_ran;
    if (!sea_ran)
        total.evaluated_mappings += c->evaluated_ran;
}

// the host-planned levels' counters, read once after the last level
int qt_host_read_stats(frac_ctx* c, frac_stats& total)
{
    unsigned long long acc[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
    FRAC_HIP(c, hipMemcpy(acc, c->d_qt_stats.ptr, sizeof(acc), hipMemcpyDeviceToHost));
    total.rejected_mappings = acc[0];
    total.hit_ranges = acc[1];
    total.fallback_ranges = acc[2];
    total.empty_ranges = acc[3];
    total.evaluated_mappings += acc[4];
    return FRAC_OK;
}

// Whether a quadtree frame runs device-planned (qt_encode_dev): the MFMA engine at every level (AUTO
// or MFMA requested; the VALU and SEA engines keep the host-planned levels below), and no level in
// the all-fallback regime (a threshold that can be met in the inexact regime).
bool qt_device_planned(const frac_ctx* c, const frac_quadtree_params* qp)
{
    if (c->p.engine != FRAC_ENGINE_AUTO && c->p.engine != FRAC_ENGINE_MFMA)
        return false;
    // the planner hard-codes the shipped layouts (8-wave Fourier work items, the default direct variants):
    // a tuning build with an A/B knob set runs the host-planned levels, which honour it
    if (kTuningBuild)
        for (const char* k : kAbKnobs) {
            const char* v = getenv(k);
            if (v && *v)
                return false;
        }
    for (uint32_t n = qp->max_size; n >= qp->min_size; n /= 2)
        if (compute_hit_limit(c->p.rms_threshold, 4 * n * n) >= kExactLimit)
            return false;
    return true;
}

// A quadtree frame with every level laid out on the device (fracenc_bucket.hip qt_plan): per level the
// domain and range bucket keys, sorts and bounds, the planner (layout, work lists, CSR map, counts
// into the level's DevPlan), qt_fill_maps, the level's search (launch_all in plan mode: worst-case
// grids whose surplus workgroups leave at once) and the level transition (qt_flags, scan, qt_scatter,
// which writes the next level's count into the next DevPlan).  Nothing comes back to the host until
// the frame is done: one synchronisation for the leaf count and the counters, one for the leaves —
// where the host-planned path synchronised twice per level (bucket counts, split count).  Records,
// leaves and counters are those of the host-planned path.
// the frame's counters (qt_level_stats, qt_plan): {rejected, hit, fallback, empty, -, total, eligible,
// flops, overflow} in kQtShards copies, summed by the host
constexpr uint32_t kQtShards = 32, kQtCounters = 9;

int qt_encode_dev(frac_ctx* c, const frac_quadtree_params* qp, LevelGrid& level, frac_encode_item* out, size_t cap,
                  size_t* n_out, frac_stats* stats, frac_qt_leaf* out32 = nullptr, bool keep32 = false)
{
    // keep32 (frac_encode_quadtree_stream): 32-byte leaves into d_qt_leaves32 and no further
    const bool want32 = out32 || keep32;
    const uint32_t W = c->src.w, H = c->src.h, T = c->p.transforms;
    const int nb = c->p.use_classifier ? 7 : 1;
    const bool timing = (c->p.flags & FRAC_FLAG_TIMING) != 0;
    const auto [tplane, tstride] = target_plane(c);
    HostTrace tr("quadtree (device-planned)");
    const size_t max_leaves = (size_t)(W / qp->min_size) * (H / qp->min_size);
    constexpr uint32_t kFirst = 2 * (kMaxBuckets + 1); // bucket bounds per level: domains, ranges
    if (want32)
        FRAC_HIP(c, c->d_qt_leaves32.ensure(max_leaves));
    else
        FRAC_HIP(c, c->d_qt_leaves.ensure(max_leaves));
    FRAC_HIP(c, c->d_ranges.ensure(max_leaves));
    FRAC_HIP(c, c->d_qt_next.ensure(max_leaves));
    FRAC_HIP(c, c->d_qt_plan.ensure(6));
    FRAC_HIP(c, c->d_qt_first.ensure(5 * kFirst));
    FRAC_HIP(c, c->d_qt_stats.ensure(kQtShards * kQtCounters));
    FRAC_HIP(c, c->d_bk_first.ensure(2 * (kMaxBuckets + 1) + 1));
    // the classifier keys of every level from the frame's block sums, summed once here (domains 2n ≤ 32 rows)
    BlockSums bs_src, bs_tgt;
    const bool use_bs = nb > 1 && qp->max_size <= 16;
    if (use_bs)
        FRAC_TRY(plane_block_sums(c, bs_src, bs_tgt));
    // the first level's ranges: createUniformGrid(W, H, max, max), generated on the device
    const uint32_t m0 = qp->max_size;
    const uint32_t nr0 = W >= m0 && H >= m0 ? ((W - m0) / m0 + 1) * ((H - m0) / m0 + 1) : 0u;
    // (the same launch zeroes the frame's counters)
    constexpr uint32_t kQtZero = kQtShards * kQtCounters;
    qt_uniform_grid<<<(std::max(nr0, kQtZero) + 255) / 256, 256, 0, c->stream>>>(
        nr0 ? (W - qp->max_size) / qp->max_size + 1 : 1u, nr0, qp->max_size, qp->max_size, c->d_ranges.ptr,
        c->d_qt_stats.ptr, kQtZero);
    // the leaves go straight into the caller's buffer when it is pinned host memory the device can write
    // (the emit kernels write them over PCIe while the later levels run); else into d_qt_leaves and one
    // copy at the end
    frac_encode_item* leaves = c->d_qt_leaves.ptr;
    frac_qt_leaf* leaves32 = want32 ? c->d_qt_leaves32.ptr : nullptr;
    uint32_t leaf_cap = (uint32_t)std::min<size_t>(max_leaves, 0xffffffffu);
    bool direct = false;
    void* const host_out = out32 ? static_cast<void*>(out32) : static_cast<void*>(out);
    if (host_out && cap) {
        hipPointerAttribute_t at{};
        void* dp = nullptr;
        if (hipPointerGetAttributes(&at, host_out) == hipSuccess && at.type == hipMemoryTypeHost &&
            hipHostGetDevicePointer(&dp, host_out, 0) == hipSuccess && dp) {
            if (out32)
                leaves32 = reinterpret_cast<frac_qt_leaf*>(dp);
            else
                leaves = reinterpret_cast<frac_encode_item*>(dp);
            leaf_cap = (uint32_t)std::min<size_t>(cap, 0xffffffffu);
            direct = true;
        }
        (void)hipGetLastError(); // pageable memory is not an error
    }
    FRAC_HIP(c, c->h_qt_sum.ensure());
    uint32_t nr_bound = nr0; // the level's worst-case range count
    int lvi = 0;             // level index (plans 0..4; plan lvi + 1 receives the next count)
    std::vector<uint64_t> runs; // the levels' timing-history runs
    for (uint32_t n = qp->max_size; n >= qp->min_size && nr_bound; n /= 2, ++lvi) {
        const int lv = __builtin_ctz(n);
        if (c->qt_doms[lv].empty()) {
            c->qt_doms[lv].resize(frac_uniform_grid(W, H, 2 * n, n, nullptr, 0));
            if (!c->qt_doms[lv].empty())
                frac_uniform_grid(W, H, 2 * n, n, c->qt_doms[lv].data(), c->qt_doms[lv].size());
        }
        level.in(lv);
        const uint32_t nd = (uint32_t)c->doms.size(), nr_max = nr_bound;
        FRAC_HIP(c, c->d_doms.ensure(nd));
        if (!c->doms_uploaded && nd) {
            FRAC_HIP(c, hipMemcpyAsync(c->d_doms.ptr, c->doms.data(), nd * sizeof(frac_grid_item),
                                       hipMemcpyHostToDevice, c->stream));
            c->doms_uploaded = true;
        }
        // the level's geometry (prepare()'s fields for a ratio-2 square level on the MFMA engine)
        c->n = (int)n;
        c->S = c->Sw = c->Sh = 2 * n;
        c->nw = c->nh = n;
        c->virt = c->generic = false;
        c->Teff = T;
        c->K2 = n * n / 2;
        c->G = n == 16 ? 1u : (n <= 4 ? T : 4u);
        c->NG = T / c->G;
        c->npos = nd;
        c->engine = FRAC_ENGINE_MFMA;
        c->tp = false;
        c->auto_prune = false; // a planned level stays on the exhaustive route
        c->hitH = compute_hit_limit(c->p.rms_threshold, 4 * n * n);
        c->all_fallback = false;
        const bool fourier = n == 8 && mfma_dft_enabled(c);
        c->dft_copies = fourier && T == 8 ? 2u : 1u;
        const uint32_t cp = c->dft_copies, KS = (n * n + 15) / 16;
        const uint32_t bpw = n == 16 ? mfma16_bpw(T) : fourier ? kDftBlocksPerWG : 4u;
        const uint32_t target = n == 16 ? kMfma16TargetWgs : fourier ? 8192u / kDftBlocksPerWG * 4u : 8192u;
        const uint32_t nblocks_cap = (nr_max + 31) / 32 + (uint32_t)nb;
        const uint32_t ntiles_cap = (nd + 31) / 32 + (uint32_t)nb;
        const uint32_t groups_cap = (nblocks_cap * cp + bpw - 1) / bpw + (uint32_t)nb * cp;
        const uint32_t nwork_cap = target + groups_cap, nent_cap = bpw * nwork_cap;
        // buffers at the level's bounds (kept across frames: ensure() reallocates only to grow)
        const size_t mx = std::max<size_t>(std::max<size_t>(nd, nr_max), 1);
        FRAC_HIP(c, c->d_porig.ensure(nd));
        FRAC_HIP(c, c->d_pool.ensure((size_t)std::max<uint32_t>(nd, 1) * c->K2));
        FRAC_HIP(c, c->d_negsd2.ensure(nd));
        for (auto* b : {&c->d_rord, &c->d_rkey, &c->d_fb_list, &c->d_m_range_slot, &c->d_qt_flags, &c->d_qt_offs})
            FRAC_HIP(c, b->ensure(nr_max));
        FRAC_HIP(c, c->d_rbucket.ensure(nr_max));
        FRAC_HIP(c, c->d_best_key.ensure(nr_max));
        FRAC_HIP(c, c->d_out.ensure(nr_max));
        FRAC_HIP(c, c->d_aux.ensure(nr_max));
        FRAC_HIP(c, c->d_fb_count.ensure(1));
        FRAC_HIP(c, c->d_bk_keys.ensure(mx));
        FRAC_HIP(c, c->d_m_slot_range.ensure((size_t)nblocks_cap * 32 * cp));
        FRAC_HIP(c, c->d_m_rconst.ensure((size_t)nblocks_cap * 32 * cp));
        FRAC_HIP(c, c->d_m_tile_pos.ensure((size_t)ntiles_cap * 32));
        FRAC_HIP(c, c->d_m_dconst.ensure((size_t)ntiles_cap * kDftCS * 4 + 256));
        FRAC_HIP(c, c->d_m_dtiles.ensure((size_t)ntiles_cap * std::max(KS, 5u) * 64));
        FRAC_HIP(c, c->d_m_rfrags.ensure((size_t)nblocks_cap * std::max(T * KS, 6u * cp) * 64));
        DBuf<uint4>& dwork = fourier ? c->d_m8_work : c->d_m_work;
        FRAC_HIP(c, dwork.ensure(nwork_cap));
        if (!fourier) { // the direct form's entries and their CSR map (the Fourier search merges per slot: none)
            FRAC_HIP(c, c->d_m_blk_ptr.ensure((size_t)nblocks_cap * cp + 1));
            FRAC_HIP(c, c->d_m_blk_ent.ensure(nent_cap));
            FRAC_HIP(c, c->d_m_entries.ensure((size_t)nwork_cap * 4u * T * 64));
        }
        FRAC_HIP(c, c->d_bk_cnt.ensure(((size_t)(nd + kBkTile - 1) / kBkTile + (nr_max + kBkTile - 1) / kBkTile + 2) *
                                       kMaxBuckets));
        tr.mark("level buffers");
        DevPlan* plan = c->d_qt_plan.ptr + lvi;
        const uint32_t* dn = lvi ? &plan->nr : nullptr; // the first level's count is the host's
        uint32_t* first = c->d_qt_first.ptr + (size_t)lv * kFirst;
        if (nb > 1) {
            // domains: keys + stable bucket sort (the pool order porig) + bounds; ranges: the same over the
            // worst case, counting only the level's *dn (the grids' categories are −1, computed here:
            // no invalid category can occur, so no error word)
            const KeySeg kd{c->d_doms.ptr, nd, c->d_src.ptr, c->d_sstride, c->d_bk_keys.ptr, nullptr, nullptr, nullptr};
            const KeySeg kr{c->d_ranges.ptr, nr_max, tplane, tstride, c->d_rkey.ptr, nullptr, nullptr, dn};
            if (use_bs) // the frame's block sums, summed once before the first level
                launch_bucket_keys_bs(kd, bs_src, 2 * n, 2 * n, kr, bs_tgt, n, n, c->stream);
            else
                launch_bucket_keys_pair(kd, 2 * n, kr, n, c->stream);
            // both sorts in one set of launches (the range counts after the domain counts in the scratch)
            const BkSeg sd = bk_seg_of(c->d_bk_keys.ptr, nd, nullptr, c->d_bk_cnt.ptr, first, c->d_porig.ptr);
            const BkSeg sr = bk_seg_of(c->d_rkey.ptr, nr_max, dn, c->d_bk_cnt.ptr + (size_t)sd.tiles * kMaxBuckets,
                                       first + kMaxBuckets + 1, c->d_rord.ptr);
            launch_bucket_sorts(sd, sr, c->stream);
        } else {
            if (nd)
                fill_iota<<<(nd + 255) / 256, 256, 0, c->stream>>>(c->d_porig.ptr, nd);
            fill_iota<<<(nr_max + 255) / 256, 256, 0, c->stream>>>(c->d_rord.ptr, nr_max);
            FRAC_HIP(c, hipMemsetAsync(c->d_rkey.ptr, 0, nr_max * sizeof(uint32_t), c->stream));
        }
        QtPlanArgs pa;
        pa.plan = plan;
        pa.dfirst = nb > 1 ? first : nullptr;
        pa.rfirst = nb > 1 ? first + kMaxBuckets + 1 : nullptr;
        pa.nb = (uint32_t)nb;
        pa.nd = nd;
        pa.nr_init = lvi ? ~0u : nr0;
        pa.bpw = bpw;
        pa.target = target;
        pa.copies = cp;
        pa.mfma_per_pair = fourier ? 6u : T * KS;
        pa.nwork_cap = nwork_cap;
        pa.nent_cap = nent_cap;
        pa.nblocks_cap = nblocks_cap;
        pa.ntiles_cap = ntiles_cap;
        pa.work = dwork.ptr;
        pa.blk_ptr = fourier ? nullptr : c->d_m_blk_ptr.ptr;
        pa.blk_ent = fourier ? nullptr : c->d_m_blk_ent.ptr;
        pa.acc = c->d_qt_stats.ptr;
        QtFillArgs& fa = pa.fill;
        fa.rord = c->d_rord.ptr;
        fa.rkey = c->d_rkey.ptr;
        fa.copies = cp;
        fa.nthreads = std::max(std::max(nblocks_cap * 32 * cp, ntiles_cap * 32), nr_max);
        fa.slot_range = c->d_m_slot_range.ptr;
        fa.range_slot = c->d_m_range_slot.ptr;
        fa.tile_pos = c->d_m_tile_pos.ptr;
        fa.rbucket = c->d_rbucket.ptr;
        fa.rconst = fourier ? nullptr : c->d_m_rconst.ptr;
        fa.best_key = c->d_best_key.ptr;
        fa.fb_count = c->d_fb_count.ptr;
        // the layout, work lists, the direct form's CSR map and per-item maps: one launch
        qt_plan<<<std::max(32u, (fa.nthreads + 255) / 256), 256, 0, c->stream>>>(pa);
        // the level's search, on the bounds: launch_all in plan mode
        c->m_work.clear();
        c->m8_work.clear();
        c->ranges_dev = true;
        c->nr_dev = nr_max;
        c->n_dev = n;
        c->ntiles = ntiles_cap;
        c->nblocks = nblocks_cap;
        c->qplan = plan;
        c->qp_nwork_cap = nwork_cap;
        const int rc = launch_all_n(c, n);
        c->qplan = nullptr;
        FRAC_TRY(rc);
        FRAC_TRY(settle_fallback(c)); // the level's records are complete before its transition reads them
        if (timing)
            runs.push_back(c->hist_runs - 1);
        tr.mark("level launch");
        level.out();
        // the level transition: split counts and counters, their prefix and the next count, leaves and quadrants
        QtSplitArgs sa;
        sa.out = c->d_out.ptr;
        sa.ranges = c->d_ranges.ptr;
        sa.plan = plan;
        sa.next = plan + 1;
        sa.nmax = nr_max;
        sa.can_split = n > qp->min_size ? 1 : 0;
        sa.split = qp->split_distance;
        sa.tcount = c->d_qt_flags.ptr;
        // (a second stream copying a level's leaves across PCIe while the next level ran measured slower: the
        // copy kernel's PCIe writes stalled the next level's bucket keys 11 → 71 µs)
        sa.leaves = leaves;
        sa.leaves32 = leaves32;
        sa.dcols = W >= 2 * n ? (W - 2 * n) / n + 1 : 0u;
        sa.leaf_cap = leaf_cap;
        sa.next_ranges = c->d_qt_next.ptr;
        sa.aux = c->d_aux.ptr;
        sa.rkey = c->d_rkey.ptr;
        sa.porig = c->d_porig.ptr;
        sa.nd = nd;
        sa.classifier = c->p.use_classifier ? 1 : 0;
        sa.acc = stats ? c->d_qt_stats.ptr : nullptr;
        sa.shards = kQtShards;
        sa.stride = kQtCounters;
        const uint32_t ntl = std::max<uint32_t>((nr_max + kBkTile - 1) / kBkTile, 1u);
        qt_split_count<<<ntl, kBkThreads, 0, c->stream>>>(sa);
        qt_split_emit<<<ntl, kBkThreads, 0, c->stream>>>(sa);
        std::swap(c->d_ranges, c->d_qt_next);
        // the next level: at most four quadrants per range, at most the full grid of its size (counted in
        // closed form: frac_uniform_grid's count loop took 0.2 ms of host time for the 2×2 grid at 2048²)
        auto grid_count = [&](uint32_t size) -> uint32_t {
            return W >= size && H >= size ? ((W - size) / size + 1) * ((H - size) / size + 1) : 0u;
        };
        nr_bound = n > qp->min_size ? std::min<uint32_t>(4 * nr_max, grid_count(n / 2)) : 0u;
        tr.mark("split (device)");
    }
    c->ranges_dev = false;
    c->ranges.clear();
    c->ranges_set = false;
    c->dirty = true;
    c->ran = false;
    // the frame's one round trip: qt_finish writes the leaf count and the summed counters into pinned
    // memory (the leaves are already in the caller's buffer when it is pinned)
    void* dsum = nullptr;
    FRAC_HIP(c, hipHostGetDevicePointer(&dsum, c->h_qt_sum.ptr, 0));
    qt_finish<<<1, 64, 0, c->stream>>>(c->d_qt_plan.ptr + lvi, lvi ? 1 : 0, c->d_qt_stats.ptr, kQtShards, kQtCounters,
                                       reinterpret_cast<QtFrameSum*>(dsum));
    FRAC_HIP(c, hipStreamSynchronize(c->stream));
    struct {
        unsigned long long acc[kQtCounters];
    } h{};
    for (uint32_t i = 0; i < kQtCounters; ++i)
        h.acc[i] = c->h_qt_sum->acc[i];
    if (h.acc[8])
        return c->fail(FRAC_E_STATE, "quadtree: a level's layout exceeded its planned bounds");
    const uint32_t n_leaves = c->h_qt_sum->leaves;
    *n_out = n_leaves;
    if (out && n_leaves && !direct)
        FRAC_HIP(c, hipMemcpy(out, c->d_qt_leaves.ptr, std::min<size_t>(cap, n_leaves) * sizeof(frac_encode_item),
                              hipMemcpyDeviceToHost));
    if (out32 && n_leaves && !direct)
        FRAC_HIP(c, hipMemcpy(out32, c->d_qt_leaves32.ptr, std::min<size_t>(cap, n_leaves) * sizeof(frac_qt_leaf),
                              hipMemcpyDeviceToHost));
    tr.mark("leaves D2H");
    if (stats) {
        frac_stats total{};
        total.rejected_mappings = h.acc[0];
        total.hit_ranges = (uint32_t)h.acc[1];
        total.fallback_ranges = (uint32_t)h.acc[2];
        total.empty_ranges = (uint32_t)h.acc[3];
        total.total_mappings = h.acc[5];
        total.evaluated_mappings = h.acc[6];
        total.matrix_flops = h.acc[7];
        total.engine = FRAC_ENGINE_MFMA;
        total.search_form = c->form_ran;
        if (timing)
            for (uint64_t r : runs)
                add_run_times(total, &c->hist[(size_t)(r % kHistRuns) * 4]);
        *stats = total;
    }
    return FRAC_OK;
}
} // namespace

extern "C" {

static int encode_quadtree_impl(frac_ctx* c, const frac_quadtree_params* qp, frac_encode_item* out,
                                frac_qt_leaf* out32, size_t cap, size_t* n_out, frac_stats* stats, bool keep32 = false);

int frac_encode_quadtree(frac_ctx* c, const frac_quadtree_params* qp, frac_encode_item* out, size_t cap,
                         size_t* n_out, frac_stats* stats)
{
    return encode_quadtree_impl(c, qp, out, nullptr, cap, n_out, stats);
}

// frac_encode_quadtree_leaves; keep32 (frac_encode_quadtree_stream, fracenc_frq1pack.hip): every leaf stays in
// d_qt_leaves32 on the device, out and cap are not used
static int encode_quadtree_leaves_checked(frac_ctx* c, const frac_quadtree_params* qp, frac_qt_leaf* out, size_t cap,
                                          size_t* n_out, frac_stats* stats, bool keep32)
{
    if (!c)
        return FRAC_E_INVALID;
    if (!qp || !n_out)
        return c->fail(FRAC_E_INVALID, "quadtree: params and n_out are required");
    if (!c->planes_set)
        return c->fail(FRAC_E_STATE, "quadtree: no frame set");
    const uint32_t W = c->src.w, H = c->src.h;
    if (W > 0xffffu || H > 0xffffu)
        return c->fail(FRAC_E_INVALID, "quadtree leaves: a frame side above 65535 does not fit the 16-bit origins");
    if (qp->min_size >= 2 && frac_uniform_grid(W, H, 2 * qp->min_size, qp->min_size, nullptr, 0) >= FRAC_QT_NO_DOMAIN)
        return c->fail(FRAC_E_INVALID, "quadtree leaves: the finest level has more domains than a 24-bit index holds");
    return encode_quadtree_impl(c, qp, nullptr, out, cap, n_out, stats, keep32);
}

int frac_encode_quadtree_leaves(frac_ctx* c, const frac_quadtree_params* qp, frac_qt_leaf* out, size_t cap,
                                size_t* n_out, frac_stats* stats)
{
    return encode_quadtree_leaves_checked(c, qp, out, cap, n_out, stats, false);
}

// frac_encode_quadtree (out: 64-byte records) and frac_encode_quadtree_leaves (out32: 32-byte leaves)
static int encode_quadtree_impl(frac_ctx* c, const frac_quadtree_params* qp, frac_encode_item* out,
                                frac_qt_leaf* out32, size_t cap, size_t* n_out, frac_stats* stats, bool keep32)
{
    if (!c)
        return FRAC_E_INVALID;
    c->rate.ready = false; // the levels reuse the run's buffers: a rate state (fracenc_qtrate.hip) ends here
    // the levels' runs write no tuples into a frac_run sink (it is sized for the context's own ranges)
    struct SinkAside {
        frac_ctx* c;
        frac_tuple* saved;
        ~SinkAside() { c->tuple_sink = saved; }
    } aside{c, c->tuple_sink};
    c->tuple_sink = nullptr;
    if (!qp || !n_out)
        return c->fail(FRAC_E_INVALID, "quadtree: params and n_out are required");
    auto valid = [](uint32_t v) { return v == 2 || v == 4 || v == 8 || v == 16; };
    if (!valid(qp->max_size) || !valid(qp->min_size) || qp->min_size > qp->max_size)
        return c->fail(FRAC_E_INVALID, "quadtree: sizes must be 2, 4, 8 or 16 with min_size <= max_size");
    if (!c->planes_set)
        return c->fail(FRAC_E_STATE, "quadtree: no frame set");
    // the device-planned path never enters frac_run, so it checks the A/B knobs itself (a product
    // build refuses them here as frac_run does)
    FRAC_TRY(check_ab_knobs(c));
    // every buffer below (ensure(), the pinned counters, the level launches) belongs to this context's
    // device, whatever device the calling thread has current
    FRAC_HIP(c, hipSetDevice(c->device));
    const uint32_t W = c->src.w, H = c->src.h;
    if (!c->same_plane && (c->tgt.w != W || c->tgt.h != H))
        return c->fail(FRAC_E_INVALID, "quadtree: source and target planes must have one size");
    auto grid = [&](uint32_t size, uint32_t off) {
        std::vector<frac_grid_item> g(frac_uniform_grid(W, H, size, off, nullptr, 0));
        if (!g.empty())
            frac_uniform_grid(W, H, size, off, g.data(), g.size());
        return g;
    };
    frac_stats total{};
    HostTrace tr("quadtree");
    qt_grids_for(c, W, H);
    if ((out32 || keep32) && !qt_device_planned(c, qp)) {
        // the host-planned levels (other engines, tuning knobs): the records, then packed here; keep32 uploads
        // the packed leaves into d_qt_leaves32, where the device-planned levels leave theirs
        if (keep32)
            cap = (size_t)(W / qp->min_size) * (H / qp->min_size);
        std::vector<frac_encode_item> rec(cap);
        FRAC_TRY(encode_quadtree_impl(c, qp, cap ? rec.data() : nullptr, nullptr, cap, n_out, stats));
        const size_t m = std::min(cap, *n_out);
        std::vector<frac_qt_leaf> up(keep32 ? m : 0);
        frac_qt_leaf* dst = keep32 ? up.data() : out32;
        for (size_t i = 0; i < m; ++i) {
            const uint32_t n = rec[i].w;
            dst[i] = qt_leaf_of(rec[i], W >= 2 * n ? (W - 2 * n) / n + 1 : 0u);
        }
        if (keep32) {
            FRAC_HIP(c, c->d_qt_leaves32.ensure(cap));
            if (m)
                FRAC_HIP(c, hipMemcpy(c->d_qt_leaves32.ptr, up.data(), m * sizeof(frac_qt_leaf), hipMemcpyHostToDevice));
        }
        return FRAC_OK;
    }
    LevelGrid level{c, c->doms_set};
    if (qt_device_planned(c, qp))
        return qt_encode_dev(c, qp, level, out, cap, n_out, stats, out32, keep32);
    // the host-planned levels start from the first level's grid (built here only: ≈40 µs of host time
    // before the device-planned frame's first launch)
    std::vector<frac_grid_item> pending = grid(qp->max_size, qp->max_size);
    // the level-to-level step runs on the device (qt_flags, scan, qt_scatter): each level's leaves are
    // appended to d_qt_leaves and its split ranges' quadrants become the next level's device range list;
    // the host reads one count per level and the leaves once at the end
    const size_t max_leaves = (size_t)(W / qp->min_size) * (H / qp->min_size);
    FRAC_HIP(c, c->d_qt_leaves.ensure(max_leaves));
    // the level range lists swap between d_ranges and d_qt_next: both at the worst-case size up front, so
    // no level (of this or a later frame) reallocates one (hipFree would also synchronise the device)
    FRAC_HIP(c, c->d_ranges.ensure(max_leaves));
    FRAC_HIP(c, c->d_qt_next.ensure(max_leaves));
    FRAC_HIP(c, c->d_qt_count.ensure(1));
    FRAC_HIP(c, c->d_qt_stats.ensure(5));
    if (stats)
        FRAC_HIP(c, hipMemsetAsync(c->d_qt_stats.ptr, 0, 5 * sizeof(unsigned long long), c->stream));
    uint32_t n_leaves = 0;
    size_t level_nr = pending.size();
    FRAC_TRY(frac_set_ranges(c, pending.data(), pending.size()));
    for (uint32_t n = qp->max_size; level_nr && n >= qp->min_size; n /= 2) {
        const int lv = __builtin_ctz(n);
        if (c->qt_doms[lv].empty())
            c->qt_doms[lv] = grid(2 * n, n);
        level.in(lv);
        c->dirty = true;
        tr.mark("grids");
        FRAC_TRY(frac_run(c));
        FRAC_TRY(settle_fallback(c)); // the level's records are complete before qt_flags reads them
        tr.mark("run (enqueue)");
        // the level's statistics accumulate on the device (no per-level download or host loop); the
        // counters are read once after the last level, the event times after this level's count
        const uint32_t nr = (uint32_t)level_nr;
        if (stats)
            qt_host_level_stats(c, nr, total);
        level.out();
        tr.mark("level stats (enqueue)");
        FRAC_HIP(c, c->d_qt_flags.ensure(nr));
        FRAC_HIP(c, c->d_qt_offs.ensure(nr));
        size_t need = 0;
        FRAC_HIP(c, hipcub::DeviceScan::ExclusiveSum(nullptr, need, c->d_qt_flags.ptr, c->d_qt_offs.ptr, (int)nr,
                                                     c->stream));
        if (need > c->qt_tmp_bytes) {
            FRAC_HIP(c, c->d_qt_tmp.ensure(need));
            c->qt_tmp_bytes = need;
        }
        qt_flags<<<(nr + 255) / 256, 256, 0, c->stream>>>(c->d_out.ptr, nr, n > qp->min_size ? 1 : 0,
                                                         qp->split_distance, c->d_qt_flags.ptr);
        size_t tb = c->qt_tmp_bytes;
        FRAC_HIP(c, hipcub::DeviceScan::ExclusiveSum(c->d_qt_tmp.ptr, tb, c->d_qt_flags.ptr, c->d_qt_offs.ptr, (int)nr,
                                                     c->stream));
        // d_qt_next holds max_leaves items already: the 4·nsplit quadrants tile part of the plane at
        // ≥ min_size each, and the last level (n == min_size) splits nothing
        qt_scatter<<<(nr + 255) / 256, 256, 0, c->stream>>>(c->d_out.ptr, c->d_ranges.ptr, nr, c->d_qt_flags.ptr,
                                                           c->d_qt_offs.ptr, c->d_qt_leaves.ptr, n_leaves,
                                                           c->d_qt_next.ptr, c->d_qt_count.ptr);
        uint32_t nsplit = 0;
        FRAC_HIP(c, hipMemcpyAsync(&nsplit, c->d_qt_count.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        FRAC_HIP(c, hipStreamSynchronize(c->stream));
        if (stats && (c->p.flags & FRAC_FLAG_TIMING)) // the level's run has completed
            add_run_times(total, last_events(c));
        n_leaves += nr - nsplit;
        level_nr = 4 * (size_t)nsplit;
        // the next level searches the device-built quadrants
        std::swap(c->d_ranges, c->d_qt_next);
        c->ranges_dev = true;
        c->nr_dev = (uint32_t)level_nr;
        c->n_dev = n / 2;
        c->ranges_set = true;
        c->ran = false;
        tr.mark("split (device)");
    }
    c->ranges_dev = false;
    c->ranges.clear();
    c->dirty = true;
    c->ran = false;
    *n_out = n_leaves;
    if (out && n_leaves)
        FRAC_HIP(c, hipMemcpy(out, c->d_qt_leaves.ptr, std::min<size_t>(cap, n_leaves) * sizeof(frac_encode_item),
                              hipMemcpyDeviceToHost));
    tr.mark("leaves D2H");
    if (stats) {
        FRAC_TRY(qt_host_read_stats(c, total));
        *stats = total;
    }
    return FRAC_OK;
}

} // extern "C"
