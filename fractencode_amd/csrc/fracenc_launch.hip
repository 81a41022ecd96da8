// fracenc_launch.hip — the launch paths of a prepared run: schedule variants, the MFMA (direct and
// Fourier), SEA (per-range and tiled), VALU and sampled forms, the fits and the fp32 fallback.
// Included by fracenc_api.hip.
namespace {

template <int N, int T, int VAR>
void launch_search_mfma_v(frac_ctx* c, const MfmaSearchArgs& a)
{
    c->mfma_var_ran = VAR; // the resolve reads the entry layout this launch writes (VAR 128: merged over t)
    // H = 0 (the default threshold): a hit is S16 = 0, the smallest possible error, so
    // the plain first-minimum search already finds the first hit
    if (c->hitH > 0)
        search_mfma<N, T, true, VAR><<<a.nwork, 256, 0, c->stream>>>(a);
    else
        search_mfma<N, T, false, VAR><<<a.nwork, 256, 0, c->stream>>>(a);
}

// FRAC_MFMA_VARIANT (A/B knob, read per run): schedule variant of the MFMA searches. Every
// value a product build accepts gives identical (exact) records; the ablations, which give
// wrong results by design, are accepted — and compiled — only by a -DFRAC_TUNING build.
// Any other value fails the run (FRAC_E_INVALID), so a stray variable cannot corrupt records.
//   search_mfma: 0..7 schedule bits, 32 s_setprio, 64 late constants, 96, 98, 128 / 130 (default)
//                the minimum over transforms first; 12 and 386; ablations 8, 16
//   search_dft:  default 35, the guarded six-MFMA form (kDftFastVar); 37 the same always carrying the tile mask;
//                21 the exact epilogue (kDftExactVar); ablations 240..243 of 35.  The direct form's values
//                select the default here (dft_variant, fracenc_plan.hip)
inline int mfma_variant(frac_ctx* c, int& var)
{
    const char* v = ab_knob("FRAC_MFMA_VARIANT");
    var = kDefaultMfmaVariant;
    if (!v || !*v)
        return FRAC_OK;
    char* end = nullptr;
    const long x = strtol(v, &end, 10);
    static const int exact[] = {0, 1, 2, 3, 4, 5, 6, 7, 12, 21, 32, 35, 37, 64, 96, 98, 128, 130, 386};
    static const int ablation[] = {8, 16, 240, 241, 242, 243};
    bool ok = end && *end == 0;
    bool known = false;
    for (int e : exact)
        known |= x == e;
    if (kTuningBuild)
        for (int e : ablation)
            known |= x == e;
    if (!ok || !known)
        return c->fail(FRAC_E_INVALID, std::string("FRAC_MFMA_VARIANT=") + v +
                                           (kTuningBuild ? " is unknown" : " is not a product variant (ablations need "
                                                                           "a -DFRAC_TUNING build)"));
    var = (int)x;
    return FRAC_OK;
}

// the direct form's schedule variant for range side N: the shipped one (the float-C epilogue for
// n ≤ 4, where it is exact), or in a tuning build FRAC_MFMA_VARIANT (386 falls back to 130 above n = 4)
template <int N>
int direct_variant(frac_ctx* c, int& var)
{
    FRAC_TRY(mfma_variant(c, var));
    const bool knob = kTuningBuild && ab_knob("FRAC_MFMA_VARIANT") && *ab_knob("FRAC_MFMA_VARIANT");
    if (!knob)
        var = N <= 4 ? kDefaultMfmaVariant4 : kDefaultMfmaVariant;
    if (N > 4 && (var & 256))
        var = kDefaultMfmaVariant;
    return FRAC_OK;
}

template <int N, int T>
int launch_search_mfma(frac_ctx* c, const MfmaSearchArgs& a)
{
    int var = 0;
    FRAC_TRY(direct_variant<N>(c, var));
#ifndef FRAC_TUNING
    (void)var; // the product build: the shipped schedule only
    launch_search_mfma_v<N, T, (N <= 4 ? kDefaultMfmaVariant4 : kDefaultMfmaVariant)>(c, a);
#else
    switch (var) {
    case 0: launch_search_mfma_v<N, T, 0>(c, a); break;
    case 1: launch_search_mfma_v<N, T, 1>(c, a); break;
    case 2: launch_search_mfma_v<N, T, 2>(c, a); break;
    case 3: launch_search_mfma_v<N, T, 3>(c, a); break;
    case 4: launch_search_mfma_v<N, T, 4>(c, a); break;
    case 5: launch_search_mfma_v<N, T, 5>(c, a); break;
    case 6: launch_search_mfma_v<N, T, 6>(c, a); break;
    case 7: launch_search_mfma_v<N, T, 7>(c, a); break;
    case 32: launch_search_mfma_v<N, T, 32>(c, a); break; // s_setprio around MFMA clusters
    case 64: launch_search_mfma_v<N, T, 64>(c, a); break; // late epilogue-constant reads
    case 96: launch_search_mfma_v<N, T, 96>(c, a); break;
    case 98: launch_search_mfma_v<N, T, 98>(c, a); break;
    case 128: launch_search_mfma_v<N, T, 128>(c, a); break; // minimum over transforms first
    case 130: launch_search_mfma_v<N, T, 130>(c, a); break;
    case 8: launch_search_mfma_v<N, T, 8>(c, a); break;   // ablation: 1-value epilogue
    case 16: launch_search_mfma_v<N, T, 16>(c, a); break; // ablation: no MFMA
    case 386:
        if constexpr (N <= 4) {
            launch_search_mfma_v<N, T, 386>(c, a); // the float-C epilogue
            break;
        }
        [[fallthrough]];
    default: launch_search_mfma_v<N, T, kDefaultMfmaVariant>(c, a); break;
    }
#endif
    return FRAC_OK;
}

// FRAC_FLAG_DIRECT_FORM (and, in a tuning build, FRAC_MFMA_DFT=0): the direct MFMA search for
// ratio-2 n = 8 instead of the rotation-group Fourier form (fracenc_dft.hip)
inline bool mfma_dft_enabled(const frac_ctx* c)
{
    if (c->p.flags & FRAC_FLAG_DIRECT_FORM)
        return false;
    const char* v = ab_knob("FRAC_MFMA_DFT");
    return v ? atoi(v) != 0 : true;
}

// whether launch_mfma<8> takes the Fourier path (launch_dft); launch_all leaves the run's
// best_key / fb_count resets to it then
inline bool dft_route(const frac_ctx* c)
{
    return (c->Teff == 4 || c->dft_copies == 2) && !c->virt && mfma_dft_enabled(c);
}

// The fit kernels' arguments for the current run (also carried by resolve_dft when it fuses the fit)
inline FitArgs fit_args(const frac_ctx* c, const uint8_t* dtgt, uint32_t tstride, uint32_t nr)
{
    FitArgs f;
    f.tgt = dtgt;
    f.tstride = tstride;
    f.ranges = c->d_ranges.ptr;
    f.doms = c->d_doms.ptr;
    f.porig = c->d_porig.ptr;
    f.pool = c->d_pool.ptr;
    f.best_key = c->d_best_key.ptr;
    f.nr = nr;
    f.T = c->p.transforms;
    f.hitH = c->hitH;
    f.smax = c->p.s_max;
    f.all_fallback = 0;
    f.out = c->d_out.ptr;
    f.aux = c->d_aux.ptr;
    f.fb_count = c->d_fb_count.ptr;
    f.fb_list = c->d_fb_list.ptr;
    f.plan = c->qplan;
    return f;
}

// fallback_grid's scratch at the list's capacity: kKeyNone / 0 when (re)allocated, kept so by the kernel
inline int ensure_fb_scratch(frac_ctx* c)
{
    const size_t n = std::max<size_t>(c->d_fb_list.cap, 1);
    if (c->d_fb_key.cap >= n && c->d_fb_done.cap >= n && c->d_fb_key.ptr && c->d_fb_done.ptr)
        return FRAC_OK;
    FRAC_HIP(c, c->d_fb_key.ensure(n));
    FRAC_HIP(c, c->d_fb_done.ensure(n));
    FRAC_HIP(c, hipMemsetAsync(c->d_fb_key.ptr, 0xff, c->d_fb_key.cap * sizeof(unsigned long long), c->stream));
    FRAC_HIP(c, hipMemsetAsync(c->d_fb_done.ptr, 0, c->d_fb_done.cap * sizeof(uint32_t), c->stream));
    return FRAC_OK;
}

// the fp32 fallback's arguments for the current run (fallback_grid)
inline FallbackArgs fallback_args(frac_ctx* c, const uint8_t* dtgt, uint32_t tstride)
{
    FallbackArgs b;
    b.tgt = dtgt;
    b.tstride = tstride;
    b.ranges = c->d_ranges.ptr;
    b.doms = c->d_doms.ptr;
    b.porig = c->d_porig.ptr;
    b.pool = c->d_pool.ptr;
    b.rbucket = c->d_rbucket.ptr;
    b.fb_count = c->d_fb_count.ptr;
    b.fb_list = c->d_fb_list.ptr;
    b.T = c->p.transforms;
    b.thr = c->p.rms_threshold;
    b.smax = c->p.s_max;
    b.out = c->d_out.ptr;
    b.aux = c->d_aux.ptr;
    b.tuples = c->fit_fused && !c->qplan ? c->tuple_sink : nullptr; // the fused resolvers' sink, if any
    b.fb_key = c->d_fb_key.ptr;
    b.fb_done = c->d_fb_done.ptr;
    // jobs per listed range: the largest bucket's domains in chunks of kFbChunk (a planned level: every domain)
    size_t maxb = 0;
    for (size_t k = 0; k < c->bucket_begin.size() && k < c->bucket_end.size(); ++k)
        maxb = std::max<size_t>(maxb, c->bucket_end[k] - c->bucket_begin[k]);
    if (c->qplan || maxb == 0)
        maxb = c->doms.size();
    b.chunks = (uint32_t)std::max<size_t>((maxb + kFbChunk - 1) / kFbChunk, 1);
    return b;
}

template <int N>
void launch_fallback_grid(frac_ctx* c, const FallbackArgs& b)
{
    fallback_grid<N><<<kFallbackBlocks, 256, 0, c->stream>>>(b);
}

// The fused resolvers' listed fp32-regime ranges, settled before anything reads the run's records: one
// fallback_grid launch (an empty list costs its dispatch).  frac_fetch settles only when a range was listed.
inline int settle_fallback(frac_ctx* c)
{
    if (!c->fb_pending)
        return FRAC_OK;
    c->fb_pending = false;
    if (c->fb_n == 16)
        launch_fallback_grid<16>(c, c->fb_args);
    else
        launch_fallback_grid<8>(c, c->fb_args);
    FRAC_HIP(c, hipGetLastError());
    return FRAC_OK;
}

// work items a search launch covers: the host-built list, or a device-planned level's bound (its
// workgroups past DevPlan::nwork leave at once)
inline uint32_t launch_nwork(const frac_ctx* c, const std::vector<uint4>& w)
{
    return c->qplan ? c->qp_nwork_cap : (uint32_t)w.size();
}

// what every MFMA search reads and writes, over the given work list
inline MfmaSearchArgs search_args(const frac_ctx* c, const uint4* work, uint32_t nwork)
{
    MfmaSearchArgs a;
    a.dtiles = c->d_m_dtiles.ptr;
    a.dconst = reinterpret_cast<const uint4*>(c->d_m_dconst.ptr);
    a.rfrags = c->d_m_rfrags.ptr;
    a.rconst = c->d_m_rconst.ptr;
    a.work = work;
    a.nwork = nwork;
    a.hitH = (uint32_t)std::max<int64_t>(c->hitH, 0);
    a.entries = c->d_m_entries.ptr;
    a.plan = c->qplan;
    return a;
}

// what every MFMA resolve reads and writes, over the given CSR map
inline MfmaResolveArgs resolve_args(const frac_ctx* c, const uint8_t* dtgt, uint32_t tstride, uint32_t nr,
                                    const uint32_t* blk_ptr, const uint32_t* blk_ent)
{
    MfmaResolveArgs v;
    v.tgt = dtgt;
    v.tstride = tstride;
    v.ranges = c->d_ranges.ptr;
    v.range_slot = c->d_m_range_slot.ptr;
    v.blk_ptr = blk_ptr;
    v.blk_ent = blk_ent;
    v.entries = c->d_m_entries.ptr;
    v.rconst = c->d_m_rconst.ptr;
    v.tile_pos = c->d_m_tile_pos.ptr;
    v.ntiles = c->ntiles;
    v.pool = c->d_pool.ptr;
    v.negsd2 = c->d_negsd2.ptr;
    v.nr = nr;
    v.hitH = c->hitH;
    v.best_key = c->d_best_key.ptr;
    v.plan = c->qplan;
    return v;
}

// the fit in the resolving wave: the resolve carries the fit's arguments and, outside a planned level, the sink
inline void fuse_fit(frac_ctx* c, MfmaResolveArgs& v)
{
    v.fused_fit = 1;
    v.fit = fit_args(c, v.tgt, v.tstride, v.nr);
    v.fit.tuples = c->qplan ? nullptr : c->tuple_sink;
    c->fit_fused = true;
}

#ifdef FRAC_CLOCK_STAMP
// the diagnostic clock build (tools/build_tuning.py --stamps): search_dft stamps s_memtime and
// s_memrealtime around its loop, per workgroup, into this buffer; frac_clock_stamps reads the last
// launch's.  Never in the product or the plain tuning build.
static unsigned long long* g_stamps = nullptr;
static size_t g_stamps_cap = 0;
static unsigned g_stamps_n = 0;
static unsigned long long* clock_stamps_for(unsigned nwg)
{
    if (nwg > g_stamps_cap) {
        if (g_stamps)
            (void)hipFree(g_stamps);
        g_stamps = nullptr;
        g_stamps_cap = 0;
        if (hipMalloc(&g_stamps, (size_t)nwg * kClockStampWords * sizeof(unsigned long long)) != hipSuccess)
            return nullptr;
        g_stamps_cap = nwg;
    }
    g_stamps_n = nwg;
    return g_stamps;
}
// out: [cap_workgroups][kClockStampWords]
extern "C" int frac_clock_stamps(unsigned long long* out, size_t cap_workgroups)
{
    if (!g_stamps || !out)
        return -1;
    const size_t n = std::min<size_t>(g_stamps_n, cap_workgroups);
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(out, g_stamps, n * kClockStampWords * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    return (int)n;
}
#endif

// search_dft with or without the hit test (H = 0: a hit is S16 = 0, which the plain maximum search finds)
template <int VAR, bool CHUNKED = false, bool TMASK = false>
void launch_search_dft(frac_ctx* c, const DftArgs& da, unsigned nwg, bool hits)
{
    if (hits)
        search_dft<true, VAR, CHUNKED, TMASK><<<nwg, 64 * kDftBlocksPerWG, 0, c->stream>>>(da);
    else
        search_dft<false, VAR, CHUNKED, TMASK><<<nwg, 64 * kDftBlocksPerWG, 0, c->stream>>>(da);
}

// n = 8, T = 4: the C4-Fourier search (6 MFMAs per 32×32 tile pair instead of 16).  inits: reset
// best_key and fb_count in the preparation kernel (launch_all skipped its memsets).  mark_prep = false: the
// fallback of AUTO's pruned route, whose prep boundary launch_tp marked (this prep counts as search time)
inline int launch_dft(frac_ctx* c, const uint8_t* dtgt, uint32_t tstride, bool inits, bool mark_prep = true)
{
    const uint32_t nr = (uint32_t)nranges(c);
    MfmaDomainPrepArgs d;
    d.pool = c->d_pool.ptr;
    d.negsd2 = c->d_negsd2.ptr;
    d.tile_pos = c->d_m_tile_pos.ptr;
    d.ntiles = c->ntiles;
    d.dtiles = c->d_m_dtiles.ptr;
    d.dconst = c->d_m_dconst.ptr;
    d.plan = c->qplan;
    FRAC_HIP(c, c->d_dft_tguard.ensure(c->ntiles));
    FRAC_HIP(c, c->d_dft_trmax.ensure((size_t)c->ntiles + 4)); // + 4: a chunk's thresholds are one scalar load
    FRAC_HIP(c, c->d_dft_tpool.ensure((size_t)c->ntiles * 32 * 32));
    const uint32_t nbk = c->nblocks * c->dft_copies; // range blocks incl. T = 8's flipped copies
    FRAC_HIP(c, c->d_dft_rguard.ensure(nbk));
    int var = 0; // FRAC_MFMA_VARIANT for this path (A/B knob; dft_variant, fracenc_plan.hip)
    FRAC_TRY(mfma_variant(c, var));
    var = dft_variant(var);
    FRAC_HIP(c, c->d_m_dtiles.ensure((size_t)c->ntiles * kDftKS * 64));
    d.dtiles = c->d_m_dtiles.ptr;
    DftDomainBuildArgs b;
    b.src = c->d_src.ptr;
    b.sstride = c->d_sstride;
    b.doms = c->d_doms.ptr;
    b.porig = c->d_porig.ptr;
    b.pool = c->d_pool.ptr;
    b.negsd2 = c->d_negsd2.ptr;
    b.tpool = c->d_dft_tpool.ptr;
    MfmaRangePrepArgs r;
    r.tgt = dtgt;
    r.tstride = tstride;
    r.ranges = c->d_ranges.ptr;
    r.slot_range = c->d_m_slot_range.ptr;
    r.nblocks = nbk;
    r.T = 4;
    r.rfrags = c->d_m_rfrags.ptr;
    r.rconst = c->d_m_rconst.ptr;
    r.flip_from = c->dft_copies == 2 ? c->nblocks : ~0u;
    r.plan = c->qplan;
    FRAC_HIP(c, c->d_dft_rorb.ensure((size_t)r.nblocks * 32 * 32));
    r.rorb = c->d_dft_rorb.ptr;
    // the search merges its domain splits per slot (64-bit atomicMax; reset by the range prep), so the resolve
    // reads one word per slot: no per-work-item entries, no CSR map
    FRAC_HIP(c, c->d_dft_slotbest.ensure((size_t)r.nblocks * 32));
    r.slotbest = c->d_dft_slotbest.ptr;
    // one launch: domain tiles, range blocks and (inits) the run's resets
    DftPrepInit in;
    if (inits) {
        in.best_key = c->d_best_key.ptr;
        in.nr = nr;
        in.fb_count = c->d_fb_count.ptr;
        in.fbc = 0; // the Fourier path never runs with all_fallback
    }
    in.dblocks = (c->ntiles * 64 + 255) / 256; // two lanes per tile row (dft_domain_build_pair_at)
    in.plan = c->qplan;
    in.copies = c->dft_copies;
    const unsigned pg = in.dblocks + (nbk * 64 + 255) / 256; // two lanes per range slot (dft_range_prep_pair_at)
    if (pg || inits)
        dft_prep<<<std::max(pg, 1u), 256, 0, c->stream>>>(d, b, c->d_dft_tguard.ptr, c->d_dft_trmax.ptr, r,
                                                         c->d_dft_rguard.ptr, in);
    if ((c->p.flags & FRAC_FLAG_TIMING) && mark_prep)
        FRAC_TRY(mark_event(c, 1));
    const std::vector<uint4>& work = c->m8_work;
    c->form_ran = FRAC_FORM_FOURIER;
    c->flops_ran = 0;
    for (const uint4& w : work) // 6 MFMA 32x32x16 (32768 flops each) per (block, tile)
        c->flops_ran += (uint64_t)w.y * (w.w - w.z) * 6ull * 32768ull;
    const uint32_t nwork = launch_nwork(c, work);
    if (nwork) {
        DftArgs da;
        da.m = search_args(c, c->d_m8_work.ptr, nwork);
        da.m.entries = nullptr; // (the direct form's: search_dft merges per slot)
        da.rguard = c->d_dft_rguard.ptr;
        da.trmax = c->d_dft_trmax.ptr;
        da.slotbest = r.slotbest;
        const unsigned nwg = nwork;
#ifdef FRAC_CLOCK_STAMP
        da.stamps = clock_stamps_for(nwg);
#endif
        const bool hits = c->hitH > 0;
#ifndef FRAC_TUNING
        // the product build: the shipped form only (variant 35, kDftDefaultVariant) — the six-MFMA
        // form with the guarded constant-folded epilogue, the unrolled chunk and buffer_load … lds stages
        static_assert(kDftDefaultVariant == 35, "the product build's Fourier search is variant 35");
        // few tiles: the run is a short chain whose resolve weighs as much as its search, and the search also
        // carries the tiles of the winning chunk that attain its maximum (TMASK) so the resolve evaluates those
        if (c->ntiles <= kDftTmaskTiles)
            launch_search_dft<kDftFastVar, false, true>(c, da, nwg, hits);
        else
            launch_search_dft<kDftFastVar>(c, da, nwg, hits);
#else // the tuning build: the shipped form, its A/B partners and its ablations (wrong results by design)
        constexpr unsigned kThreads = 64 * kDftBlocksPerWG;
        switch (var) {
        case 37: launch_search_dft<kDftFastVar, false, true>(c, da, nwg, hits); break; // 35 carrying the tile mask
        case 21: launch_search_dft<kDftExactVar>(c, da, nwg, hits); break;              // the exact epilogue
        case 240: search_dft<false, kDftFastVar | 8><<<nwg, kThreads, 0, c->stream>>>(da); break;   // MFMAs, one-value epilogue
        case 241: search_dft<false, kDftFastVar | 16><<<nwg, kThreads, 0, c->stream>>>(da); break;  // the fast epilogue, no MFMA
        case 242: search_dft<false, kDftFastVar | 512><<<nwg, kThreads, 0, c->stream>>>(da); break; // no barrier
        case 243: search_dft<false, kDftFastVar | 64><<<nwg, kThreads, 0, c->stream>>>(da); break;  // no LDS-DMA / barrier
                                                                                                   // after the first stages
        default: launch_search_dft<kDftFastVar>(c, da, nwg, hits); break; // 35
        }
#endif
    }
    if (c->p.flags & FRAC_FLAG_TIMING)
        FRAC_TRY(mark_event(c, 2));
    if (nr) {
        MfmaResolveArgs v = resolve_args(c, dtgt, tstride, nr, nullptr, nullptr); // no CSR map, no entries
        v.entries = nullptr;
        v.T = c->dft_copies == 2 ? 8u : 4u;
        v.slot_range = c->d_m_slot_range.ptr;
        v.nslots = c->nblocks * 32u;
        v.flip_slots = c->dft_copies == 2 ? c->nblocks * 32u : 0u;
        v.tpool = c->d_dft_tpool.ptr;
        v.rorb = c->d_dft_rorb.ptr;
        v.slotbest = r.slotbest;
        FRAC_HIP(c, c->d_rstat.ensure(nr));
        v.rstat = c->d_rstat.ptr;
        fuse_fit(c, v); // (launch_all skips fit_rstat)
        // one-wave workgroups: a finished range frees its slot at once (0.254 vs 0.271 ms finish
        // against 4-wave workgroups, 30-sample A/B, profiles/r01/ab_fourier_variants.log); T = 8: two
        // waves, the slot and its flipped copy resolved at the same time
        v.paired = c->dft_copies == 2 ? 1 : 0;
        resolve_dft<false><<<std::max(1u, v.nslots), v.paired ? 128 : 64, 0, c->stream>>>(v);
    }
    return FRAC_OK;
}

template <int N>
int launch_mfma(frac_ctx* c, const uint8_t* dtgt, uint32_t tstride, bool inits = false)
{
    // T = the transforms per pool row: 1 in the sampled form (one row per domain and transform)
    const uint32_t nr = (uint32_t)nranges(c), T = c->Teff;
    if constexpr (N == 8) {
        if (dft_route(c))
            return launch_dft(c, dtgt, tstride, inits);
    }
    int dvar = 0;
    FRAC_TRY(direct_variant<N>(c, dvar));
    const int fmode = (dvar & 256) ? 1 : 0; // the float-C epilogue: its row constants and B scaling
    // n ≤ 4 with the transforms merged in the search (resolve_small): the search merges its work items per range
    // slot itself (one 64-bit atomicMax per slot and work item; reset by mfma_range_prep), so the resolve reads one
    // word per slot instead of walking the block's entries through the CSR map
    unsigned long long* slotbest = nullptr;
    if (N <= 4 && T >= 4 && (dvar & (128 | 256)) && c->nblocks) {
        FRAC_HIP(c, c->d_dft_slotbest.ensure((size_t)c->nblocks * 32));
        slotbest = c->d_dft_slotbest.ptr;
    }
    // the domain tiles and the range blocks' fragments in one launch (mfma_prep)
    MfmaDomainPrepArgs d;
    d.fmode = fmode;
    d.pool = c->d_pool.ptr;
    d.negsd2 = c->d_negsd2.ptr;
    d.tile_pos = c->d_m_tile_pos.ptr;
    d.ntiles = c->ntiles;
    d.dtiles = c->d_m_dtiles.ptr;
    d.dconst = c->d_m_dconst.ptr;
    d.plan = c->qplan;
    if ((N == 4 || N == 16) && !c->virt) { // the pool rows built here (launch_all skips pool_build)
        d.src = c->d_src.ptr;
        d.sstride = c->d_sstride;
        d.doms = c->d_doms.ptr;
        d.porig = c->d_porig.ptr;
        d.pool_out = c->d_pool.ptr;
        d.negsd2_out = c->d_negsd2.ptr;
    }
    MfmaRangePrepArgs r;
    r.tgt = dtgt;
    r.tstride = tstride;
    r.ranges = c->d_ranges.ptr;
    r.slot_range = c->d_m_slot_range.ptr;
    r.nblocks = c->nblocks;
    r.T = T;
    r.rfrags = c->d_m_rfrags.ptr;
    r.rconst = c->d_m_rconst.ptr;
    r.plan = c->qplan;
    r.fmode = fmode;
    r.slotbest = slotbest;
    // n = 16: 16 lanes per tile row and one workgroup per range block; else a thread per tile row and per
    // (block, transform, K-step, lane)
    const uint32_t dblocks = !c->ntiles ? 0u
                             : N == 16  ? (c->ntiles * 32 * MfmaGeom<16>::KS + 255) / 256
                                        : (c->ntiles * 32 + 255) / 256;
    const uint32_t rblocks = !c->nblocks ? 0u
                             : N == 16   ? c->nblocks
                                         : (uint32_t)(((size_t)c->nblocks * T * MfmaGeom<N>::KS * 64 + 255) / 256);
    // rconst is a sum of per-pixel terms, accumulated by the transform-0 threads (n < 16; a planned level's
    // qt_fill_maps zeroed it)
    if (N != 16 && c->nblocks && !c->qplan)
        FRAC_HIP(c, hipMemsetAsync(c->d_m_rconst.ptr, 0, (size_t)c->nblocks * 32 * sizeof(uint32_t), c->stream));
    if (dblocks + rblocks) {
        if constexpr (N == 16) {
            if (T == 8)
                mfma_prep<16, 8><<<dblocks + rblocks, 256, 0, c->stream>>>(d, r, dblocks);
            else if (T == 1)
                mfma_prep<16, 1><<<dblocks + rblocks, 256, 0, c->stream>>>(d, r, dblocks);
            else
                mfma_prep<16, 4><<<dblocks + rblocks, 256, 0, c->stream>>>(d, r, dblocks);
        } else {
            mfma_prep<N><<<dblocks + rblocks, 256, 0, c->stream>>>(d, r, dblocks);
        }
    }
    if (c->p.flags & FRAC_FLAG_TIMING)
        FRAC_TRY(mark_event(c, 1));
    c->form_ran = FRAC_FORM_DIRECT;
    c->flops_ran = 0;
    for (const uint4& w : c->m_work) // T·KS MFMA 32x32x16 per (range block, domain tile)
        c->flops_ran += (uint64_t)w.y * (w.w - w.z) * T * MfmaGeom<N>::KS * 32768ull;
    const uint32_t nwork = launch_nwork(c, c->m_work);
    if (nwork) {
        MfmaSearchArgs a = search_args(c, c->d_m_work.ptr, nwork);
        a.slotbest = slotbest;
        if constexpr (N == 16) { // 4-wave workgroups: mfma16_bpw(T) range blocks × their T transforms
            const unsigned nwg = nwork;
            const bool hits = c->hitH > 0;
            if (T == 8) {
                if (hits)
                    search_mfma16<8, true><<<nwg, 256, 0, c->stream>>>(a);
                else
                    search_mfma16<8, false><<<nwg, 256, 0, c->stream>>>(a);
            } else if (T == 1) {
                if (hits)
                    search_mfma16<1, true><<<nwg, 256, 0, c->stream>>>(a);
                else
                    search_mfma16<1, false><<<nwg, 256, 0, c->stream>>>(a);
            } else {
                if (hits)
                    search_mfma16<4, true><<<nwg, 256, 0, c->stream>>>(a);
                else
                    search_mfma16<4, false><<<nwg, 256, 0, c->stream>>>(a);
            }
        } else if (T == 8)
            FRAC_TRY((launch_search_mfma<N, 8>(c, a)));
        else if (T == 1)
            FRAC_TRY((launch_search_mfma<N, 1>(c, a)));
        else
            FRAC_TRY((launch_search_mfma<N, 4>(c, a)));
    }
    if (c->p.flags & FRAC_FLAG_TIMING)
        FRAC_TRY(mark_event(c, 2));
    if (nr) {
        MfmaResolveArgs v = resolve_args(c, dtgt, tstride, nr, c->d_m_blk_ptr.ptr, c->d_m_blk_ent.ptr);
        v.T = T;
        v.merged = (N != 16 && T > 1 && (c->mfma_var_ran & (128 | 256))) ? 1 : 0; // entries merged over t
        v.fmode = (N != 16 && (c->mfma_var_ran & 256)) ? 1 : 0;                  // fmap'd float-C minima
        v.slotbest = slotbest;
        if constexpr (N == 16)
            v.rfrags = c->d_m_rfrags.ptr; // the range copies from search_mfma16's B fragments
        if (!c->virt) // (the sampled form fits at its own points: gen_fit)
            fuse_fit(c, v);
        if constexpr (N <= 4) {
            if (T >= 4) // a pool row per lane, the transforms across lanes
                resolve_small<N><<<(nr + 3) / 4, 256, 0, c->stream>>>(v);
            else
                resolve_mfma<N><<<(nr + 3) / 4, 256, 0, c->stream>>>(v);
        } else {
            resolve_mfma<N><<<(nr + 3) / 4, 256, 0, c->stream>>>(v);
        }
    }
    return FRAC_OK;
}

// SEA engine, tiled form (fracenc_tp.hip): sorted tiles and blocks, per-range seed bounds,
// per-group windows, the Fourier search over the windows with one record per block and lane, resolve_dft.
// No buffer is sized from the windows (the records are nblocks·64, allocated at prepare()); one host
// synchronisation remains, for the run's totals: frac_stats' counts and the budget test.  (The windowed search
// queued before it, skipped on the device when over the budget, measured no gain: DESIGN §7.9.)
// The route is tp_keys (with the run's resets), the sort's three launches per key byte (tp_sort_count,
// tp_sort_offsets, tp_sort_scatter: six at 16-bit keys, nine with buckets), tp_build, tp_prep, the seed search_dft,
// tp_seed_windows, tp_plan (the totals), the synchronisation, search_dft and resolve_dft, all on one stream.
// budgeted (FRAC_ENGINE_AUTO's pruned route): when the windows hold more than kAutoPruneBudget of the run's
// block × tile pairs the attempt is abandoned before the windowed search is launched, and the exhaustive
// Fourier search (launch_dft) produces the records in the same run on the same stream.
int launch_tp(frac_ctx* c, const uint8_t* dtgt, uint32_t tstride, bool timing, bool budgeted = false)
{
    const uint32_t nr = (uint32_t)nranges(c), P = c->npos;
    const uint32_t nt = c->ntiles, nbk = c->nblocks, ng = (uint32_t)c->tp_groups.size();
    // resolve_dft<true> keeps one copy per slot: T = 8's flipped copies would go unmerged here, and
    // prepare() routes only T = 4 to the tiled form (c->tp)
    if (c->p.transforms != 4)
        return c->fail(FRAC_E_STATE, "the tiled SEA form runs T = 4 only");
    c->form_ran = FRAC_FORM_SEA_MFMA;
    c->flops_ran = 0;
    c->evaluated_ran = 0;
    // the pixel pass: the pool rows, −ΣD4² and the ranges' pixels (rpix) with both sides' sort keys, and the run's
    // best_key and fb_count resets (launch_all skipped its fills)
    if (P || nr) {
        TpKeyArgs k;
        k.src = c->d_src.ptr;
        k.sstride = c->d_sstride;
        k.doms = c->d_doms.ptr;
        k.porig = c->d_porig.ptr;
        k.P = P;
        k.bucket_end = c->d_sea_bend.ptr;
        k.nb = (uint32_t)c->bucket_end.size();
        k.dkey = c->d_sea_dkey.ptr;
        k.dpos = c->d_sea_dpos.ptr;
        k.pool = c->d_pool.ptr;
        k.negsd2 = c->d_negsd2.ptr;
        k.dblocks = (uint32_t)(((uint64_t)P * 2 + 255) / 256); // two lanes per pool position
        k.tgt = dtgt;
        k.tstride = tstride;
        k.ranges = c->d_ranges.ptr;
        k.rbucket_idx = c->d_tp_rbk.ptr;
        k.nr = nr;
        k.rkey = c->d_sea_rkey.ptr;
        k.rord = c->d_sea_rord.ptr;
        k.rpix = c->d_tp_rpix.ptr;
        k.best_key = c->d_best_key.ptr;
        k.fb_count = c->d_fb_count.ptr;
        // two lanes per range
        tp_keys<<<k.dblocks + (uint32_t)(((uint64_t)nr * 2 + 255) / 256), 256, 0, c->stream>>>(k);
    }
    // Both sides' sorts in the same launches (fracenc_tpsort.hip): stable, tp_key_bits / 8 passes of three small
    // kernels each on this stream, into the tables fill_tp sized.  An even number of passes leaves the sorted
    // pairs in the buffers tp_keys wrote, an odd one in their twins.
    FRAC_HIP(c, tp_sort_pairs(c->d_tp_sort_table.ptr,
                              TpSortBufs{c->d_sea_dkey.ptr, c->d_sea_dpos.ptr, c->d_sea_dkey2.ptr, c->d_sea_dpos2.ptr, P},
                              TpSortBufs{c->d_sea_rkey.ptr, c->d_sea_rord.ptr, c->d_sea_rkey2.ptr, c->d_sea_rord2.ptr, nr},
                              c->tp_key_bits, c->stream));
    const bool twin = tp_sort_in_second(c->tp_key_bits);
    // the tiles and the slots from the two sorted orders
    if (nt || nbk) {
        TpBuildArgs t;
        t.bk = c->tp_bk;
        t.skey = twin ? c->d_sea_dkey2.ptr : c->d_sea_dkey.ptr;
        t.spos = twin ? c->d_sea_dpos2.ptr : c->d_sea_dpos.ptr;
        t.ntiles = nt;
        t.tile_pos = c->d_tp_tile_pos.ptr;
        t.tile_sd = c->d_tp_tile_sd.ptr;
        t.tblocks = (nt * 32 + 255) / 256;
        t.rkey = twin ? c->d_sea_rkey2.ptr : c->d_sea_rkey.ptr;
        t.rord = twin ? c->d_sea_rord2.ptr : c->d_sea_rord.ptr;
        t.nblocks = nbk;
        t.slot_range = c->d_tp_slot_range.ptr;
        t.range_slot = c->d_tp_range_slot.ptr;
        t.blk_sr = c->d_tp_blk_sr.ptr;
        t.blk_u = c->d_tp_blk_u.ptr;
        tp_build<<<t.tblocks + (nbk * 32 + 255) / 256, 256, 0, c->stream>>>(t);
    }
    // the domain tiles from the pool rows, the range blocks from rpix, and the seed work (which reads what
    // tp_build wrote); the windowed search's guard thresholds come with the tile guards
    const bool search = nr && ng; // else no ranges, or no domain in any range's bucket
    {
        MfmaDomainPrepArgs d;
        d.pool = c->d_pool.ptr;
        d.negsd2 = c->d_negsd2.ptr;
        d.tile_pos = c->d_tp_tile_pos.ptr;
        d.ntiles = nt;
        d.dtiles = c->d_m_dtiles.ptr;
        d.dconst = c->d_m_dconst.ptr;
        DftDomainBuildArgs b;
        b.src = c->d_src.ptr;
        b.sstride = c->d_sstride;
        b.doms = c->d_doms.ptr;
        b.porig = c->d_porig.ptr;
        b.pool = c->d_pool.ptr;
        b.negsd2 = c->d_negsd2.ptr;
        b.tpool = c->d_dft_tpool.ptr;
        MfmaRangePrepArgs r;
        r.tgt = dtgt;
        r.tstride = tstride;
        r.ranges = c->d_ranges.ptr;
        r.slot_range = c->d_tp_slot_range.ptr;
        r.nblocks = nbk;
        r.T = 4;
        r.rfrags = c->d_m_rfrags.ptr;
        r.rconst = c->d_m_rconst.ptr;
        FRAC_HIP(c, c->d_dft_rorb.ensure((size_t)std::max(nbk, 1u) * 32 * 32));
        r.rorb = c->d_dft_rorb.ptr;
        r.rpix = c->d_tp_rpix.ptr;
        TpSeedWorkArgs sw;
        if (search) {
            sw.groups = c->d_tp_groups.ptr;
            sw.ngroups = ng;
            sw.blk_sr = c->d_tp_blk_sr.ptr;
            sw.tile_sd = c->d_tp_tile_sd.ptr;
            sw.work = c->d_tp_work.ptr;
        }
        const uint32_t dblocks = (nt * 64 + 255) / 256; // two lanes per tile row, a wave per tile
        const uint32_t rblocks = (nbk * 64 + 255) / 256; // two lanes per range slot
        const uint32_t pg = dblocks + rblocks + (sw.ngroups + 255) / 256;
        if (pg)
            tp_prep<<<pg, 256, 0, c->stream>>>(d, b, c->d_dft_tguard.ptr, kTpFast ? c->d_dft_trmax.ptr : nullptr, dblocks,
                                               r, c->d_dft_rguard.ptr, rblocks, sw);
    }
    if (timing)
        FRAC_TRY(mark_event(c, 1));
    if (!search) { // every record is the default
        if (timing && budgeted)
            FRAC_TRY(mark_event(c, 2));
        return FRAC_OK;
    }
    DftArgs da;
    da.m = search_args(c, c->d_tp_work.ptr, ng); // (host-planned only: no plan)
    da.rguard = c->d_dft_rguard.ptr;
    da.trmax = nullptr; // the seed search runs the exact epilogue (kTpSeedVar); the windowed search's below
    // seed: the Fourier search over one tile per group, into the records the windowed search writes again
    da.rec = c->d_tp_rec.ptr;
    search_dft<false, kTpSeedVar, true><<<ng, 64 * kDftBlocksPerWG, 0, c->stream>>>(da);
    // per group: its blocks' seed bounds, then its window
    TpWindowArgs w;
    w.groups = c->d_tp_groups.ptr;
    w.ngroups = ng;
    w.blk_sr = c->d_tp_blk_sr.ptr;
    w.blk_u = c->d_tp_blk_u.ptr;
    w.rec = c->d_tp_rec.ptr;
    w.slot_range = c->d_tp_slot_range.ptr;
    w.rconst = c->d_m_rconst.ptr;
    w.tile_sd = c->d_tp_tile_sd.ptr;
    w.hitH = c->hitH;
    w.work = c->d_tp_work.ptr;
    w.pairs = c->d_tp_pairs.ptr;
    w.bk = c->tp_bk;
    w.evals = c->d_tp_evals.ptr;
    w.sevals = c->d_tp_sevals.ptr;
    tp_seed_windows<<<ng, 256, 0, c->stream>>>(w);
    // the totals (the searched pairs and evaluations) written straight into the host's pinned block
    void* dtot = nullptr;
    FRAC_HIP(c, hipHostGetDevicePointer(&dtot, c->h_tp_tot.ptr, 0));
    tp_plan<<<1, kTpPlanThreads, 0, c->stream>>>(ng, c->d_tp_pairs.ptr, c->d_tp_evals.ptr, c->d_tp_sevals.ptr,
                                                 reinterpret_cast<uint32_t*>(dtot),
                                                 kTpLongestFirst ? c->d_tp_order.ptr : nullptr);
    FRAC_HIP(c, hipStreamSynchronize(c->stream));
    uint32_t tot[8];
    for (int k = 0; k < 8; ++k)
        tot[k] = c->h_tp_tot->w[k];
    const uint64_t pairs = (uint64_t)tot[2] | ((uint64_t)tot[3] << 32);
    if (budgeted) {
        // the seed search is issued work on either route: one tile per block, the tiled form's MFMAs
        const uint64_t seed_flops = c->tp_seed_pairs * 6ull * 32768ull;
        const uint64_t seed_evals = (uint64_t)tot[6] | ((uint64_t)tot[7] << 32);
        if (pairs * kAutoPruneBudgetDen > c->tp_full_pairs * kAutoPruneBudgetNum) {
            if (getenv("FRAC_TRACE"))
                fprintf(stderr, "[frac auto] windows %llu of %llu block x tile pairs: over the budget, exhaustive search "
                                "(windowed search not launched)\n", (unsigned long long)pairs, (unsigned long long)c->tp_full_pairs);
            // launch_dft reads the MFMA route's own maps and lists and rebuilds every frame-derived buffer in
            // dft_prep (fill_tp); best_key and fb_count were reset by tp_keys and nothing has written them
            FRAC_TRY(launch_dft(c, dtgt, tstride, false, false));
            c->flops_ran += seed_flops;
            c->evaluated_ran = c->eligible_pairs + seed_evals;
            return FRAC_OK;
        }
        c->flops_ran = seed_flops;
        c->evaluated_ran = seed_evals;
    }
    // issued matrix work (8 MFMA 32×32×16 per block × tile) and the (range, domain) pairs in the windows
    // (padding slots and rows of partial blocks and tiles are no pairs)
    c->flops_ran += pairs * 6ull * 32768ull;
    c->evaluated_ran += (uint64_t)tot[4] | ((uint64_t)tot[5] << 32);
    da.trmax = kTpFast ? c->d_dft_trmax.ptr : nullptr;
    da.order = kTpLongestFirst ? c->d_tp_order.ptr : nullptr; // the longest windows first (tp_plan)
    launch_search_dft<kTpVar, true>(c, da, ng, c->hitH > 0);
    if (timing)
        FRAC_TRY(mark_event(c, 2));
    MfmaResolveArgs v = resolve_args(c, dtgt, tstride, nr, nullptr, nullptr); // (records, no CSR map)
    v.entries = nullptr;
    v.rec = c->d_tp_rec.ptr;
    v.blk_group = c->d_tp_blk_group.ptr;
    v.work = c->d_tp_work.ptr;
    v.T = 4;
    v.slot_range = c->d_tp_slot_range.ptr;
    v.range_slot = c->d_tp_range_slot.ptr; // (resolve_args names the MFMA route's maps)
    v.tile_pos = c->d_tp_tile_pos.ptr;
    v.nslots = c->nblocks * 32u;
    v.tpool = c->d_dft_tpool.ptr;
    v.rorb = c->d_dft_rorb.ptr;
    FRAC_HIP(c, c->d_rstat.ensure(nr));
    v.rstat = c->d_rstat.ptr;
    fuse_fit(c, v);
    // resolve_dft<true> (SORTED) keeps every tie of the ΣD4-ordered chunks but does not merge T = 8's
    // flipped copies (that is the !SORTED path): the tiled form exists for T = 4 only (prepare)
    v.flip_slots = 0;
    if (c->dft_copies != 1 || c->p.transforms != 4)
        return c->fail(FRAC_E_STATE, "SEA tiled form: T = 4 only (resolve_dft<true> has no flipped copies)");
    // tuples bound for host memory leave in range order, else the walk is in slot order; in groups of
    // kTpGrpItems with one fit per range (resolve_dft_groups), or — kTpGrpHits false — with a hit threshold
    // (H > 0; at H = 0 a hit is an exact match) one wave per item: the first-hit walks of a group's items differ
    // widely in length
    const bool by_range = kTpRangeOrder && v.fit.tuples && c->tuple_sink_host;
    if (kTpGrpHits || c->hitH <= 0) {
        if (by_range)
            resolve_dft_groups<true><<<std::max(1u, tp_grp_grid(nr)), kTpGrpWaves * 64, 0, c->stream>>>(v);
        else
            resolve_dft_groups<false><<<std::max(1u, tp_grp_grid(v.nslots)), kTpGrpWaves * 64, 0, c->stream>>>(v);
    } else if (by_range)
        resolve_dft<true, true><<<std::max(1u, (nr + 3) / 4), 256, 0, c->stream>>>(v);
    else
        resolve_dft<true><<<std::max(1u, (v.nslots + 3) / 4), 256, 0, c->stream>>>(v);
    return FRAC_OK;
}

// SEA engine (fracenc_sea.hip): domain keys → radix sort (bucket, ΣD4) → sorted entries;
// range keys → radix sort by ΣR; then one wave per range writes best_key.
template <int N>
int launch_sea(frac_ctx* c, const uint8_t* dtgt, uint32_t tstride, bool timing)
{
    if constexpr (N == 8) {
        if (c->tp)
            return launch_tp(c, dtgt, tstride, timing);
    }
    const uint32_t nr = (uint32_t)nranges(c), P = c->npos * (c->virt ? c->p.transforms : 1u);
    if (P) {
        sea_domain_keys<N><<<(P + 255) / 256, 256, 0, c->stream>>>(c->d_pool.ptr, P, c->d_sea_bend.ptr,
                                                                   (uint32_t)c->bucket_end.size(), c->d_sea_dkey.ptr,
                                                                   c->d_sea_dpos.ptr);
        size_t tb = c->sea_tmp_bytes;
        FRAC_HIP(c, sort_pairs_u32(c->d_sea_tmp.ptr, tb, c->d_sea_dkey.ptr, c->d_sea_dkey2.ptr, c->d_sea_dpos.ptr,
                                   c->d_sea_dpos2.ptr, P, 20, c->stream));
        const uint32_t pieces = (N * N / 2 + 3) / 4;
        sea_domain_entries<N><<<(P * pieces + 255) / 256, 256, 0, c->stream>>>(
            c->d_sea_dkey2.ptr, c->d_sea_dpos2.ptr, c->d_negsd2.ptr, c->d_pool.ptr, P, c->d_sea_ent.ptr,
            c->d_sea_spool.ptr, c->d_sea_snegsd2.ptr);
    }
    if (nr) {
        sea_range_keys<N><<<(nr + 255) / 256, 256, 0, c->stream>>>(dtgt, tstride, c->d_ranges.ptr, nr,
                                                                    c->d_sea_rkey.ptr, c->d_sea_rord.ptr);
        size_t tb = c->sea_tmp_bytes;
        FRAC_HIP(c, sort_pairs_u32(c->d_sea_tmp.ptr, tb, c->d_sea_rkey.ptr, c->d_sea_rkey2.ptr, c->d_sea_rord.ptr,
                                   c->d_sea_rord2.ptr, nr, 17, c->stream));
    }
    if (timing)
        FRAC_TRY(mark_event(c, 1));
    FRAC_HIP(c, hipMemsetAsync(c->d_sea_count.ptr, 0, sizeof(unsigned long long), c->stream));
    if (nr) {
        SeaArgs a;
        a.tgt = dtgt;
        a.tstride = tstride;
        a.ranges = c->d_ranges.ptr;
        a.rbucket = c->d_rbucket.ptr;
        a.rorder = c->d_sea_rord2.ptr;
        a.ent = c->d_sea_ent.ptr;
        a.spool = c->d_sea_spool.ptr;
        a.snegsd2 = c->d_sea_snegsd2.ptr;
        a.nr = nr;
        a.hitH = c->hitH;
        a.best_key = c->d_best_key.ptr;
        a.evaluated = c->d_sea_count.ptr;
        if (c->Teff == 1) // the sampled form: one pool row per (domain, transform)
            sea_search<N, 1><<<(nr + 3) / 4, 256, 0, c->stream>>>(a);
        else if (c->p.transforms == 8)
            sea_search<N, 8><<<(nr + 3) / 4, 256, 0, c->stream>>>(a);
        else
            sea_search<N, 4><<<(nr + 3) / 4, 256, 0, c->stream>>>(a);
    }
    c->form_ran = FRAC_FORM_SEA;
    c->flops_ran = 0;
    return FRAC_OK;
}

// the sampled form's view of the context (fracenc_gen.hip)
GenArgs gen_args(frac_ctx* c, const uint8_t* dtgt, uint32_t tstride)
{
    GenArgs g;
    g.src = c->d_src.ptr;
    g.sstride = c->d_sstride;
    g.tgt = dtgt;
    g.tstride = tstride;
    g.doms = c->d_doms.ptr;
    g.ranges = c->d_ranges.ptr;
    g.porig = c->d_porig.ptr;
    g.nw = c->nw;
    g.nh = c->nh;
    g.Sw = c->Sw;
    g.Sh = c->Sh;
    g.T = c->p.transforms;
    g.K2 = c->K2;
    g.pool = c->d_pool.ptr;
    g.negsd2 = c->d_negsd2.ptr;
    g.nrows = c->npos * c->p.transforms;
    return g;
}

// the sampled form's fit (every range) and fp32 fallback (the flagged ones)
int launch_gen_finish(frac_ctx* c, const GenArgs& g)
{
    const uint32_t nr = (uint32_t)nranges(c);
    if (!nr)
        return FRAC_OK;
    if (!c->all_fallback) {
        GenFitArgs f;
        f.g = g;
        f.best_key = c->d_best_key.ptr;
        f.nr = nr;
        f.hitH = c->hitH;
        f.smax = c->p.s_max;
        f.all_fallback = 0;
        f.out = c->d_out.ptr;
        f.aux = c->d_aux.ptr;
        f.fb_count = c->d_fb_count.ptr;
        f.fb_list = c->d_fb_list.ptr;
        gen_fit<<<(nr + 255) / 256, 256, 0, c->stream>>>(f);
    }
    GenFallbackArgs b;
    b.g = g;
    b.rbucket = c->d_rbucket.ptr;
    b.fb_count = c->d_fb_count.ptr;
    b.fb_list = c->d_fb_list.ptr;
    b.thr = c->p.rms_threshold;
    b.smax = c->p.s_max;
    b.out = c->d_out.ptr;
    b.aux = c->d_aux.ptr;
    gen_fallback<<<512, 256, 0, c->stream>>>(b);
    return FRAC_OK;
}

// range sizes without a templated engine (n ∉ {2, 4, 8, 16}): the sampled form's pool, gen_search,
// gen_fit and gen_fallback
int launch_generic(frac_ctx* c)
{
    const uint32_t nr = (uint32_t)nranges(c);
    const bool timing = (c->p.flags & FRAC_FLAG_TIMING) != 0;
    const auto [dtgt, tstride] = target_plane(c);
    if (timing)
        FRAC_TRY(begin_timing(c));
    c->fit_fused = false; // gen_fit writes the records; frac_run packs the sink's tuples from them
    c->fb_pending = false;
    if (nr)
        FRAC_HIP(c, hipMemsetAsync(c->d_best_key.ptr, 0xff, nr * sizeof(unsigned long long), c->stream));
    FRAC_HIP(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->d_fb_count.ptr), (int)(c->all_fallback ? nr : 0u),
                                  1, c->stream));
    const GenArgs g = gen_args(c, dtgt, tstride);
    if (g.nrows)
        gen_pool_build<<<(g.nrows + 255) / 256, 256, 0, c->stream>>>(g);
    if (timing)
        FRAC_TRY(mark_event(c, 1));
    if (nr && !c->all_fallback) {
        GenSearchArgs a;
        a.g = g;
        a.rbucket = c->d_rbucket.ptr;
        a.nr = nr;
        a.hitH = c->hitH;
        a.best_key = c->d_best_key.ptr;
        gen_search<<<(nr + 3) / 4, 256, 0, c->stream>>>(a);
    }
    if (timing)
        FRAC_TRY(mark_event(c, 2));
    FRAC_TRY(launch_gen_finish(c, g));
    if (timing) {
        FRAC_TRY(mark_event(c, 3));
        ++c->hist_runs;
    }
    FRAC_HIP(c, hipGetLastError());
    c->engine_ran = FRAC_ENGINE_VALU;
    c->form_ran = FRAC_FORM_SAMPLED;
    c->flops_ran = 0;
    c->evaluated_ran = c->all_fallback ? 0 : c->eligible_pairs;
    return FRAC_OK;
}

template <int N>
int launch_all(frac_ctx* c)
{
    const uint32_t nr = (uint32_t)nranges(c), P = c->npos * (c->virt ? c->p.transforms : 1u);
    const bool timing = (c->p.flags & FRAC_FLAG_TIMING) != 0;
    const uint8_t* dsrc = c->d_src.ptr;
    const auto [dtgt, tstride] = target_plane(c);
    HostTrace tr("launch");
    if (timing)
        FRAC_TRY(begin_timing(c));
    c->fit_rstat = false;
    c->fit_fused = false;
    const bool use_mfma = c->engine == FRAC_ENGINE_MFMA && !c->all_fallback;
    // AUTO's pruned route: the tiled form's windows, or the Fourier search after them (launch_tp budgeted)
    const bool prune = N == 8 && use_mfma && c->auto_prune && !c->qplan;
    // the Fourier path resets best_key and fb_count in its preparation kernel (dft_prep)
    const bool dft_inits = N == 8 && use_mfma && nr && dft_route(c) && !prune;
    // so does the tiled form, in its key kernel (tp_keys: launch_tp, by either caller)
    const bool tp_inits = N == 8 && nr && (prune || (c->engine == FRAC_ENGINE_SEA && !c->all_fallback && c->tp));
    if (!dft_inits && !tp_inits && !c->qplan) { // (a planned level's qt_fill_maps did both)
        if (nr)
            FRAC_HIP(c, hipMemsetAsync(c->d_best_key.ptr, 0xff, nr * sizeof(unsigned long long), c->stream));
        const uint32_t fbc = c->all_fallback ? nr : 0u;
        // a device-side fill, not an H2D copy from pageable host memory (which serialises the host
        // with the stream)
        FRAC_HIP(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->d_fb_count.ptr), (int)fbc, 1, c->stream));
    }
    // the Fourier path and the SEA engine's tiled form build the pool in their fused domain pass
    // (dft_domain_build_pair_at)
    // (and the direct form at n = 4 / 16 in mfma_prep's domain half)
    const bool fused_pool = !c->virt &&
                            ((N == 8 && ((use_mfma && (c->p.transforms == 4 || c->dft_copies == 2) && mfma_dft_enabled(c)) ||
                                         (c->engine == FRAC_ENGINE_SEA && !c->all_fallback && c->tp))) ||
                             ((N == 4 || N == 16) && use_mfma));
    const GenArgs g = gen_args(c, dtgt, tstride);
    if (P && c->virt) // the sampled form: one row per (domain, transform), fracenc_gen.hip
        gen_pool_build<<<(P + 255) / 256, 256, 0, c->stream>>>(g);
    else if (P && !fused_pool) { // pool_lanes<N>() lanes per pool position
        const unsigned nblk = (unsigned)(((uint64_t)P * pool_lanes<N>() + 255) / 256);
        pool_build<N><<<nblk, 256, 0, c->stream>>>(dsrc, c->d_sstride, c->d_doms.ptr, c->d_porig.ptr, P, c->d_pool.ptr,
                                                   c->d_negsd2.ptr);
    }
    const bool use_sea = c->engine == FRAC_ENGINE_SEA && !c->all_fallback;
    tr.mark("memsets + pool");
    if (prune)
        FRAC_TRY(launch_tp(c, dtgt, tstride, timing, true));
    else if (use_mfma)
        FRAC_TRY(launch_mfma<N>(c, dtgt, tstride, dft_inits));
    if constexpr (N <= 8) {
        if (use_sea)
            FRAC_TRY(launch_sea<N>(c, dtgt, tstride, timing));
    }
    tr.mark("engine launch");
    const bool use_valu = !use_mfma && !use_sea;
    if (timing && use_valu)
        FRAC_TRY(mark_event(c, 1));
    if (use_valu && !c->all_fallback && !c->work.empty()) {
        SearchArgs a;
        a.tgt = dtgt;
        a.tstride = tstride;
        a.ranges = c->d_ranges.ptr;
        a.slot_range = c->d_slot_range.ptr;
        a.pool = c->d_pool.ptr;
        a.negsd2 = c->d_negsd2.ptr;
        a.work = c->d_work.ptr;
        a.nwork = (uint32_t)c->work.size();
        a.hitH = (int32_t)std::max<int64_t>(c->hitH, 0);
        a.best_key = c->d_best_key.ptr;
        const dim3 grid((a.nwork + 3) / 4), block(256);
        const bool hits = c->hitH > 0; // H = 0: the first maximum of w is the first hit
        if (N == 16 || c->G == 1) { // one copy: n = 16, or the sampled form's identity transform
            if (hits)
                search_valu<N, 1, true><<<grid, block, 0, c->stream>>>(a);
            else
                search_valu<N, 1, false><<<grid, block, 0, c->stream>>>(a);
        } else if constexpr (N <= 4) {
            if (c->G == 8) {
                if (hits)
                    search_valu<N, 8, true><<<grid, block, 0, c->stream>>>(a);
                else
                    search_valu<N, 8, false><<<grid, block, 0, c->stream>>>(a);
            } else {
                if (hits)
                    search_valu<N, 4, true><<<grid, block, 0, c->stream>>>(a);
                else
                    search_valu<N, 4, false><<<grid, block, 0, c->stream>>>(a);
            }
        } else if constexpr (N < 16) { // n = 16 never takes a 4-copy group (4 × 128 words of copies would spill)
            if (hits)
                search_valu<N, 4, true><<<grid, block, 0, c->stream>>>(a);
            else
                search_valu<N, 4, false><<<grid, block, 0, c->stream>>>(a);
        }
    }
    if (timing && !use_mfma)
        FRAC_TRY(mark_event(c, 2));
    if (c->virt) {
        FRAC_TRY(launch_gen_finish(c, g));
    } else if (!c->all_fallback && nr && !c->fit_fused) {
        FitArgs f = fit_args(c, dtgt, tstride, nr);
        if (c->fit_rstat)
            fit_rstat<N><<<(nr + 255) / 256, 256, 0, c->stream>>>(f, c->d_rstat.ptr);
        else
            fit_winner<N><<<std::max(1u, (nr + 4 * (64 / fit_lanes<N>()) - 1) / (4 * (64 / fit_lanes<N>()))), 256, 0,
                            c->stream>>>(f);
    }
    // the fp32 fallback: the fused resolvers (n ≥ 8; below no range leaves the exact regime) list their
    // fp32-regime ranges and fallback_grid settles them before the records are read (settle_fallback); every
    // other path runs it here
    c->fb_pending = false;
    if (nr && !c->virt) {
        FRAC_TRY(ensure_fb_scratch(c));
        const FallbackArgs b = fallback_args(c, dtgt, tstride);
        if (c->fit_fused && !c->all_fallback) {
            if constexpr (N >= 8) {
                c->fb_pending = true;
                c->fb_n = N;
                c->fb_args = b;
            }
        } else {
            launch_fallback_grid<N>(c, b);
        }
    }
    if (timing) {
        FRAC_TRY(mark_event(c, 3));
        ++c->hist_runs;
    }
    FRAC_HIP(c, hipGetLastError());
    tr.mark("fit + fallback");
    c->engine_ran = use_mfma ? FRAC_ENGINE_MFMA : use_sea ? FRAC_ENGINE_SEA : FRAC_ENGINE_VALU;
    if (!(use_sea && c->tp) && !prune) // the tiled form counted its evaluated pairs in launch_tp
        c->evaluated_ran = c->all_fallback ? 0 : c->eligible_pairs; // SEA: read back at fetch
    if (use_valu) {
        c->form_ran = FRAC_FORM_DOT2;
        c->flops_ran = 0;
    }
    return FRAC_OK;
}

// launch_all for the templated range side n ∈ {2, 4, 8, 16}
int launch_all_n(frac_ctx* c, uint32_t n)
{
    switch (n) {
    case 2: return launch_all<2>(c);
    case 4: return launch_all<4>(c);
    case 16: return launch_all<16>(c);
    default: return launch_all<8>(c);
    }
}

} // namespace
