// fracenc_ctx.h — the host layer's context: the types that own its GPU resources, frac_ctx itself, the
// error macros, the timing events and the small helpers every host file uses.  Included by
// fracenc_api.hip only (after the kernel files).
namespace {

thread_local std::string g_last_error;

// (key, value) radix sort of u32 pairs on the low `bits` key bits. rocPRIM's default picks a
// block-sort + merge-sort path below 2^20 items: 17 launches for the 2^18 keys of a C3 frame,
// whose launch gaps cost more than the sort. Merge-sort limit 0 selects Onesweep (histogram +
// one pass per 8-bit digit).
using OnesweepConfig =
    rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config, 0>;
hipError_t sort_pairs_u32(void* tmp, size_t& bytes, const uint32_t* kin, uint32_t* kout, const uint32_t* vin,
                          uint32_t* vout, uint32_t n, uint32_t bits, hipStream_t s)
{
    return rocprim::radix_sort_pairs<OnesweepConfig>(tmp, bytes, kin, kout, vin, vout, n, 0u, bits, s);
}

// The context's GPU resources, each owned by its type: a member frees itself when the context goes
// (after ~frac_ctx has synchronised the streams), so a new buffer is one declaration.  Move-only.

// a device buffer that only grows; at least one element once ensure() has succeeded
template <class T>
struct DBuf {
    T* ptr = nullptr;
    size_t cap = 0;
    DBuf() = default;
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
    DBuf(DBuf&& o) noexcept : ptr(o.ptr), cap(o.cap) { o.ptr = nullptr, o.cap = 0; }
    DBuf& operator=(DBuf&& o) noexcept
    {
        std::swap(ptr, o.ptr);
        std::swap(cap, o.cap);
        return *this;
    }
    ~DBuf() { release(); }
    hipError_t ensure(size_t n)
    {
        if (n <= cap && ptr)
            return hipSuccess;
        release();
        const size_t want = std::max<size_t>(n, 1);
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&ptr), want * sizeof(T));
        if (e == hipSuccess)
            cap = want;
        return e;
    }

private:
    void release()
    {
        if (ptr)
            (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
};
static_assert(!std::is_copy_constructible_v<DBuf<int>>);

// one pinned host object, allocated on first use
template <class T>
struct Pinned {
    T* ptr = nullptr;
    Pinned() = default;
    Pinned(Pinned&& o) noexcept : ptr(o.ptr) { o.ptr = nullptr; }
    ~Pinned()
    {
        if (ptr)
            (void)hipHostFree(ptr);
    }
    hipError_t ensure() { return ptr ? hipSuccess : hipHostMalloc(reinterpret_cast<void**>(&ptr), sizeof(T)); }
    T* operator->() const { return ptr; }
};

// pinned host bytes that only grow
struct PinnedBytes {
    uint8_t* ptr = nullptr;
    size_t cap = 0;
    PinnedBytes() = default;
    PinnedBytes(PinnedBytes&& o) noexcept : ptr(o.ptr), cap(o.cap) { o.ptr = nullptr, o.cap = 0; }
    ~PinnedBytes() { release(); }
    hipError_t ensure(size_t n)
    {
        if (n <= cap && ptr)
            return hipSuccess;
        release();
        const size_t want = std::max<size_t>(n, 1);
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&ptr), want);
        if (e == hipSuccess)
            cap = want;
        return e;
    }

private:
    void release()
    {
        if (ptr)
            (void)hipHostFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
};

// an event, created by its user (the flags differ) into `e`
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    ~Event()
    {
        if (e)
            (void)hipEventDestroy(e);
    }
    operator hipEvent_t() const { return e; }
};

// a stream the context created (a caller's stream, frac_set_stream, is a plain hipStream_t)
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
    ~Stream()
    {
        if (s)
            (void)hipStreamDestroy(s);
    }
    operator hipStream_t() const { return s; }
};

// the device FRQ1 packer's section table (fracenc_frq1pack.hip: frq1_table writes it, frq1_pack reads it)
struct Frq1Table {
    uint32_t bm_word[4], rec_word[4]; // the level's bitmap / record section: first body dword
    uint32_t reach0[4], leaf0[4];     // reached nodes / leaves before the level
    uint32_t words, leaves;           // the body's dwords, the stream's leaves
};
struct Frq1Result {
    Frq1Table t;
    unsigned long long mm[4]; // max ~key(contrast), max key(contrast), the same of the brightness
};

} // namespace

struct frac_ctx {
    int device = 0;
    frac_params p{};
    // the streams come before every buffer: members go in reverse order, the buffers first
    Stream own_stream;
    hipStream_t stream = nullptr; // own_stream, or the caller's (frac_set_stream)
    // Host planes after the first of a geometry (frac_set_frame, frac_set_planes, frac_set_frame_async: one
    // helper, upload_planes in fracenc_api.hip): the upload runs on the context's copy stream into the twin of
    // each plane buffer, which the runs already enqueued do not read, after the runs that last read that twin
    // (next_free); the context's stream waits for the upload (up_done) and the buffers swap, so frame k+1 crosses
    // PCIe while frame k's kernels still run.  The blocking setters then wait for up_done alone, not for the
    // context's stream.  Everything here is created on the first frame that has a predecessor of its geometry:
    // a one-shot encode has no twin and no copy stream.
    struct FrameStream {
        Stream copy_stream;
        DBuf<uint8_t> d_src_next, d_tgt_next;
        Event up_done, next_free;
        bool next_free_recorded = false;
    } frame;
    std::string err;

    struct PlaneSize {
        uint32_t w = 0, h = 0;
    } src, tgt;
    bool same_plane = true;
    bool planes_set = false;
    DBuf<uint8_t> d_src, d_tgt;
    uint32_t d_sstride = 0, d_tstride = 0;

    std::vector<frac_grid_item> doms, ranges;
    bool doms_set = false, ranges_set = false;
    bool dirty = true;

    // prepared state
    int n = 0;               // range side (0: rectangular ranges or domains, the sampled form)
    uint32_t S = 0;          // domain side (width for rectangles)
    uint32_t nw = 0, nh = 0, Sw = 0, Sh = 0; // range and domain width / height
    bool virt = false;       // sampled form (fracenc_gen.hip): one pool row per (domain, transform)
    bool generic = false;    // sampled form with a range size no templated engine covers (gen_search)
    uint32_t Teff = 4;       // transforms the engines search per pool row (1 in the sampled form)
    uint32_t K2 = 0;         // dwords per pool row
    uint32_t G = 4, NG = 1;
    uint32_t npos = 0;                      // pool positions (= domains); d_porig maps them to domain indices
    std::vector<uint32_t> bucket_begin, bucket_end; // per bucket (category + 1): pool positions
    BucketLayout layout{};                  // per-bucket counts and offsets (fracenc_bucket.hip); VALU slots
    BucketLayout mlayout{};                 // the same with the MFMA engine's 32-slot blocks and tiles
    uint32_t nvslots = 0;                   // VALU engine: range slots (64 per wave)
    bool doms_uploaded = false;             // d_doms holds c->doms
    bool doms_trusted = false;              // c->doms built by this library (quadtree levels): not re-validated
    bool ranges_dev = false;                // d_ranges was filled on the device (quadtree level): nr_dev items of n_dev
    uint32_t nr_dev = 0, n_dev = 0;
    std::vector<uint32_t> h_rkey, h_porig;  // frac_fetch: per-range bucket, pool order (classifier stats)
    std::vector<uint4> work;
    int64_t hitH = -1;
    bool all_fallback = false;

    DBuf<frac_grid_item> d_doms, d_ranges;
    DBuf<uint32_t> d_porig, d_pool, d_fb_list, d_fb_count;
    // fallback_grid's per-listed-range scratch: the least key so far and the jobs done; all-ones / zero between
    // runs (the last job of a range resets its pair), set so when (re)allocated
    DBuf<unsigned long long> d_fb_key;
    DBuf<uint32_t> d_fb_done;
    // a fused resolver's fp32-regime ranges are listed, not evaluated: fallback_grid settles them before the
    // run's records are read (settle_fallback; frac_fetch launches it only when a range was listed)
    bool fb_pending = false;
    int fb_n = 0;
    FallbackArgs fb_args{};
    DBuf<int32_t> d_negsd2, d_slot_range;
    DBuf<uint4> d_work;
    DBuf<uint2> d_rbucket;
    DBuf<uint32_t> d_rord, d_rkey;           // bucket-sorted range order; per range bucket
    DBuf<uint32_t> d_bk_keys, d_bk_first, d_bk_cnt;
    DBuf<uint16_t> d_bsum_s, d_bsum_t; // the source / target plane's block sums (frame_block_sums)
    DBuf<unsigned long long> d_best_key;
    DBuf<frac_encode_item> d_out;
    DBuf<RangeAux> d_aux;

    // MFMA engine layout
    uint32_t engine = FRAC_ENGINE_VALU;    // engine chosen for the current geometry
    uint32_t nblocks = 0, ntiles = 0;
    std::vector<uint4> m_work;             // per WG (4 range blocks: search_mfma)
    std::vector<uint32_t> m_blk_ptr, m_blk_ent;
    std::vector<uint4> m8_work;            // per WG (kDftBlocksPerWG = 8 range blocks: search_dft); no CSR map:
                                           // the Fourier search merges its splits per slot (d_dft_slotbest)
    bool m8_built = false;                 // m8_work was built for this geometry (it may still hold no work)
    // T = 8 on the Fourier path (n = 8, ratio 2): Flip_Rotate_k = Flip ∘ Rotate_k (image/transform.h:32-41),
    // so the flip half is the rotation search of each range read through Flip — a second copy of every
    // range block (blocks nblocks .. 2·nblocks − 1, same bucket), resolved together with the original
    // (resolve_dft: Rotate-group index t' of the flipped copy = transform 4 + (−t' mod 4))
    uint32_t dft_copies = 1;
    DBuf<uint4> d_m8_work;
    DBuf<int32_t> d_m_slot_range, d_m_tile_pos;
    DBuf<uint32_t> d_m_range_slot, d_m_blk_ptr, d_m_blk_ent, d_m_rconst, d_m_dconst;
    DBuf<uint4> d_m_work, d_m_dtiles, d_m_rfrags;
    DBuf<uint2> d_m_entries;

    // decoder state
    DBuf<uint8_t> d_dec_src, d_dec_tgt, d_color;
    DBuf<unsigned long long> d_dec_part;
    DBuf<DecodeState> d_dec_state;
    Pinned<DecodeState> h_dec_state;
    DBuf<uint2> d_dft_tguard;
    DBuf<int32_t> d_dft_trmax; // the six-MFMA fast path's per-tile R6 threshold (kDftFast6)
    DBuf<uint32_t> d_dft_tpool; // pool rows in tile order (resolve_dft)
    DBuf<uint32_t> d_dft_rorb;  // range pixel pairs in orbit order, per slot (resolve_dft)
    DBuf<frac_qt_leaf> d_qt_leaves32; // frac_encode_quadtree_leaves' device-side leaves (pageable caller buffer)
    DBuf<unsigned long long> d_dft_slotbest; // per slot the search's merged word (search_dft → resolve_dft,
                                             // search_mfma n ≤ 4 → resolve_small)
    DBuf<uint4> d_rstat;        // per range: the winner's sums (resolve_dft → fit_rstat)
    DBuf<frac_grid_item> d_cls_items;
    DBuf<uint32_t> d_cls_list;
    DBuf<int32_t> d_cls_out;
    DBuf<uint32_t> d_dft_rguard;
    // SEA engine: sort keys/values (double-buffered for the radix sort), sorted entries
    DBuf<uint32_t> d_sea_dkey, d_sea_dkey2, d_sea_dpos, d_sea_dpos2, d_sea_rkey, d_sea_rkey2, d_sea_rord,
        d_sea_rord2, d_sea_bend, d_sea_spool;
    DBuf<SeaEntry> d_sea_ent;
    DBuf<int32_t> d_sea_snegsd2;
    DBuf<frac_tuple> d_tuples; // frac_fetch_tuples staging
    frac_tuple* tuple_sink = nullptr; // frac_set_tuple_sink: every frac_run's tuples also go here
    bool tuple_sink_host = false;     // the sink is host memory (the sorted resolve then walks in range order)
    // SEA engine, tiled form (fracenc_tp.hip)
    bool tp = false;
    TpBuckets tp_bk{};
    std::vector<uint4> tp_groups;
    uint32_t tp_key_bits = 16; // (bucket << 16 | Σ) sort keys: 16 + ⌈log2 nb⌉ bits
    std::vector<uint2> tp_blk_group;
    DBuf<uint4> d_tp_groups;
    DBuf<uint2> d_tp_blk_group, d_tp_tile_sd, d_tp_blk_sr;
    DBuf<uint32_t> d_tp_blk_u, d_tp_pairs;
    DBuf<uint8_t> d_tp_rpix;   // [nr][64] the ranges' pixels in range order (tp_keys → tp_prep)
    DBuf<uint32_t> d_tp_order; // [groups] the windowed search's work item per workgroup, longest window first (tp_plan)
    DBuf<uint4> d_tp_rec;     // [nblocks·64] search_dft CHUNKED's record per block and lane (DftArgs::rec)
    struct TpTotals {
        uint32_t w[8];
    };
    Pinned<TpTotals> h_tp_tot; // mapped: tp_plan writes the run's totals there (read after launch_tp's synchronisation)
    // the tiled form's own maps and work lists, in its sorted layout (rebuilt every run): under AUTO the
    // MFMA engine's domain-ordered ones (d_m_tile_pos, the slot maps, d_m8_work) stay prepared beside them
    DBuf<int32_t> d_tp_slot_range, d_tp_tile_pos;
    DBuf<uint32_t> d_tp_range_slot;
    DBuf<uint4> d_tp_work;
    DBuf<unsigned long long> d_tp_sevals; // per group, the (range, domain) pairs of its seed tile
    // FRAC_ENGINE_AUTO's pruned route (select_engine): the tiled form's windows first, the exhaustive
    // Fourier search in the same run when they exceed kAutoPruneBudget of tp_full_pairs
    bool auto_prune = false;
    uint64_t tp_full_pairs = 0; // block × tile pairs with every window open (Σ groups: blocks · bucket tiles)
    uint64_t tp_seed_pairs = 0; // block × tile pairs of the seed search (Σ groups: blocks)
    DBuf<int32_t> d_tp_rbk;
    DBuf<uint32_t> d_tp_sort_table; // tp_sort_pairs' digit tables, both sides (fill_tp: tp_sort_table_words)
    DBuf<Frc1MinMax> d_frc_mm;             // frac_pack_frc1
    DBuf<unsigned long long> d_frc_rec;
    DBuf<uint32_t> d_frc_words;
    DBuf<uint32_t> d_frc_in, d_frc_status; // frac_decode_frc1: the padded stream body; {bad, domain-less} counts
    // frac_decode_frq1: the padded body; the levels' node origins (two buffers, level k reads one and writes the
    // other); a level's per-dword split ranks; the leaf entries; the fast path's leaf number per min_size cell
    DBuf<uint32_t> d_frq_in, d_frq_nodes[2], d_frq_rank, d_frq_map;
    DBuf<uint4> d_frq_leaves;
    // frac_decode_frc3: the decoded Y, U and V planes (pitch plane_pitch of each width), which never leave the
    // device, and after them the host variant's RGB staging rows (frac_decode_error_frc3: the host's reference)
    DBuf<uint8_t> d_frc3;
    // quadtree: the per-level domain grids (geometry only) of the last frame size, by log2(n)
    uint32_t qt_w = 0, qt_h = 0;
    std::vector<frac_grid_item> qt_doms[5];
    DBuf<frac_grid_item> qt_ddoms[5];     // their device copies
    DBuf<frac_grid_item> d_qt_next;       // the next level's ranges, built on the device
    DBuf<frac_encode_item> d_qt_leaves;   // the frame's leaves, in output order
    DBuf<uint32_t> d_qt_flags, d_qt_offs, d_qt_count;
    DBuf<unsigned long long> d_qt_stats; // quadtree: the levels' frac_stats counters (qt_level_stats)
    // device-planned quadtree levels (frac_encode_quadtree, MFMA engine): the levels' plans (+1 for
    // the count after the last), their bucket bounds, and the first level's range grid
    DBuf<DevPlan> d_qt_plan;
    Pinned<QtFrameSum> h_qt_sum; // mapped: qt_finish writes the frame's counts there
    DBuf<uint32_t> d_qt_first;
    const DevPlan* qplan = nullptr; // set while a device-planned level launches (launch_all in plan mode)
    uint32_t qp_nwork_cap = 0;      // its work-item bound: the search grid
    DBuf<uint8_t> d_qt_tmp;
    size_t qt_tmp_bytes = 0;
    bool qt_dvalid[5] = {false, false, false, false, false};
    // quadtree rate sweep (fracenc_qtrate.hip): the full tree of the last frac_quadtree_rate_build, level-major
    // (level k's N_k = 4^k·N_0 nodes from off[k]), and what answers every threshold from it.  Everything is
    // sized at build time, for the worst case; the readers allocate nothing from a device count.
    struct QtRate {
        bool ready = false;                // a readable state: cleared by every setter, frac_run and the quadtree calls
        uint32_t W = 0, H = 0, max_size = 0, min_size = 0, levels = 0, transforms = 0;
        bool classifier = false;           // the search ran classified (an FRQ1 header's flag bit 0)
        uint32_t nodes[4] = {0, 0, 0, 0};  // N_k of the full tree
        uint32_t off[5] = {0, 0, 0, 0, 0}; // first node of level k; off[levels] = the tree's node count
        uint32_t ndoms[4] = {0, 0, 0, 0};  // domains of level k: createUniformGrid(W, H, 2n, n)
        uint32_t nkeys = 0;                // nodes that can split: off[levels − 1]
        DBuf<frac_qt_leaf> d_nodes;        // every node's record, packed as qt_leaf_of
        DBuf<double> d_e;                  // [nkeys] split keys e(v) = min(d(v), e(parent(v)))
        DBuf<unsigned long long> d_key, d_skey; // their order-preserving bit patterns, unsorted / sorted
        DBuf<uint32_t> d_lvl, d_slvl;      // the keys' levels, unsorted / sorted with them
        DBuf<uint32_t> d_pre;              // [3][nkeys + 1] per level: keys of that level before sorted position i
        DBuf<uint32_t> d_flag, d_rank;     // [nodes + 1] frac_quadtree_rate_leaves: leaf flags, their exclusive scan
        DBuf<uint8_t> d_tmp;               // hipcub's scratch, the largest of the sort and the two scans
        size_t tmp_bytes = 0;
        DBuf<double> d_split;              // frac_quadtree_rate_sizes: thresholds in, results out
        DBuf<unsigned long long> d_bytes;
        DBuf<uint32_t> d_counts;           // [n][5]: leaves, splits[4]
        DBuf<unsigned long long> d_fit;    // frac_quadtree_rate_fit: {least fitting key, least size}
        DBuf<frac_qt_leaf> d_out;          // frac_quadtree_rate_leaves into pageable memory: staged here
        struct Result {
            unsigned long long key, bytes, min_bytes;
            uint32_t leaves, found;
        };
        Pinned<Result> h_res;              // mapped: the fit's answer, the emit's leaf count
    } rate;
    // the device FRQ1 packer (fracenc_frq1pack.hip), sized by the tree's node counts and the worst-case body:
    // per node of the level-major tree {reached, leaf} flags and their exclusive scan ([nodes + 1]), the search
    // route's leaf number per node, the zeroed body, the leaves' four bound keys, the section table
    struct Frq1Pack {
        DBuf<unsigned long long> d_flag, d_rank, d_mm;
        DBuf<uint32_t> d_slot, d_body;
        DBuf<uint8_t> d_tmp; // hipcub's scratch
        size_t tmp_bytes = 0;
        DBuf<Frq1Table> d_tab;
        Pinned<Frq1Result> h_res; // mapped: the table and the keys
    } frq1pack;
    // rate–distortion pruning of the rate state's tree (fracenc_qtrd.hip): the nodes' integer distortions, made
    // on the first RD call after a build, and the readers' multipliers, per-multiplier sums and answers.  Sized by
    // the tree's node count or by the caller's n.
    struct QtRd {
        bool q_ready = false;             // d_q holds the current rate state's q(v); frac_quadtree_rate_build clears it
        DBuf<uint32_t> d_q;               // [nodes] q(v) = llrint(d(v)·64n²), level-major like rate.d_nodes
        DBuf<unsigned long long> d_lam;   // the multipliers of one launch
        struct Acc {
            unsigned long long dist;      // Σ q over the partition's leaves
            uint32_t S[4];                // reached, splitting nodes per level
        };
        DBuf<Acc> d_acc;                  // [copies][n] per multiplier, one atomic per wave and quantity into a copy
        DBuf<unsigned long long> d_bytes, d_dist; // frac_quadtree_rd_sizes: results out
        DBuf<uint32_t> d_counts;          // [n][5]: leaves, splits[4]
        struct Fit {
            long long lo;                 // −1, or a multiplier whose stream does not fit
            unsigned long long hi;        // a multiplier whose stream fits (once found)
            unsigned long long bytes, dist, min_bytes;
            uint32_t leaves, found;
        };
        DBuf<Fit> d_fit;                  // frac_quadtree_rd_fit: the interval between the rounds
        Pinned<Fit> h_fit;                // mapped: its answer
    } rd;
    // decoded error (fracenc_quality.hip): the covered rectangle's sum and its block sums, the sum's pinned
    // landing place, the rate readers' stream on its way from the packer to the decoder, and the rate state's
    // sorted keys on the host (the quality fit's candidates); for a colour container the R, G and B sums and
    // their landing place
    struct Quality {
        struct Rgb {
            unsigned long long sse[3];
        };
        DBuf<unsigned long long> d_total, d_block, d_rgb_total;
        Pinned<unsigned long long> h_total;
        Pinned<Rgb> h_rgb_total;
        PinnedBytes stream;
        std::vector<unsigned long long> skey;
    } quality;
    DBuf<uint8_t> d_sea_tmp;
    DBuf<unsigned long long> d_sea_count; // candidates the SEA search evaluated
    DBuf<unsigned long long> d_tp_evals;  // tiled form: per group, the (range, domain) pairs of its window
    uint64_t eligible_pairs = 0;          // Σ over ranges of its bucket's domain count
    uint64_t evaluated_ran = 0;           // frac_stats.evaluated_mappings of the last run
    size_t sea_tmp_bytes = 0;
    DBuf<frac_encode_item> d_dec_items;
    DBuf<unsigned long long> d_dec_sum;
    Pinned<unsigned long long> h_dec_sum;

    std::vector<RangeAux> h_aux;
    Event ev[5];
    Event handoff; // frac_set_stream: the new stream waits for the old one's work (created on use)
    // FRAC_FLAG_TIMING: the same four boundaries (start | prep | search | finish) of every run
    // since the last frac_timing_history call, a ring of kHistRuns runs (created on first use)
    std::vector<Event> hist;
    uint64_t hist_runs = 0, hist_read = 0;
    int prep_knobs = -1; // FRAC_MFMA_VARIANT / FRAC_MFMA_DFT as of the last prepare (frac_run)
    int mfma_var_ran = 0; // the schedule variant search_mfma last ran with (its entry layout)
    bool ran = false;
    uint32_t engine_ran = FRAC_ENGINE_VALU;
    uint32_t form_ran = FRAC_FORM_DOT2;
    bool fit_rstat = false; // resolve_dft recorded the winners' sums (fit_rstat instead of fit_winner)
    bool fit_fused = false; // resolve_dft wrote the records itself (no fit launch)
    uint64_t flops_ran = 0;

    // idle before anything is released: the members free themselves after this body
    ~frac_ctx()
    {
        (void)hipSetDevice(device);
        if (stream)
            (void)hipStreamSynchronize(stream);
        if (frame.copy_stream)
            (void)hipStreamSynchronize(frame.copy_stream);
    }

    int fail(int code, const std::string& msg)
    {
        err = msg;
        g_last_error = msg;
        return code;
    }
    int hip(hipError_t e, const char* what)
    {
        if (e == hipSuccess)
            return FRAC_OK;
        return fail(FRAC_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    }
};

// ranges of the current search: the caller's list, or (quadtree levels) a list the device built
inline size_t nranges(const frac_ctx* c) { return c->ranges_dev ? c->nr_dev : c->ranges.size(); }

#define FRAC_TRY(expr)                                                                                                 \
    do {                                                                                                               \
        int _rc = (expr);                                                                                              \
        if (_rc != FRAC_OK)                                                                                            \
            return _rc;                                                                                                \
    } while (0)
#define FRAC_HIP(ctx, expr) FRAC_TRY((ctx)->hip((expr), #expr))

namespace {
constexpr uint32_t kHistRuns = 256;

// Boundary k of the current run (0 start, 1 search begins, 2 search ends, 3 finish ends), one
// event each: the run's slot in the timing history (frac_timing_history), which frac_stats reads
// for the last run (last_events). Every record is a marker packet the GPU waits on, so a second
// record per boundary cost C2 (Lenna 512², T = 8) ≈ 17 µs per frame.
// Boundaries 0–2 only time the chain: their markers skip the system-scope fence (a cache write-back
// and invalidate per marker, and the next kernel starting on a cold L2).  Boundary 3 ends the run
// and keeps the default fence, so a host that synchronises on the stream still sees every write.
hipError_t create_timing_event(hipEvent_t* e, size_t k)
{
    return (k % 4) == 3 ? hipEventCreate(e) : hipEventCreateWithFlags(e, hipEventDisableSystemFence);
}

int mark_event(frac_ctx* c, int k)
{
    hipEvent_t e = c->hist.empty() ? c->ev[k] : c->hist[(size_t)(c->hist_runs % kHistRuns) * 4 + k];
    FRAC_HIP(c, hipEventRecord(e, c->stream));
    return FRAC_OK;
}

// the four boundaries of the last completed launch (after launch_all / launch_generic counted it)
const Event* last_events(const frac_ctx* c)
{
    if (c->hist.empty() || c->hist_runs == 0)
        return c->ev;
    return &c->hist[(size_t)((c->hist_runs - 1) % kHistRuns) * 4];
}

// a completed run's times between its boundaries e[0..3], added to the stats
void add_run_times(frac_stats& s, const Event* e)
{
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e[0], e[3]) == hipSuccess)
        s.ms_device += ms;
    if (hipEventElapsedTime(&ms, e[0], e[1]) == hipSuccess)
        s.ms_prep += ms;
    if (hipEventElapsedTime(&ms, e[1], e[2]) == hipSuccess)
        s.ms_search += ms;
    if (hipEventElapsedTime(&ms, e[2], e[3]) == hipSuccess)
        s.ms_finish += ms;
}

// a timed run begins: the history ring on first use, then boundary 0
int begin_timing(frac_ctx* c)
{
    if (c->hist.empty()) {
        c->hist.resize(4 * kHistRuns);
        for (size_t i = 0; i < c->hist.size(); ++i)
            FRAC_HIP(c, create_timing_event(&c->hist[i].e, i));
    }
    return mark_event(c, 0);
}

// device rows are padded to 64 bytes
inline uint32_t plane_pitch(uint32_t w) { return (w + 63u) & ~63u; }

// a w×h plane between two pitches: one linear copy when the pitches agree (a 2-D copy is a slower path)
int copy_plane(frac_ctx* c, void* dst, uint32_t dpitch, const void* src, uint32_t spitch, uint32_t w, uint32_t h,
               hipMemcpyKind kind, hipStream_t stream)
{
    if (spitch == dpitch)
        FRAC_HIP(c, hipMemcpyAsync(dst, src, (size_t)spitch * (h - 1) + w, kind, stream));
    else
        FRAC_HIP(c, hipMemcpy2DAsync(dst, dpitch, src, spitch, w, h, kind, stream));
    return FRAC_OK;
}

// the plane the ranges lie on: the source plane unless a target plane was set
struct PlaneRef {
    const uint8_t* ptr;
    uint32_t stride;
};
inline PlaneRef target_plane(const frac_ctx* c)
{
    return c->same_plane ? PlaneRef{c->d_src.ptr, c->d_sstride} : PlaneRef{c->d_tgt.ptr, c->d_tstride};
}

// a host list to its device buffer, on the context's stream
template <class T>
int upload(frac_ctx* c, DBuf<T>& d, const std::vector<T>& v)
{
    FRAC_HIP(c, d.ensure(v.size()));
    if (v.empty())
        return FRAC_OK;
    return c->hip(hipMemcpyAsync(d.ptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, c->stream), "upload");
}
} // namespace

namespace {

int check_params(const frac_params* p, std::string& msg)
{
    if (!p) {
        msg = "params is NULL";
        return FRAC_E_INVALID;
    }
    if (p->transforms != 4 && p->transforms != 8) {
        msg = "transforms must be 4 or 8";
        return FRAC_E_INVALID;
    }
    if (p->engine > FRAC_ENGINE_SEA) {
        msg = "unknown engine";
        return FRAC_E_INVALID;
    }
    if (p->flags & ~(FRAC_FLAG_TIMING | FRAC_FLAG_DIRECT_FORM | FRAC_FLAG_SEA_PER_RANGE | FRAC_FLAG_DECODE_STEPWISE |
                     FRAC_FLAG_EXHAUSTIVE | FRAC_FLAG_PRUNE)) {
        msg = "unknown flag bits";
        return FRAC_E_INVALID;
    }
    return FRAC_OK;
}

// The A/B knobs of the tuning build.  A product build compiles only the shipped forms (the
// alternative exact forms are frac_params flags), so it refuses a run with any of these set rather
// than silently running the default: encode(), the C++ EncodingEngineCore and the reference-side
// binding cannot be steered into an A/B form by the environment.
constexpr const char* kAbKnobs[] = {"FRAC_MFMA_VARIANT", "FRAC_MFMA_DFT", "FRAC_DFT_WGS", "FRAC_XCD_ORDER",
                                    "FRAC_SEA_TILED", "FRAC_DECODE_UNFUSED"};

// the knob's value in a tuning build; nullptr in a product build (check_ab_knobs refused it)
inline const char* ab_knob(const char* name) { return kTuningBuild ? getenv(name) : nullptr; }

int check_ab_knobs(frac_ctx* c)
{
    if (kTuningBuild)
        return FRAC_OK;
    for (const char* k : kAbKnobs) {
        const char* v = getenv(k);
        if (v && *v)
            return c->fail(FRAC_E_INVALID, std::string(k) + "=" + v +
                                               ": A/B knobs exist only in a -DFRAC_TUNING build "
                                               "(tools/build_tuning.py); the alternative exact forms are frac_params flags");
    }
    return FRAC_OK;
}

// FRAC_TRACE=1: host wall-clock of the preparation and quadtree phases on stderr (tuning aid)
struct HostTrace {
    bool on;
    const char* what;
    std::chrono::steady_clock::time_point t0, t;
    explicit HostTrace(const char* w) : on(getenv("FRAC_TRACE") != nullptr), what(w)
    {
        t0 = t = std::chrono::steady_clock::now();
    }
    void mark(const char* phase)
    {
        if (!on)
            return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[frac %s] %-22s %8.3f ms (total %8.3f)\n", what, phase,
                std::chrono::duration<double, std::milli>(now - t).count(),
                std::chrono::duration<double, std::milli>(now - t0).count());
        t = now;
    }
};

} // namespace
