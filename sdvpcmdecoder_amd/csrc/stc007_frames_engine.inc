/*
 * stc007_frames_engine.inc - sdv_binarize_frames (include/sdvpcm.h): the chain speculation of engine.inc's header for STC-007 tapes, with everything such a
 * tape adds to it - reference-level sweeps settled off the frame kernel, crowds of given-up frames and their leaders, levels and histories carried along
 * the chain.  Included at the end of engine.inc, so by the one translation unit of either build; the flag block's layout and the pool of sweeps, which
 * sdv_binarize_lines shares, are engine.inc's (flag_tail_ofs, ensure_memo_capacity, settle_sweep_chunks).
 *
 *   ChainPlan (stc007_chain_plan.h)   what the host decides: plain code on bytes that were read back
 *   Stc007FrameCall                   what touches the device in one call: the launches, the copies, the pool of sweeps
 *   stc007_binarize_frames_impl       the call: checks, arguments, cold frame, first round, then round after round
 *                                     read back - settle sweeps - plan - upload - model kernels - round
 */
#include "stc007_chain_plan.h"

/* What the fused entry (sdv_decode_frames) hands the one frame call it makes: the stitcher's field buffers, for the frames the whole-frame capture takes
 * from end to end (FrameArgs::direct_fields; none: direct_fields == NULL), and device work of the stage behind, to be queued right behind the first round
 * - a tape that plays settles in that round, and the stage behind need not wait for the host to have seen that (none: after_first_round == NULL; it
 * returns SDV_OK or an error). */
struct FusedHooks {
    void *direct_fields; sdv::DirectFrame *direct_frames; int direct_seg_ofs, direct_pitch, direct_lines;
    int (*after_first_round)(void *ctx); void *after_ctx;
};

/* One call of the frame entry, as far as it touches the device. */
struct Stc007FrameCall {
    sdv_engine *const e;
    const rt::stream_t s;
    const int n, height;            /* frames of the call (the filler frame of END_FILE among them), lines of a frame */
    sdv::FrameArgs a;
    sdv::PredictArgs pa;
    uint8_t *const flag;            /* e->h_flag: what the last read_flags brought */
    const size_t tail_ofs;          /* where the last state sits behind the flags */
    const size_t tail_bytes;        /* ... and behind it the count of sweep requests */
    const size_t sig_ofs;           /* ... and the give-up signatures (read back with the rest once a crowd gave up) */
    /* the count of requests lives behind the flags and the last state for the time of the call: it comes back with every round's one read-back */
    int32_t *const d_count;
    /* Reference-level sweeps (stc007_sweep_device.h).  The full kernel does not sweep: a line that needs the outcome of a sweep looks it up, and
     * where there is none it leaves a request and its frame comes back as given up.  After every round the requests that are new are settled
     * (all of them at once, a wave per 64 levels of a line) and those frames decoded again, with the outcomes at hand. */
    bool memo_ready = false; int memo_done = 0;
    int sweeps_seen = 0;            /* requests of the call as of the last read-back */
    bool cold_frame = false;        /* the round decodes the first frame of a cold chain: nothing is tuned, its first lines are swept */
    bool round_fat = false;         /* the last round's general frames ran in the kernel that settles its sweeps itself */
    bool timing_pending = false;

    Stc007FrameCall(sdv_engine *e_, rt::stream_t s_, int n_, int height_)
        : e(e_), s(s_), n(n_), height(height_), flag(e_->h_flag), tail_ofs(flag_tail_ofs((size_t)n_)), tail_bytes(FLAG_TAIL_BYTES), sig_ofs(tail_ofs + FLAG_SIG_OFS),
          d_count(reinterpret_cast<int32_t *>(e_->d_flag + tail_ofs + sizeof(sdv_v2d_state)))
    {
        memset(&a, 0, sizeof(a));
        memset(&pa, 0, sizeof(pa));
    }

    /* the arguments of the frame kernels and of sdv_k_predict, as far as they hold for the whole call; takes the caller's per-frame marks */
    int set_arguments(const uint8_t *luma, size_t row_stride, size_t frame_stride, int width, uint32_t first_frame_no, unsigned flags, int n_real,
                      sdv_line_rec *out_lines, sdv_frame_stats *out_stats, const FusedHooks *hooks)
    {
        a.luma = luma; a.frame_stride = frame_stride; a.row_stride = row_stride; a.width = width; a.height = height;
        a.first_frame_no = first_frame_no;
        a.new_file_frame = (flags & SDV_FLAG_NEW_FILE) ? 0 : -1;
        a.end_file_frame = (flags & SDV_FLAG_END_FILE) ? n_real : -1;
        a.doubled = (flags & SDV_FLAG_DOUBLED) ? 1 : 0;
        a.mode = (uint8_t)e->mode; a.check_line_copy = (uint8_t)e->check_line_dup; a.coordinate_damper = (uint8_t)e->coordinate_damper;
        a.m2_format = (uint8_t)e->m2_format;
        a.preset = e->preset;
        a.states_in = e->d_states_in; a.states_out = e->d_states_out;
        a.recs = out_lines; a.stats = out_stats; a.scratch = e->d_scratch;
        a.flag = e->d_flag; a.refs = e->d_refs; a.n_total = n;
        a.sig = e->d_flag + sig_ofs;
        { const int rc = take_frame_flags(e, (size_t)n, s, &a.frame_flags); if (rc != SDV_OK) return rc; }
        if (hooks && hooks->direct_fields && hooks->direct_frames && !(flags & (SDV_FLAG_NEW_FILE | SDV_FLAG_END_FILE))) {
            a.direct_fields = hooks->direct_fields; a.direct_frames = hooks->direct_frames; a.direct_seg_ofs = hooks->direct_seg_ofs;
            a.direct_pitch = hooks->direct_pitch; a.direct_lines = hooks->direct_lines < hooks->direct_pitch ? hooks->direct_lines : hooks->direct_pitch;
        }
        pa.states = e->d_states_in; pa.doubled = a.doubled; pa.min_ref_lvl = e->preset.min_ref_lvl; pa.first_of = NULL; pa.skip = NULL; pa.flag = e->d_flag;
        return SDV_OK;
    }

    /* the two counts behind the last state, as of the last read_flags: sweep requests handed out, passes that met the frame's last one */
    int sweep_count() const { int32_t c; memcpy(&c, flag + tail_ofs + sizeof(sdv_v2d_state), sizeof(c)); return (int)c; }
    uint32_t frames_met() const { int32_t met; memcpy(&met, flag + tail_ofs + sizeof(sdv_v2d_state) + 4, sizeof(met)); return (uint32_t)met; }

    int prepare_memo()
    {
        if (memo_ready) return SDV_OK;
        { const int mrc = ensure_memo_capacity(e, (size_t)n, (size_t)height); if (mrc != SDV_OK) return mrc; }
        RT_CHECK(rt::dfill_bytes(e->d_memo_head, 0xFF, (size_t)n * (size_t)height * sizeof(int32_t), s));
        RT_CHECK(rt::dfill_bytes(d_count, 0, 16, s));
        RT_CHECK(rt::dfill_bytes(e->d_bw_memo, 0, (size_t)n * (size_t)height * sizeof(unsigned long long), s));
        a.bw_memo = e->d_bw_memo;
        const bool plain_now = e->plain_general && (e->plain_calls % 8u) != 7u;
        if ((size_t)n * 2 * sdv::TC_ENTRIES <= e->d_tc_snaps.cap && !dev_env("SDV_NO_TC") && !plain_now) {
            RT_CHECK(rt::dfill_bytes(e->d_tc_hdr, 0, (size_t)n * 2 * sizeof(uint32_t), s));        /* no frame has a complete pass yet */
            a.tc_snaps = e->d_tc_snaps; a.tc_hdr = e->d_tc_hdr; a.tc_keys = e->d_tc_keys;
        }
        a.memo = e->d_memo; a.memo_head = e->d_memo_head; a.memo_count = d_count; a.memo_cap = (int32_t)e->d_memo.cap;
        memo_ready = true; memo_done = 0;
        return SDV_OK;
    }

    /* settle what the last round asked for; count = requests handed out so far (read back with the flags) */
    int settle_sweeps(int count)
    {
        if (!memo_ready) return SDV_OK;
        const int cap = (int)e->d_memo.cap, have = count < cap ? count : cap;
        sweeps_seen = count;
        if (round_fat) {            /* settled where they were asked for */
            round_fat = false;
            if (have > memo_done) { e->info.sweeps += (uint32_t)(have - memo_done); memo_done = have; }
        }
        if (have > memo_done) {
            sdv::SweepArgs sa;
            memset(&sa, 0, sizeof(sa));
            sa.luma = a.luma; sa.frame_stride = a.frame_stride; sa.row_stride = a.row_stride; sa.width = a.width;
            sa.doubled = a.doubled; sa.mode = a.mode; sa.preset = a.preset;
            { const int src = settle_sweep_chunks(e, sa, memo_done, have, s); if (src != SDV_OK) return src; }
            e->info.sweeps += (uint32_t)(have - memo_done);
        }
        memo_done = have;
        if (count > cap) {
            /* the pool ran over: the requests that did not fit were dropped (their frames come again and ask again) - a bigger pool for them */
            rt::DevBuf<sdv::SweepMemo> bigger;      /* (the one buffer that grows with its contents; an early return frees it) */
            RT_CHECK(bigger.reserve((size_t)count + (size_t)count / 2 + 4096));
            RT_CHECK(rt::d2d(bigger, e->d_memo, (size_t)cap * sizeof(sdv::SweepMemo), s));
            RT_CHECK(rt::ssync(s));
            e->d_memo.swap(bigger);
            const int32_t c32 = cap;
            RT_CHECK(rt::h2d(d_count, &c32, sizeof(c32), s));
            RT_CHECK(rt::ssync(s));                 /* (the copy's source is on this stack frame) */
            a.memo = e->d_memo; a.memo_cap = (int32_t)e->d_memo.cap;
        }
        return SDV_OK;
    }

    /* One scheduling round is the lean kernel over a range or a list and the full kernel over a range or a list, timed together: begin_round, the
     * launches, end_round. */
    int begin_round(bool with_full)
    {
        if (e->profiling) RT_CHECK(e->timer.start(s));
        return with_full ? prepare_memo() : SDV_OK;
    }
    int end_round(uint32_t launched, uint32_t general)
    {
        if (e->profiling) { RT_CHECK(e->timer.stop(s)); timing_pending = true; }       /* read after the next synchronising copy */
        /* the last frame's outgoing state travels with the flags: one read-back per round (the frame writes it there itself, v2d_store_state) */
        e->info.rounds++; e->info.frames_launched += launched; e->info.frames_general += general;
        return SDV_OK;
    }
    /* the frames [lo, hi), all of them through the lean kernel or all of them through the full one */
    int run_round_range(int lo, int hi, bool full)
    {
        { const int rc = begin_round(full); if (rc != SDV_OK) return rc; }
        a.frame_list = NULL; a.frame_lo = lo; a.frame_hi = hi;
        /* (the cold chain's first frame: the kernel that settles the sweeps it asks for itself - see run_round_lists.  Not for a short call whose frames ALL
         * ask for sweeps, ten each: those are better settled side by side - 400 PAL frames 7.7 against 8.4 ms) */
        const bool fat = full && memo_ready && cold_frame && hi - lo == 1 && !dev_env("SDV_NO_FAT");
        if (fat) { a.fat_levels = e->d_sweep_levels; round_fat = true; }
        dev_count_frames(e, a, !full, hi - lo);
        RT_CHECK(launch_frames(a, s, !full));
        a.fat_levels = NULL;
        return end_round((uint32_t)(hi - lo), full ? (uint32_t)(hi - lo) : 0u);
    }
    /* The lists of a round go to the device through the page-locked staging e->h_lists, five slots of n ints: every round ends with a synchronising
     * read-back before the next lists are made, so the staging is free again by then.
     *   slots 0-1   the lean list, the full list behind it     one copy, to d_list_lean        (run_round_lists)
     *   slots 2-4   anchors, level patches, first_of, packed   one copy, to d_anchors          (upload_round_lists) */
    int *staged_frame_lists() const { return e->h_lists; }
    int *staged_round_lists() const { return e->h_lists + 2 * (size_t)n; }
    /* the frames of list_lean through the lean kernel, those of list_full through the full one */
    int run_round_lists(const std::vector<int> &list_lean, const std::vector<int> &list_full)
    {
        { const int rc = begin_round(!list_full.empty()); if (rc != SDV_OK) return rc; }
        uint32_t launched = 0, general = 0;
        if (!list_lean.empty() || !list_full.empty()) {
            int *h = staged_frame_lists();
            if (!list_lean.empty()) memcpy(h, list_lean.data(), list_lean.size() * sizeof(int));
            if (!list_full.empty()) memcpy(h + list_lean.size(), list_full.data(), list_full.size() * sizeof(int));
            RT_CHECK(rt::h2d(e->d_list_lean, h, (list_lean.size() + list_full.size()) * sizeof(int), s));
        }
        if (!list_lean.empty()) {
            a.frame_list = e->d_list_lean;
            dev_count_frames(e, a, true, (int)list_lean.size());
            RT_CHECK(launch_frames(a, s, true, (int)list_lean.size()));
            launched += (uint32_t)list_lean.size();
        }
        if (!list_full.empty()) {
            a.frame_list = e->d_list_lean + list_lean.size();
            /* A small round on a tape whose lines ask for sweeps: the kernel that settles them while the frame waits (sdv_k_stc007_frames_fat) - no round
             * for the frame to come again with the outcome at hand.  (The first rounds of a damaged tape are not small, and their thousands of sweeps are
             * better settled all at once: the machine is full of them.) */
            const bool fat = memo_ready && sweeps_seen > 0 && list_full.size() <= (e->d_sweep_levels.cap / 256 < 512 ? e->d_sweep_levels.cap / 256 : (size_t)512) && !dev_env("SDV_NO_FAT");
            if (fat) { a.fat_levels = e->d_sweep_levels; round_fat = true; }
            dev_count_frames(e, a, false, (int)list_full.size());
            RT_CHECK(launch_frames(a, s, false, (int)list_full.size()));
            a.fat_levels = NULL;
            launched += (uint32_t)list_full.size(); general += (uint32_t)list_full.size();
        }
        a.frame_list = NULL;
        return end_round(launched, general);
    }

    int resolve_timing()
    {
        if (timing_pending) {
            float ms = 0.f;
            RT_CHECK(e->timer.elapsed_ms(&ms));
            e->info.kernel_ms += ms;        /* (the call's rounds add up) */
            timing_pending = false;
        }
        return SDV_OK;
    }

    /* A round's one read-back: every frame of [first, n) has written how it left the chain (stc007_device.h, v2d_store_state); the last state and the
     * counts come with them.  ahead (the fused entry's first round): the read-back, then the work of the stage behind, and the host waits for the
     * read-back only. */
    int read_flags(int first, const FusedHooks *ahead = NULL)
    {
        const size_t bytes = tail_ofs + tail_bytes - (size_t)first;
        if (!ahead) {
            RT_CHECK(rt::d2h_pinned(flag + first, e->d_flag + first, bytes, s));
            return SDV_OK;
        }
        RT_CHECK(rt::d2h_async(flag + first, e->d_flag + first, bytes, s));
        RT_CHECK(rt::record(e->mark, s));
        const int rc = ahead->after_first_round(ahead->after_ctx);
        /* (the flags' read-back is in flight into h_flag, and the stage behind may have queued kernels that write the caller's buffers: an error return
         * waits for all of it - the caller may free or reuse its memory the moment the call is back) */
        if (rc != SDV_OK) { (void)rt::ssync(s); return rc; }
        const rt::status_t ev_rc = rt::wait_host(e->mark);
        if (ev_rc != rt::OK) { (void)rt::ssync(s); set_error(e, std::string("rt::wait_host(e->mark): ") + rt::err_str(ev_rc)); return SDV_ERR_HIP; }
        return rc;
    }
    /* A cold chain cannot be predicted: its first frame is decoded alone, with the full kernel (again while sweeps are owed to it: nothing is tuned, the
     * first lines go through the reference-level sweep); what it hands on is what frame 1 starts from. */
    int decode_cold_frame()
    {
        cold_frame = true;
        for (int pass = 0;; pass++) {
            if (pass > 2 * height + 16) { set_error(e, "the sweeps of the first frame did not settle"); return SDV_ERR_HIP; }
            int rc = run_round_range(0, 1, true); if (rc != SDV_OK) return rc;
            rc = read_flags(0); if (rc != SDV_OK) return rc;
            rc = resolve_timing(); if (rc != SDV_OK) return rc;
            rc = settle_sweeps(sweep_count()); if (rc != SDV_OK) return rc;
            if ((flag[0] & sdv::VF_KIND) != sdv::VF_ABORTED) break;
        }
        cold_frame = false;
        if (n > 1) RT_CHECK(rt::d2d(&e->d_states_in[1], &e->d_states_out[0], sizeof(sdv_v2d_state), s));
        return SDV_OK;
    }

    /* the give-up signatures of the frames, behind the block read_flags brings */
    int read_signatures(const uint8_t **sig)
    {
        RT_CHECK(rt::d2h_pinned(flag + sig_ofs, e->d_flag + sig_ofs, (size_t)n, s));
        *sig = flag + sig_ofs;
        return SDV_OK;
    }

    /* the round's three small lists in one copy: anchors, then the level patches, then first_of (staging slots 2-4); where they lie on the device */
    struct RoundLists { int *anchors; uint32_t *patches; int *first_of; };
    int upload_round_lists(const ChainPlan &p, RoundLists *d)
    {
        static_assert(sizeof(uint32_t) == sizeof(int), "one staging area for the three lists");
        const std::vector<int> &anchors = p.anchors, &first_of = p.first_of; const std::vector<uint32_t> &patches = p.patches;
        int *h = staged_round_lists();          /* every list holds at most n */
        if (!anchors.empty()) memcpy(h, anchors.data(), anchors.size() * sizeof(int));
        if (!patches.empty()) memcpy(h + anchors.size(), patches.data(), patches.size() * sizeof(uint32_t));
        if (!first_of.empty()) memcpy(h + anchors.size() + patches.size(), first_of.data(), first_of.size() * sizeof(int));
        int *const d_anch = e->d_anchors;
        RT_CHECK(rt::h2d(d_anch, h, (anchors.size() + patches.size() + first_of.size()) * sizeof(int), s));
        d->anchors = d_anch; d->patches = reinterpret_cast<uint32_t *>(d_anch + anchors.size()); d->first_of = d_anch + anchors.size() + patches.size();
        return SDV_OK;
    }

    /* The states the round's frames start from, made on the device: the anchors take what their predecessors really handed on, patched levels are
     * written in, the frames behind the anchors are predicted from them, the history moves on along the chain - and the frames it reaches join the round. */
    int start_states(ChainPlan &p, bool use_skip, bool trace)
    {
        const int first = p.first, hi = p.hi;
        RoundLists d;
        { const int rc = upload_round_lists(p, &d); if (rc != SDV_OK) return rc; }
        sdv::AnchorArgs aa; aa.states_in = e->d_states_in; aa.states_out = e->d_states_out; aa.list = d.anchors; aa.n = (int)p.anchors.size(); aa.flag = e->d_flag;
        RT_CHECK(RT_LAUNCH_ITEMS(sdv_k_anchor, sdv::anchor_body, 0, aa.n, 256, s, aa));
        if (!p.patches.empty()) {
            sdv::RefPatchArgs ra; ra.states_in = e->d_states_in; ra.patch = d.patches; ra.n = (int)p.patches.size();
            RT_CHECK(RT_LAUNCH_ITEMS(sdv_k_ref_patch, sdv::ref_patch_body, 0, ra.n, 256, s, ra));
        }
        pa.first = first; pa.hi = hi; pa.first_of = d.first_of;
        if (use_skip) { RT_CHECK(rt::dfill_bytes(e->d_skip + first, 0, (size_t)(hi - first), s)); pa.skip = e->d_skip; }
        RT_CHECK(launch_predict(pa, s));
        pa.skip = NULL;
        if (p.any_moved && !p.anchors.empty() && !dev_env("SDV_SCHED_NO_CARRY")) {     /* the history moves on (sdv_k_hist_carry): frames it reaches are decoded in this round too */
            RT_CHECK(rt::dfill_bytes(e->d_patched + first, 0, (size_t)(hi - first), s));
            sdv::HistCarryArgs ha; ha.states_in = e->d_states_in; ha.refs = e->d_refs; ha.anchors = d.anchors; ha.n_anchors = (int)p.anchors.size(); ha.hi = hi; ha.patched = e->d_patched; ha.skip = use_skip ? e->d_skip.p : NULL;
            RT_CHECK(RT_LAUNCH_ITEMS(sdv_k_hist_carry, sdv::hist_carry_body, 0, ha.n_anchors, 64, s, ha));
            RT_CHECK(rt::d2h_pinned(e->h_patched + first, e->d_patched + first, (size_t)(hi - first), s));
            const size_t reached = p.add_carried(e->h_patched);
            if (trace) fprintf(stderr, "[sched]   the history moved on into %zu more frames\n", reached);
        }
        return SDV_OK;
    }

    /* developer aid (SDV_SCHED_TRACE): what the plan made of the round's flags, and what the first broken link disagrees on */
    int trace_round(const ChainPlan &p, unsigned iter)
    {
        const int b0 = p.b0;
        if (b0 >= 0 && b0 + 1 < n) {
            sdv_v2d_state so, si;
            RT_CHECK(rt::d2h(&so, &e->d_states_out[b0], sizeof(so), s)); RT_CHECK(rt::d2h(&si, &e->d_states_in[b0 + 1], sizeof(si), s));
            const uint32_t *x = (const uint32_t *)&so, *y = (const uint32_t *)&si;
            for (unsigned i = 0; i < sizeof(so) / 4; i++) if (x[i] != y[i]) fprintf(stderr, "[sched]   link %d: dword %u out %08x, next frame started from %08x\n", b0, i, x[i], y[i]);
        }
        int nch = 0;
        for (int k = p.first; k < n; k++) if (p.kind[(size_t)k] == sdv::VF_BREAK) nch += p.changed[(size_t)k];
        fprintf(stderr, "[sched]   of the broken links: %d behind frames that only re-tuned their levels\n", nch);
        fprintf(stderr, "[sched] iter %u first %d: %zu given up (%d crowd leaders), %d breaks (first at %d); %u frame decodes, %.3f ms in kernels so far\n", iter, p.first, p.list_full.size(), p.n_leaders, p.n_break, b0, e->info.frames_launched, e->info.kernel_ms);
        return SDV_OK;
    }
};

/* hooks: the fused entry's hand-over for this one call, NULL from everybody else */
static int stc007_binarize_frames_impl(sdv_engine *e, const uint8_t *luma, size_t row_stride, size_t frame_stride, int width, int height,
                                       int n_frames, uint32_t first_frame_no, unsigned flags, sdv_line_rec *out_lines, size_t lines_cap,
                                       sdv_frame_stats *out_stats, size_t stats_cap, void *stream, const FusedHooks *hooks)
{
    if (!e) return SDV_ERR_BAD_ARG;
    FrameFlagsConsumed flags_consumed(e);
    int rc = check_frame_call(e, luma, out_lines, out_stats, row_stride, frame_stride, width, height, n_frames, flags, lines_cap, stats_cap,
                              SDV_MAX_WIDTH, sdv::BITS_IN_LINE, "line shorter than the 137 bit cells of an STC-007 line", sdv_binarize_records(height, n_frames, flags), "line records");
    if (rc != SDV_OK) return rc;
    rt::stream_t s = (rt::stream_t)stream;
    SDV_ON_DEVICE(e);
    const int n_real = n_frames;
    if (flags & SDV_FLAG_END_FILE) n_frames++;          /* the filler frame is decoded like any other frame of the chain */
    rc = ensure_capacity(e, (size_t)n_frames, (size_t)height);
    if (rc != SDV_OK) return rc;
    const int n = n_frames;
    Stc007FrameCall c(e, s, n, height);
    rc = c.set_arguments(luma, row_stride, frame_stride, width, first_frame_no, flags, n_real, out_lines, out_stats, hooks); if (rc != SDV_OK) return rc;
    sdv::FrameArgs &a = c.a;
    sdv::PredictArgs &pa = c.pa;

    memset(&e->info, 0, sizeof(e->info));
    dev_reset_counts(e);
    e->info.frames = (uint32_t)n_frames;
    /* A stream that plays (the chain is tuned, the last call's frames did not need the full kernel): the waves of the first round make the state they start
     * from themselves, from the one state that is known (FrameArgs::predict_in_kernel) - no copy and no kernel in front of the frame kernel.  The states go to
     * the device the usual way (copy + sdv_k_predict) when that round was not the last. */
    const bool cold = e->chain.bin.in_def_reference < e->preset.min_ref_lvl || e->chain.reset_stats;       /* nothing tuned yet */
    bool states_owed = !cold && !e->worn_tape && !dev_env("SDV_NO_PREDICT_IN_KERNEL");
    if (!states_owed) RT_CHECK(rt::h2d(e->d_states_in, &e->chain, sizeof(sdv_v2d_state), s));

    uint8_t *const flag = c.flag;
    ChainPlan plan;
    int first = 0;          /* frames below are final */
    if (cold) { rc = c.decode_cold_frame(); if (rc != SDV_OK) return rc; first = 1; }
    /* first pass over everything: predicted from the one state that is known, lean kernel - unless the last call on this stream had to give most of
     * its frames to the full kernel (a tape with damage in every frame): then the lean kernel would only give them all up again, twice (once as a
     * crowd, once after the crowd's first frame), and the frames go to the full kernel at once */
    const bool worn = e->worn_tape && !cold;
    if (first < n) {
        pa.first = first; pa.hi = n; pa.first_of = NULL;
        if (states_owed) { a.predict_in_kernel = 1; a.base_frame = first; a.base = e->chain; }
        else RT_CHECK(launch_predict(pa, s));
        rc = c.run_round_range(first, n, worn); if (rc != SDV_OK) return rc;
        a.predict_in_kernel = 0;
    }
    plan.begin(n, first, worn);         /* (the call's per-frame vectors: made while the first round runs) */
    bool have_tail = false;
    const bool trace = dev_env("SDV_SCHED_TRACE") != NULL;        /* developer aid */
    for (unsigned iter = 0; plan.first < n; iter++) {
        if (iter > 4u * (unsigned)n + 16u) { set_error(e, "chain speculation did not settle"); return SDV_ERR_HIP; }
        rc = c.read_flags(plan.first, iter == 0 && hooks && hooks->after_first_round ? hooks : NULL); if (rc != SDV_OK) return rc;
        have_tail = true;
        rc = c.resolve_timing(); if (rc != SDV_OK) return rc;
        if (c.memo_ready) {
            const int before = c.memo_done;
            rc = c.settle_sweeps(c.sweep_count()); if (rc != SDV_OK) return rc;
            if (c.memo_done > before && iter > 0) iter--;         /* (a round that only waited for sweeps is not one the speculation failed in) */
        }
        if (!trace && ChainPlan::all_links_hold(flag, plan.first, n)) { plan.rest_ran_lean(); break; }
        if (states_owed) {      /* the round was not the last: what its waves were started from, for the kernels and the book-keeping of the rounds behind it */
            states_owed = false;
            RT_CHECK(rt::h2d(e->d_states_in, &e->chain, sizeof(sdv_v2d_state), s));
            pa.first = 0; pa.hi = n; pa.first_of = NULL;
            RT_CHECK(launch_predict(pa, s));
        }
        plan.take_flags(flag);
        plan.release_crowds();
        plan.collect_given_up_and_breaks();
        const uint8_t *sig = NULL;
        if (plan.some_crowd_is_fresh() && !dev_env("SDV_SCHED_NO_SIG")) { rc = c.read_signatures(&sig); if (rc != SDV_OK) return rc; }
        plan.pick_leaders(sig);
        if (trace) { rc = c.trace_round(plan, iter); if (rc != SDV_OK) return rc; }
        /* given-up frames first: the full kernel decodes them from the states they have */
        if (!plan.list_full.empty()) { rc = c.run_round_lists(plan.list_lean, plan.list_full); if (rc != SDV_OK) return rc; continue; }
        if (!plan.advance()) break;                             /* the whole chain holds */
        if (plan.level_break && !dev_env("SDV_SCHED_NO_PASS")) {
            RT_CHECK(rt::d2h_pinned(e->h_refs, e->d_refs, 3 * (size_t)n, s));
            plan.carry_levels(e->h_refs);
            if (trace) fprintf(stderr, "[sched]   a level carried on into %zu frames\n", plan.patches.size());
        }
        plan.build_segments();
        const bool use_skip = !dev_env("SDV_SCHED_NO_SKIP");
        rc = c.start_states(plan, use_skip, trace); if (rc != SDV_OK) return rc;
        a.skip = use_skip ? e->d_skip.p : NULL;
        if (!plan.any_hard && plan.contiguous) rc = c.run_round_range(plan.run_lo, plan.run_hi, false);
        else rc = c.run_round_lists(plan.list_lean, plan.list_full);
        a.skip = NULL;
        if (rc != SDV_OK) return rc;
    }
    if (have_tail && c.memo_ready) e->info.frames_met = c.frames_met();     /* (behind the count of sweep requests) */
    plan.judge_tape(cold, c.memo_ready, a.tc_hdr != NULL, e->info.frames_general, e->info.frames_met, e->worn_tape, e->plain_general, e->plain_calls);
    if (have_tail) memcpy(&e->chain, flag + c.tail_ofs, sizeof(sdv_v2d_state));     /* came with the flags of the round that settled the chain */
    else { RT_CHECK(rt::d2h(&e->chain, &e->d_states_out[n_frames - 1], sizeof(sdv_v2d_state), s)); rc = c.resolve_timing(); if (rc != SDV_OK) return rc; }
    return SDV_OK;
}

extern "C" int sdv_binarize_frames(sdv_engine *e, const uint8_t *luma, size_t row_stride, size_t frame_stride, int width, int height,
                                   int n_frames, uint32_t first_frame_no, unsigned flags, sdv_line_rec *out_lines, size_t lines_cap,
                                   sdv_frame_stats *out_stats, size_t stats_cap, void *stream)
{
    return stc007_binarize_frames_impl(e, luma, row_stride, frame_stride, width, height, n_frames, first_frame_no, flags, out_lines, lines_cap, out_stats, stats_cap, stream, NULL);
}
