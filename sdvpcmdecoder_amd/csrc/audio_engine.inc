/*
 * audio_engine.inc - host side of sdv_audio_process / sdv_wav_pack / sdv_wav_header (include/sdvpcm.h): the reference's
 * AudioProcessor and the bytes of SamplesToWAV.  Included after pcm16_engine.inc by the same two translation units (product: HIP;
 * tests: SIMT emulator).
 * A call is: tag positions (one launch + a read-back of a few bytes), the stretch table (host: the tags split the burst into
 * stretches that each start from a purged window), prepare (work array + bitmaps) and the bitmap summary, the plan (one wave per
 * stretch, bitmaps only), a read-back of the per-stretch results, the sample work of the listed windows, a second read-back (mask
 * counts, the plan check), and - unless the caller's buffer was the work array - emit.  The stream state - what waits in the window,
 * the masking mode, the running sample index - is replaced only when the call succeeds.  sdv_audio_deemphasis (two launches,
 * nothing read back), sdv_audio_resample (three launches, with a delay bit a fourth, the count read back once) and sdv_decode_frames (the workers of
 * a format back to back)
 * live here too, this being the last include of both builds.
 */
#include <algorithm>

struct sdv_audio {
    /* (made by new sdv_audio(): everything that is not a buffer starts as zero) */
    int mask_mode;
    rt::DevBuf<sdv_sample_pair> d_carry, d_carry_spare, d_carry_snap; uint32_t n_carry;    /* what waits in the window (at most 512 pairs each) */
    uint64_t next_index;            /* PCMSample::index of the next pair that leaves */
    bool stalled;                   /* the window is full and its first pairs can never leave: the worker takes no more input (audioprocessor.cpp:108) */
    rt::DevBuf<uint32_t> d_count; rt::DevBuf<uint64_t> d_tags;
    rt::DevBuf<sdva::Stretch> d_st; rt::DevBuf<sdva::StretchResult> d_res;
    rt::DevBuf<sdv_sample_pair> d_w;
    rt::DevBuf<uint64_t> d_bad1, d_bad3, d_v0, d_v1, d_m0, d_m1;
    rt::DevBuf<uint8_t> d_bad2;
    rt::DevBuf<sdva::WinRec> d_wins; rt::DevBuf<uint32_t> d_win_base;
    /* sdv_decode_frames: what passes from stage to stage */
    rt::DevBuf<uint8_t> d_chain_recs; rt::DevBuf<sdv_frame_stats> d_chain_stats; rt::DevBuf<sdv_sample_pair> d_chain_pairs;
    /* sdv_audio_deemphasis: the mode, the filter between two calls (on the device; de_idle: not looked at, the next call starts idle), a record per tile */
    int de_mode; bool de_idle;
    rt::DevBuf<sdva::DeState> d_de_state, d_de_tiles;
    /* sdv_audio_resample: the mode; the open segment between two calls - pairs seen, outputs emitted, its last RS_HIST pairs (on the device) -;
     * the tap table ([k][phase], made on first use), a summary and a start per tile, the call's result */
    int rs_mode; uint64_t rs_seen, rs_emitted; bool rs_taps_ready;
    rt::DevBuf<sdv_sample_pair> d_rs_hist, d_rs_hist_spare;
    rt::DevBuf<double> d_rs_taps;
    rt::DevBuf<sdva::RsSum> d_rs_sums; rt::DevBuf<sdva::RsStart> d_rs_starts; rt::DevBuf<sdva::RsResult> d_rs_result;
    /* ... its skew stage (a delay bit in rs_mode): the pairs its open segment has seen (SK_MANY: more than its history holds), its last SK_HIST
     * pairs (on the device), the half-sample row, the resampler's output where the stage follows it, the call's result */
    uint32_t sk_seen; bool sk_taps_ready;
    rt::DevBuf<sdv_sample_pair> d_sk_hist, d_sk_hist_spare, d_sk_mid;
    rt::DevBuf<double> d_sk_taps;
    rt::DevBuf<sdva::SkResult> d_sk_result;
};

static sdv_audio *audio_get(sdv_engine *e)
{
    if (e->audio) return e->audio;
    sdv_audio *t = new sdv_audio();
    t->mask_mode = SDV_DROP_IGNORE;     /* the constructor's DROP_IGNORE (audioprocessor.cpp:15) */
    t->de_mode = SDV_DEEMPH_OFF; t->de_idle = true;
    t->rs_mode = SDV_RESAMPLE_OFF;
    e->audio = t;
    return t;
}
static void audio_free(sdv_engine *e)
{
    sdv_audio *t = e->audio;
    if (!t) return;
    delete t;
    e->audio = NULL;
}

extern "C" {

int sdv_set_audio_masking(sdv_engine *e, int drop_mode)
{
    if (!e) return SDV_ERR_BAD_ARG;
    const bool cubic = drop_mode == SDV_DROP_INTER_CUBIC_BLOCK || drop_mode == SDV_DROP_INTER_CUBIC_WORD;      /* (no reference equivalent) */
    if ((drop_mode < 0 || drop_mode >= SDV_DROP_MAX) && !cubic) { set_error(e, "no such masking mode"); return SDV_ERR_BAD_ARG; }     /* setMasking ignores it (:1534) */
    audio_get(e)->mask_mode = drop_mode;
    return SDV_OK;
}

int sdv_reset_audio(sdv_engine *e)
{
    if (!e) return SDV_ERR_BAD_ARG;
    sdv_audio *t = audio_get(e);
    t->n_carry = 0; t->next_index = 0; t->stalled = false;
    return SDV_OK;
}

size_t sdv_audio_pending(const sdv_engine *e) { return e && e->audio ? e->audio->n_carry : 0; }
int sdv_audio_stalled(const sdv_engine *e) { return e && e->audio && e->audio->stalled ? 1 : 0; }
uint64_t sdv_audio_next_index(const sdv_engine *e) { return e && e->audio ? e->audio->next_index : 0; }

} // extern "C"

/* One span of a call: the worker's turns over pairs[0, n_pairs) with the queue running dry behind them.  `split_at`: set to the position
 * of an END_FILE tag that finds fewer than three pairs in the window when there is one - the span then ends in front of it (see
 * sdv_audio_process) - else to n_pairs.  Purge records go out with `out_base` / `in_base` added. */
static int audio_process_span(sdv_engine *e, sdv_audio *t, const sdv_sample_pair *pairs, size_t n_pairs, int stop, sdv_sample_pair *out_pairs, size_t out_cap,
                              size_t *n_out, sdv_audio_purge *out_purges, size_t purges_cap, size_t *n_purges, uint64_t *n_masked, rt::stream_t s,
                              uint64_t out_base, uint32_t in_base, size_t *split_at, bool purge_only)
{
    *n_out = 0; *n_purges = 0; *n_masked = 0; *split_at = n_pairs;

    /* 1. the tags */
    std::vector<uint64_t> tags;
    if (n_pairs > 0) {
        RT_CHECK(rt::dfill_bytes(t->d_count, 0, 4 * sizeof(uint32_t), s));
        sdva::TagArgs ta; ta.pairs = pairs; ta.n = (uint32_t)n_pairs; ta.count = t->d_count; ta.list = t->d_tags;
        RT_LAUNCH64(sdv_k_ap_tags, (n_pairs + 1023) / 1024, ta, s);
        uint32_t n_tags = 0;
        RT_CHECK(rt::d2h(&n_tags, t->d_count, sizeof(uint32_t), s));
        if (n_tags > (uint32_t)sdva::MAX_TAGS) { set_error(e, "more than 65536 service tags in one burst"); return SDV_ERR_UNSUPPORTED; }
        tags.resize(n_tags);
        if (n_tags) RT_CHECK(rt::d2h(tags.data(), t->d_tags, n_tags * sizeof(uint64_t), s));
        std::sort(tags.begin(), tags.end());
    }

    /* 2. the stretches between the purges, their places in W and in the output */
    std::vector<sdva::Stretch> st;
    std::vector<sdv_audio_purge> purges;
    {
        sdva::Stretch cur; memset(&cur, 0, sizeof(cur));
        cur.head = t->n_carry; cur.head_is_carry = 1; cur.in_start = 0;
        uint64_t w_pos = 0, o_pos = 0;
        auto close = [&](uint32_t data_end, uint8_t end_kind) {
            cur.v_len = cur.head + (data_end - cur.in_start); cur.end_kind = end_kind; cur.stop = (end_kind == sdva::END_OPEN && stop) ? 1 : 0;
            cur.w_base = (uint32_t)w_pos; cur.out_base = o_pos;
            st.push_back(cur);
            w_pos += cur.v_len;
        };
        for (uint64_t tg : tags) {
            const uint32_t pos = (uint32_t)(tg >> 8); const uint8_t kind = (uint8_t)(tg & 0xFF);
            if (kind != SDV_PAIR_SRV_NEW_FILE && kind != SDV_PAIR_SRV_END_FILE) {
                set_error(e, "sample pair " + std::to_string(pos) + " carries a service tag that is neither NEW_FILE nor END_FILE");
                return SDV_ERR_UNSUPPORTED;
            }
            if (kind == SDV_PAIR_SRV_END_FILE && cur.head + (pos - cur.in_start) < (uint32_t)sdva::KEEP) {
                /* an END_FILE that finds fewer than three pairs in the window: outputAudio returns before the purge (:1298-1301), the
                 * file goes on.  The turn ends at the tag all the same, so the span ends here, open, and the caller deals with the window. */
                *split_at = pos; n_pairs = pos; stop = 0;
                break;
            }
            close(pos, kind == SDV_PAIR_SRV_NEW_FILE ? sdva::END_NEW_FILE : sdva::END_END_FILE);
            o_pos += cur.v_len > 0 ? cur.v_len - 1 : 0;         /* the purge puts out everything but the last pair */
            sdv_audio_purge p; memset(&p, 0, sizeof(p));
            p.first_pair = o_pos; p.tag_index = pos; p.kind = kind == SDV_PAIR_SRV_NEW_FILE ? SDV_AP_PURGE_NEW_FILE : SDV_AP_PURGE_END_FILE;
            purges.push_back(p);
            memset(&cur, 0, sizeof(cur));
            cur.head = 1; cur.head_is_carry = 0; cur.in_start = pos + 1;
        }
        close((uint32_t)n_pairs, sdva::END_OPEN);
        if (w_pos >= 0x7FFFFFFFull) { set_error(e, "too many sample pairs in one call"); return SDV_ERR_BAD_ARG; }
    }
    size_t n_st = st.size();
    uint32_t total_w = st.back().w_base + st.back().v_len;
    bool stalled = false; int stop_here = stop;
    const int mode = t->mask_mode;
    const bool ignore = mode == SDV_DROP_IGNORE;

    uint64_t total_out = st.back().out_base, masked = 0;
    uint32_t left = 0, carry_from = 0;
    sdv_sample_pair *work = NULL; bool is_direct = false;
    if (total_w > 0) {
        RT_CHECK(rt::reserve_all(n_st, n_st + n_st / 2 + 16, t->d_st, t->d_res));
        /* The work array.  Where every stretch that can put something out lies at the same index in the work array as in the output - a
         * burst that continues or holds one file, the streaming case: only a purge that drops a pair shifts what follows it - the caller's
         * buffer is the work array and the emit pass falls away (the pairs cross HBM once in each direction); else a buffer of the engine. */
        bool direct = !ignore && out_pairs && out_cap >= (size_t)total_w;
        if (direct && pairs && (const char *)pairs < (const char *)(out_pairs + out_cap) && (const char *)out_pairs < (const char *)(pairs + n_pairs))
            direct = false;         /* input and output overlap (a call in place): the input has to be read before anything is written */
        for (size_t k = 0; k < n_st && direct; k++) if (st[k].v_len > 1 && (uint64_t)st[k].w_base != st[k].out_base) direct = false;
        if (!direct) RT_CHECK(t->d_w.reserve((size_t)total_w, (size_t)total_w + total_w / 8 + 4096));
        work = direct ? out_pairs : t->d_w.p; is_direct = direct;
        const size_t n1 = ((size_t)total_w + 63) / 64, n2 = (n1 + 63) / 64, n3 = (n2 + 63) / 64;
        {
            const size_t c = n1 + n1 / 8 + 64;
            RT_CHECK(rt::reserve_all(n1, c, t->d_bad1, t->d_v0, t->d_v1, t->d_m0, t->d_m1));
            RT_CHECK(t->d_bad2.reserve((n1 + 63) / 64 * 64 + 64, (c + 63) / 64 * 64 + 64)); RT_CHECK(t->d_bad3.reserve((n1 + 4095) / 4096 + 1, (c + 4095) / 4096 + 1));
        }
        /* the window lists: a full window that does not stall puts out at least MIN_ADVANCE pairs */
        std::vector<uint32_t> win_base(n_st + 1);
        size_t n_slots = 0;
        for (size_t k = 0; k < n_st; k++) { win_base[k] = (uint32_t)n_slots; n_slots += st[k].v_len / (size_t)sdva::MIN_ADVANCE + 2; }
        win_base[n_st] = (uint32_t)n_slots;
        RT_CHECK(t->d_wins.reserve(n_slots, n_slots + n_slots / 8 + 64));
        RT_CHECK(t->d_win_base.reserve(n_st + 1, n_st + 1 + n_st / 2 + 16));
        RT_CHECK(rt::h2d(t->d_win_base, win_base.data(), (n_st + 1) * sizeof(uint32_t), s));
        if (n_pairs == 0) RT_CHECK(rt::dfill_bytes(t->d_count + 1, 0, sizeof(uint32_t), s));    /* has_mi (zeroed with the tag counter otherwise) */
        RT_CHECK(rt::h2d(t->d_st, st.data(), n_st * sizeof(sdva::Stretch), s));
        RT_CHECK(rt::dfill_bytes(t->d_bad2, 0, n2 * 64, s));

        /* 3. W and the bitmap */
        sdva::PrepArgs pa; pa.pairs = pairs; pa.carry = t->d_carry; pa.st = t->d_st; pa.n_st = (uint32_t)n_st; pa.total_w = total_w; pa.w = work;
        pa.bad1 = t->d_bad1; pa.bad2 = t->d_bad2; pa.bad3 = t->d_bad3; pa.ignore = ignore ? 1 : 0;
        pa.v0 = t->d_v0; pa.v1 = t->d_v1; pa.m0 = t->d_m0; pa.m1 = t->d_m1; pa.has_mi = t->d_count + 1;
        pa.by_block = (mode == SDV_DROP_MUTE_BLOCK || mode == SDV_DROP_HOLD_BLOCK || mode == SDV_DROP_INTER_LIN_BLOCK || mode == SDV_DROP_INTER_CUBIC_BLOCK) ? 1 : 0;
        RT_LAUNCH64(sdv_k_ap_prepare, ((size_t)total_w + 255) / 256, pa, s);
        sdva::SummArgs sm; sm.bad2 = t->d_bad2; sm.n_blocks = (uint32_t)n2; sm.bad3 = t->d_bad3;
        RT_LAUNCH64(sdv_k_ap_summary, n3, sm, s);

        /* 4. the plan (one wave per stretch, bitmaps only), then the sample work of the listed windows (one wave per chain of windows) */
        sdva::PlanArgs la; la.st = t->d_st; la.n_st = (uint32_t)n_st; la.v0 = t->d_v0; la.v1 = t->d_v1; la.m0 = t->d_m0; la.m1 = t->d_m1;
        la.bad1 = t->d_bad1; la.bad2 = t->d_bad2; la.bad3 = t->d_bad3; la.has_mi = t->d_count + 1; la.n_words = (uint32_t)n1;
        la.wins = t->d_wins; la.win_base = t->d_win_base; la.res = t->d_res;
        std::vector<sdva::StretchResult> res(n_st);
        if (!purge_only) {
            RT_LAUNCH64(sdv_k_ap_plan, n_st, la, s);
            RT_CHECK(rt::d2h(res.data(), t->d_res, n_st * sizeof(sdva::StretchResult), s));
        } else {                                        /* stop() on a stalled worker: no turn runs, the window leaves as it is */
            memset(res.data(), 0, n_st * sizeof(sdva::StretchResult));
            RT_CHECK(rt::dfill_bytes(t->d_res, 0, n_st * sizeof(sdva::StretchResult), s));
        }
        size_t listed = 0;
        for (size_t k = 0; k < n_st; k++) {
            listed += res[k].n_win;
            if (res[k].flags & sdva::RES_STALLED) {
                /* A full window whose first pairs can never leave (invalid samples with nothing valid in front of them): the worker's fill loop
                 * no longer runs (:108), so nothing behind this window is ever taken - not the pairs, not the tags.  The stretch ends here,
                 * open, with the window waiting; stop() still purges it. */
                stalled = true;
                n_st = k + 1; st.resize(n_st); purges.resize(k);
                total_w = st.back().w_base + st.back().v_len; total_out = st.back().out_base; stop_here = 0;
                n_slots = win_base[n_st];
                st.back().end_kind = sdva::END_OPEN; st.back().stop = 0;
                RT_CHECK(rt::h2d(t->d_st, st.data(), n_st * sizeof(sdva::Stretch), s));
                break;
            }
        }
        if (listed > 0) {
            sdva::ExecArgs xa; xa.st = t->d_st; xa.n_st = (uint32_t)n_st; xa.w = work; xa.wins = t->d_wins; xa.win_base = t->d_win_base; xa.res = t->d_res;
            xa.n_slots = n_st == 1 ? res[0].n_win : (uint32_t)n_slots;
            xa.how = (mode == SDV_DROP_MUTE_BLOCK || mode == SDV_DROP_MUTE_WORD) ? sdva::HOW_MUTE : (mode == SDV_DROP_HOLD_BLOCK || mode == SDV_DROP_HOLD_WORD) ? sdva::HOW_HOLD :
                     (mode == SDV_DROP_INTER_CUBIC_BLOCK || mode == SDV_DROP_INTER_CUBIC_WORD) ? sdva::HOW_CUBIC : sdva::HOW_LIN;
            if (xa.how == sdva::HOW_CUBIC) RT_LAUNCH64(sdv_k_ap_windows_cubic, xa.n_slots, xa, s); else RT_LAUNCH64(sdv_k_ap_windows, xa.n_slots, xa, s);
            RT_CHECK(rt::d2h(res.data(), t->d_res, n_st * sizeof(sdva::StretchResult), s));
            for (size_t k = 0; k < n_st; k++) {
                masked += res[k].masked;
                if (res[k].flags & sdva::RES_PLAN_MISMATCH) { set_error(e, "internal: a window put out a different number of pairs than planned"); return SDV_ERR_HIP; }
            }
        }
        const sdva::Stretch &last = st.back();
        if (stop_here) { total_out += last.v_len > 0 ? last.v_len - 1 : 0; left = 0; }
        else { total_out += res[n_st - 1].popped; left = stalled ? (uint32_t)sdva::WIN : res[n_st - 1].left; carry_from = last.w_base + res[n_st - 1].popped; }
    }
    if (stop_here) {
        sdv_audio_purge p; memset(&p, 0, sizeof(p));
        p.first_pair = total_out; p.tag_index = (uint32_t)n_pairs; p.kind = SDV_AP_PURGE_STOP;
        purges.push_back(p);
    }
    *n_out = (size_t)total_out; *n_purges = purges.size();
    if (n_masked) *n_masked = masked;
    if (total_out > out_cap || purges.size() > purges_cap || (total_out > 0 && !out_pairs) || (!purges.empty() && !out_purges)) {
        set_error(e, "output buffers too small: " + std::to_string((unsigned long long)total_out) + " sample pairs and " + std::to_string(purges.size()) + " purge records are needed");
        return SDV_ERR_BAD_ARG;
    }

    /* 5. emit; what waits moves to the spare buffer and becomes the state */
    if (total_w > 0 && !is_direct) {
        sdva::EmitArgs ea; ea.st = t->d_st; ea.n_st = (uint32_t)n_st; ea.res = t->d_res; ea.w = t->d_w; ea.total_w = total_w; ea.out = out_pairs; ea.out_cap = out_cap;
        ea.carry_out = t->d_carry_spare; ea.ignore = ignore ? 1 : 0;
        RT_LAUNCH64(sdv_k_ap_emit, ((size_t)total_w + 255) / 256, ea, s);
    } else if (total_w > 0 && !stop_here && left > 0) {
        /* the output is in place already; what still waits is the tail of the open stretch (of a stalled one: the window) */
        RT_CHECK(rt::d2d(t->d_carry_spare, work + carry_from, (size_t)left * sizeof(sdv_sample_pair), s));
    }
    if (!purges.empty()) {
        for (sdv_audio_purge &p : purges) { p.first_pair += out_base; p.tag_index += in_base; }
        RT_CHECK(rt::h2d(out_purges, purges.data(), purges.size() * sizeof(sdv_audio_purge), s));
        for (sdv_audio_purge &p : purges) { p.first_pair -= out_base; p.tag_index -= in_base; }
    }
    if (stop_here) {
        /* purgePipeline leaves one silent pair in the window and the index at 1 (:1734-1744) */
        sdv_sample_pair q; memset(&q, 0, sizeof(q));
        q.sample_flags[0] = q.sample_flags[1] = SDV_SF_BLOCK_OK | SDV_SF_WORD_VALID; q.sample_rate = 44056;
        RT_CHECK(rt::h2d(t->d_carry_spare, &q, sizeof(q), s));
        left = 1;
    }
    RT_CHECK(rt::ssync(s));
    t->d_carry.swap(t->d_carry_spare);
    t->n_carry = left;
    t->stalled = stalled;
    if (stalled) *split_at = n_pairs;           /* nothing behind the window is looked at */
    if (!purges.empty()) t->next_index = total_out - purges.back().first_pair; else t->next_index += total_out;
    return SDV_OK;
}

extern "C" {

int sdv_audio_process(sdv_engine *e, const sdv_sample_pair *pairs, size_t n_pairs, int stop, sdv_sample_pair *out_pairs, size_t out_cap,
                      size_t *n_out, sdv_audio_purge *out_purges, size_t purges_cap, size_t *n_purges, uint64_t *n_masked, void *stream)
{
    if (!e || !n_out || !n_purges) return SDV_ERR_BAD_ARG;
    *n_out = 0; *n_purges = 0;
    if (n_masked) *n_masked = 0;
    if (n_pairs > 0 && !pairs) { set_error(e, "null sample pair buffer"); return SDV_ERR_NULL_LINES; }
    if (n_pairs >= 0x7FFF0000u) { set_error(e, "too many sample pairs in one call"); return SDV_ERR_BAD_ARG; }
    rt::stream_t s = (rt::stream_t)stream;
    SDV_ON_DEVICE(e);
    sdv_audio *t = audio_get(e);
    RT_CHECK(t->d_count.reserve(4));
    RT_CHECK(t->d_tags.reserve(sdva::MAX_TAGS));
    RT_CHECK(rt::reserve_all(sdva::WIN, sdva::WIN, t->d_carry, t->d_carry_spare, t->d_carry_snap));
    /* The turns of the worker's loop end where its queue runs dry - the end of the call - and at an END_FILE tag (fillUntilBufferFull
     * leaves its loop there, :138-152).  An END_FILE that finds fewer than three pairs in the window does not purge (outputAudio :1298-1301):
     * the one or two pairs are scanned as the end of a file and stay, and the next turn fills up behind them.  Such a tag therefore splits
     * the call into spans that are worked off one after the other, each from the window the one before it left; everything else - any number
     * of files - is one span.  A failed call takes nothing: the state of the stream at its start is kept until the last span has succeeded. */
    const uint32_t n_carry0 = t->n_carry; const uint64_t next_index0 = t->next_index; const bool stalled0 = t->stalled;
    bool snapped = false;
    auto restore = [&]() {
        if (!snapped) return;
        (void)rt::d2d(t->d_carry, t->d_carry_snap, (size_t)sdva::WIN * sizeof(sdv_sample_pair), s); (void)rt::ssync(s);
        t->n_carry = n_carry0; t->next_index = next_index0; t->stalled = stalled0;
    };
    size_t from = 0, out_total = 0, purges_total = 0; uint64_t masked_total = 0;
    for (;;) {
        size_t got = 0, got_purges = 0, split = 0; uint64_t got_masked = 0;
        const bool was_stalled = t->stalled;
        /* a stalled worker no longer takes input (:108); stop() still purges the window as it is (:1655-1660, :1716-1745) */
        if (was_stalled && !stop) break;
        const size_t span_n = was_stalled ? 0 : n_pairs - from;
        const int rc = audio_process_span(e, t, (pairs && span_n) ? pairs + from : NULL, span_n, stop, out_pairs ? out_pairs + out_total : NULL, out_cap > out_total ? out_cap - out_total : 0, &got,
                                          out_purges ? out_purges + purges_total : NULL, purges_cap > purges_total ? purges_cap - purges_total : 0, &got_purges, &got_masked, s,
                                          out_total, (uint32_t)(was_stalled ? n_pairs : from), &split, was_stalled);
        out_total += got; purges_total += got_purges; masked_total += got_masked;
        if (rc != SDV_OK) { *n_out = out_total; *n_purges = purges_total; restore(); return rc; }
        if (was_stalled) break;                         /* purged */
        if (t->stalled) { if (!snapped) { RT_CHECK(rt::d2d(t->d_carry_snap, t->d_carry_spare, (size_t)sdva::WIN * sizeof(sdv_sample_pair), s)); snapped = true; } continue; }
        if (split >= span_n) break;                     /* the span took everything (and stop(), when asked for) */
        /* the END_FILE at from + split found one or two pairs in the window (now the engine's carry): scanBuffer ran over them as the end of a
         * file - the second one, where invalid, becomes a forced zero (fixBadSamples :1122-1172; DROP_IGNORE: clearInvalids :1404-1409) */
        if (!snapped) {
            /* the state at the start of the call is still in the spare buffer (the span swapped the two) */
            RT_CHECK(rt::d2d(t->d_carry_snap, t->d_carry_spare, (size_t)sdva::WIN * sizeof(sdv_sample_pair), s));
            snapped = true;
        }
        if (t->n_carry > 0) {
            sdv_sample_pair w2[2];
            RT_CHECK(rt::d2h(w2, t->d_carry, t->n_carry * sizeof(sdv_sample_pair), s));
            for (uint32_t i = 0; i < t->n_carry; i++)
                for (int ch = 0; ch < 2; ch++) {
                    if (t->mask_mode == SDV_DROP_IGNORE) w2[i].sample_flags[ch] |= SDV_SF_WORD_VALID;
                    else if (i == 1 && !(w2[i].sample_flags[ch] & SDV_SF_WORD_VALID)) { w2[i].audio_word[ch] = 0; w2[i].sample_flags[ch] |= SDV_SF_WORD_VALID | SDV_SF_WORD_MASKED; }
                }
            RT_CHECK(rt::h2d(t->d_carry, w2, t->n_carry * sizeof(sdv_sample_pair), s));
            RT_CHECK(rt::ssync(s));
        }
        from += split + 1;
        if (from >= n_pairs && !stop) break;            /* (with stop: one more span, empty, for the purge) */
    }
    *n_out = out_total; *n_purges = purges_total;
    if (n_masked) *n_masked = masked_total;
    return SDV_OK;
}

int sdv_wav_pack(sdv_engine *e, const sdv_sample_pair *pairs, size_t n, int16_t *pcm, void *stream)
{
    if (!e) return SDV_ERR_BAD_ARG;
    if (n == 0) return SDV_OK;
    if (!pairs) { set_error(e, "null sample pair buffer"); return SDV_ERR_NULL_LINES; }
    if (!pcm) { set_error(e, "null output buffer"); return SDV_ERR_NULL_BLOCK; }
    SDV_ON_DEVICE(e);
    rt::stream_t s = (rt::stream_t)stream;
    sdva::WavArgs a; a.pairs = pairs; a.n = n; a.pcm = (uint32_t *)pcm;
    RT_LAUNCH64(sdv_k_wav_pack, (n + 63) / 64, a, s);
    return SDV_OK;
}

void sdv_wav_header(uint8_t hdr[44], uint64_t n_pairs, uint16_t last_sample_rate)
{
    /* default_header (samples2wav.cpp:4-21) with the four fields updateHeader rewrites (:111-206) */
    static const uint8_t def[44] = { 'R', 'I', 'F', 'F', 0, 0, 0, 0, 'W', 'A', 'V', 'E', 'f', 'm', 't', ' ', 0x10, 0, 0, 0, 0x01, 0, 0x02, 0,
                                     0x44, 0xAC, 0, 0, 0x10, 0xB1, 0x02, 0, 0x04, 0, 0x10, 0, 'd', 'a', 't', 'a', 0, 0, 0, 0 };
    memcpy(hdr, def, 44);
    const uint32_t rate = last_sample_rate == 44056 ? 44056u : 44100u;     /* SamplesToWAV::setSampleRate (:257-289) */
    const uint32_t file_size = (uint32_t)(44u + 4u * n_pairs), fields[4] = { file_size - 8u, rate, rate * 4u, file_size - 44u };
    const int ofs[4] = { 4, 24, 28, 40 };
    for (int f = 0; f < 4; f++) for (int k = 0; k < 4; k++) hdr[ofs[f] + k] = (uint8_t)(fields[f] >> (8 * k));
}


/* ---- de-emphasis (no reference equivalent: the definition is in include/sdvpcm.h) ------------------------------------------ */
void sdv_deemphasis_coeffs(uint16_t sample_rate, double c[3])
{
    const double fs = sample_rate == 44056 ? 44056.0 : 44100.0, K = 2.0 * fs, T1 = 50e-6, T2 = 15e-6;
    c[0] = (1.0 + K * T2) / (1.0 + K * T1);
    c[1] = (1.0 - K * T2) / (1.0 + K * T1);
    c[2] = (1.0 - K * T1) / (1.0 + K * T1);
}

int sdv_set_deemphasis(sdv_engine *e, int mode)
{
    if (!e) return SDV_ERR_BAD_ARG;
    if (mode != SDV_DEEMPH_OFF && mode != SDV_DEEMPH_AUTO && mode != SDV_DEEMPH_FORCE) { set_error(e, "no such de-emphasis mode"); return SDV_ERR_BAD_ARG; }
    audio_get(e)->de_mode = mode;
    return SDV_OK;
}

int sdv_reset_deemphasis(sdv_engine *e)
{
    if (!e) return SDV_ERR_BAD_ARG;
    audio_get(e)->de_idle = true;
    return SDV_OK;
}

int sdv_audio_deemphasis(sdv_engine *e, const sdv_sample_pair *pairs, size_t n, sdv_sample_pair *out_pairs, void *stream)
{
    if (!e) return SDV_ERR_BAD_ARG;
    sdv_audio *t = audio_get(e);
    if (n == 0) { if (t->de_mode == SDV_DEEMPH_OFF) t->de_idle = true; return SDV_OK; }
    if (!pairs) { set_error(e, "null sample pair buffer"); return SDV_ERR_NULL_LINES; }
    if (!out_pairs) { set_error(e, "null output buffer"); return SDV_ERR_NULL_BLOCK; }
    if (n >= 0x7FFF0000u) { set_error(e, "too many sample pairs in one call"); return SDV_ERR_BAD_ARG; }
    if (out_pairs != pairs && (const char *)pairs < (const char *)(out_pairs + n) && (const char *)out_pairs < (const char *)(pairs + n)) {
        set_error(e, "the output overlaps the input without being the input"); return SDV_ERR_BAD_ARG;
    }
    SDV_ON_DEVICE(e);
    rt::stream_t s = (rt::stream_t)stream;
    if (t->de_mode == SDV_DEEMPH_OFF) {
        if (out_pairs != pairs) RT_CHECK(rt::d2d(out_pairs, pairs, n * sizeof(sdv_sample_pair), s));
        t->de_idle = true;
        return SDV_OK;
    }
    const size_t n_tiles = (n + sdva::DE_TILE - 1) / sdva::DE_TILE;
    RT_CHECK(t->d_de_state.reserve(1));
    RT_CHECK(t->d_de_tiles.reserve(n_tiles, n_tiles + n_tiles / 8 + 64));
    sdva::DeArgs a; memset(&a, 0, sizeof(a));
    a.in = pairs; a.out = out_pairs; a.n = n; a.tiles = t->d_de_tiles; a.state = t->d_de_state;
    sdv_deemphasis_coeffs(44056, a.c[0]); sdv_deemphasis_coeffs(44100, a.c[1]);
    a.force = t->de_mode == SDV_DEEMPH_FORCE ? 1 : 0; a.head_idle = t->de_idle ? 1 : 0;
    /* the state in front of every tile from the input alone, then the tiles: the second pass reads nothing another tile writes (a call in place) */
    RT_LAUNCH64(sdv_k_deemph_warm, n_tiles, a, s);
    RT_LAUNCH64(sdv_k_deemph, n_tiles, a, s);
    t->de_idle = false;
    return SDV_OK;
}


/* ---- resampling 44 056 Hz -> 44 100 Hz (no reference equivalent: the definition is in include/sdvpcm.h) --------------------- */
static double rs_bessel_i0(double x)
{
    const double q = x * x / 4.0;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; k++) { term *= q / ((double)k * (double)k); sum += term; if (term < 1e-18 * sum) break; }
    return sum;
}
void sdv_resample_taps(int phase, double taps[128])
{
    if (phase != SDV_RESAMPLE_PHASE_HALF && (phase < 0 || phase >= SDV_RESAMPLE_L)) { for (int k = 0; k < 128; k++) taps[k] = 0.0; return; }
    const double frac = phase == SDV_RESAMPLE_PHASE_HALF ? 0.5 : (double)phase / (double)SDV_RESAMPLE_L;
    const double beta = 12.0, pi = 3.14159265358979323846, i0_beta = rs_bessel_i0(beta);
    long double sum = 0.0L;             /* (the normalisation must not cost the rows their gain of 1 at DC) */
    for (int k = 0; k < 128; k++) {
        const double d = (double)(k - (SDV_RESAMPLE_HALF - 1)) - frac;
        double r = 1.0 - (d / SDV_RESAMPLE_HALF) * (d / SDV_RESAMPLE_HALF);
        if (r < 0.0) r = 0.0;
        const double w = rs_bessel_i0(beta * sqrt(r)) / i0_beta, x = pi * d;
        taps[k] = (d == 0.0 ? 1.0 : sin(x) / x) * w;
        sum += (long double)taps[k];
    }
    const double total = (double)sum;
    for (int k = 0; k < 128; k++) taps[k] /= total;
}

enum { RS_DELAY_BITS = SDV_RESAMPLE_DELAY_RIGHT | SDV_RESAMPLE_DELAY_LEFT };
static size_t sk_waiting(const sdv_audio *t) { return (size_t)std::min<uint32_t>(t->sk_seen, (uint32_t)sdva::SK_WAIT); }

int sdv_set_resample(sdv_engine *e, int mode)
{
    if (!e) return SDV_ERR_BAD_ARG;
    const int delay = mode & RS_DELAY_BITS;
    if (mode < 0 || (mode & ~(SDV_RESAMPLE_TO_44100 | RS_DELAY_BITS)) || delay == RS_DELAY_BITS) { set_error(e, "no such resampling mode"); return SDV_ERR_BAD_ARG; }
    sdv_audio *t = audio_get(e);
    if (delay != (t->rs_mode & RS_DELAY_BITS) && t->sk_seen > 0) {
        set_error(e, "the skew stage holds waiting pairs of the delay that is set: flush (sdv_audio_resample) or reset (sdv_reset_resample) first");
        return SDV_ERR_BAD_ARG;
    }
    t->rs_mode = mode;
    return SDV_OK;
}

int sdv_reset_resample(sdv_engine *e)
{
    if (!e) return SDV_ERR_BAD_ARG;
    sdv_audio *t = audio_get(e);
    t->rs_seen = 0; t->rs_emitted = 0; t->sk_seen = 0;
    return SDV_OK;
}

size_t sdv_audio_resample_pending(const sdv_engine *e)
{
    if (!e || !e->audio) return 0;
    return (size_t)std::min<uint64_t>(e->audio->rs_seen, (uint64_t)SDV_RESAMPLE_HALF) + sk_waiting(e->audio);
}

/* outputs the first j pairs of a segment own (sdva::rs_owned) */
static uint64_t rs_owned_host(uint64_t j) { return j == 0 ? 0 : j + (j - 1) / SDV_RESAMPLE_M; }

size_t sdv_audio_resample_room(const sdv_engine *e, size_t n_pairs)
{
    if (!e || !e->audio || e->audio->rs_mode == SDV_RESAMPLE_OFF) return n_pairs;
    /* (the skew stage puts out one pair per pair it is given, and what waited in it) */
    if (!(e->audio->rs_mode & SDV_RESAMPLE_TO_44100)) return n_pairs + sk_waiting(e->audio);
    /* what the open segment owes when it ends, and per new pair one output and one more per thousand (a segment of n new pairs owns
     * n + floor((n - 1) / 1000); n pairs that continue the open one at most ceil(n 1001 / 1000) more than it owes) */
    const sdv_audio *t = e->audio;
    return (size_t)(rs_owned_host(t->rs_seen) - t->rs_emitted) + n_pairs + n_pairs / SDV_RESAMPLE_M + 2 + sk_waiting(t);
}

/* The resampler's three launches for one call, its result left in d_rs_result (the caller reads it back, or the skew stage does on the device). */
static int rs_queue(sdv_engine *e, sdv_audio *t, const sdv_sample_pair *pairs, size_t n_pairs, int flush, sdv_sample_pair *out_pairs, size_t out_cap, rt::stream_t s)
{
    if (!t->rs_taps_ready) {
        /* the table, transposed: the 64 lanes of a wave walk neighbouring phases of one tap */
        std::vector<double> tab((size_t)sdva::RS_TAPS * sdva::RS_PITCH, 0.0);
        double row[128];
        for (int p = 0; p < SDV_RESAMPLE_L; p++) { sdv_resample_taps(p, row); for (int k = 0; k < 128; k++) tab[(size_t)k * sdva::RS_PITCH + p] = row[k]; }
        RT_CHECK(t->d_rs_taps.reserve(tab.size()));
        RT_CHECK(rt::h2d(t->d_rs_taps, tab.data(), tab.size() * sizeof(double), s));
        RT_CHECK(rt::ssync(s));
        t->rs_taps_ready = true;
    }
    const size_t n_tiles = (n_pairs + sdva::RS_TILE - 1) / sdva::RS_TILE;
    RT_CHECK(rt::reserve_all(sdva::RS_HIST, sdva::RS_HIST, t->d_rs_hist, t->d_rs_hist_spare));
    RT_CHECK(t->d_rs_result.reserve(1));
    RT_CHECK(t->d_rs_sums.reserve(n_tiles + 1, n_tiles + n_tiles / 8 + 64));
    RT_CHECK(t->d_rs_starts.reserve(n_tiles + 1, n_tiles + n_tiles / 8 + 64));
    sdva::RsArgs a; memset(&a, 0, sizeof(a));
    a.in = pairs; a.out = out_pairs; a.n = (int64_t)n_pairs; a.out_cap = out_cap; a.hist = t->d_rs_hist; a.hist_out = t->d_rs_hist_spare;
    a.taps = t->d_rs_taps; a.sums = t->d_rs_sums; a.starts = t->d_rs_starts; a.result = t->d_rs_result;
    a.seen0 = t->rs_seen; a.emitted0 = t->rs_emitted; a.n_tiles = (uint32_t)n_tiles; a.flush = flush ? 1 : 0;
    RT_LAUNCH64(sdv_k_resample_classify, n_tiles, a, s);
    RT_LAUNCH64(sdv_k_resample_scan, 1, a, s);
    RT_LAUNCH64(sdv_k_resample_emit, n_tiles ? n_tiles : 1, a, s);
    return SDV_OK;
}

/* sdv_audio_resample with a delay bit: stage A - the copy (the skew stage then reads the caller's pairs where they lie) or the resampler, into a
 * buffer of the engine - and the skew stage behind it, which takes the resampler's count from device memory.  One read-back, behind both. */
static int audio_resample_skewed(sdv_engine *e, sdv_audio *t, const sdv_sample_pair *pairs, size_t n_pairs, int flush, sdv_sample_pair *out_pairs, size_t out_cap, size_t *n_out, void *stream)
{
    if (n_pairs > 0 && !pairs) { set_error(e, "null sample pair buffer"); return SDV_ERR_NULL_LINES; }
    if (n_pairs >= 0x7FFF0000u) { set_error(e, "too many sample pairs in one call"); return SDV_ERR_BAD_ARG; }
    const bool to_44100 = (t->rs_mode & SDV_RESAMPLE_TO_44100) != 0;
    const size_t room = sdv_audio_resample_room(e, n_pairs), room_a = room - sk_waiting(t);
    const bool run_a = to_44100 && (n_pairs > 0 || (flush && t->rs_seen > 0));
    if (!run_a && n_pairs == 0 && !(flush && t->sk_seen > 0)) {
        /* nothing in and no tail to put out */
        if (flush || !to_44100) { t->rs_seen = 0; t->rs_emitted = 0; }
        if (flush) t->sk_seen = 0;
        return SDV_OK;
    }
    if (!out_pairs) { set_error(e, "null output buffer"); return SDV_ERR_NULL_BLOCK; }
    if (out_cap < room) {
        set_error(e, "output buffer too small: room for " + std::to_string((unsigned long long)room) + " sample pairs is needed (sdv_audio_resample_room)");
        return SDV_ERR_BAD_ARG;
    }
    if (pairs && (const char *)pairs < (const char *)(out_pairs + out_cap) && (const char *)out_pairs < (const char *)(pairs + n_pairs)) {
        set_error(e, "the output overlaps the input"); return SDV_ERR_BAD_ARG;
    }
    SDV_ON_DEVICE(e);
    rt::stream_t s = (rt::stream_t)stream;
    if (!t->sk_taps_ready) {
        double row[128];
        sdv_resample_taps(SDV_RESAMPLE_PHASE_HALF, row);
        RT_CHECK(t->d_sk_taps.reserve(128));
        RT_CHECK(rt::h2d(t->d_sk_taps, row, sizeof(row), s));
        RT_CHECK(rt::ssync(s));
        t->sk_taps_ready = true;
    }
    RT_CHECK(rt::reserve_all(sdva::SK_HIST, sdva::SK_HIST, t->d_sk_hist, t->d_sk_hist_spare));
    RT_CHECK(t->d_sk_result.reserve(1));
    sdva::SkArgs a; memset(&a, 0, sizeof(a));
    a.in = pairs; a.n = (int64_t)n_pairs;
    if (run_a) {
        RT_CHECK(t->d_sk_mid.reserve(room_a, room_a + room_a / 8 + 4096));
        const int rc = rs_queue(e, t, pairs, n_pairs, flush, t->d_sk_mid, room_a, s);
        if (rc != SDV_OK) return rc;
        a.in = t->d_sk_mid; a.n = (int64_t)room_a; a.a_result = t->d_rs_result;
    }
    a.out = out_pairs; a.out_cap = out_cap; a.hist = t->d_sk_hist; a.hist_out = t->d_sk_hist_spare; a.taps = t->d_sk_taps; a.result = t->d_sk_result;
    a.seen0 = t->sk_seen; a.flush = flush ? 1 : 0; a.channel = (t->rs_mode & SDV_RESAMPLE_DELAY_RIGHT) ? 1 : 0;
    const size_t n_tiles = ((size_t)a.n + sdva::SK_TILE - 1) / sdva::SK_TILE;
    RT_LAUNCH64(sdv_k_skew, n_tiles ? n_tiles : 1, a, s);
    sdva::SkResult res;
    RT_CHECK(rt::d2h(&res, t->d_sk_result, sizeof(res), s));
    if (res.n_out > out_cap || (run_a && res.a.n_out > room_a)) { set_error(e, "internal: the resampler counted more outputs than sdv_audio_resample_room allows"); return SDV_ERR_HIP; }
    if (run_a) { t->d_rs_hist.swap(t->d_rs_hist_spare); t->rs_seen = res.a.seen; t->rs_emitted = res.a.emitted; }
    else if (flush || !to_44100) { t->rs_seen = 0; t->rs_emitted = 0; }
    t->d_sk_hist.swap(t->d_sk_hist_spare);
    t->sk_seen = res.seen;
    *n_out = (size_t)res.n_out;
    return SDV_OK;
}

int sdv_audio_resample(sdv_engine *e, const sdv_sample_pair *pairs, size_t n_pairs, int flush, sdv_sample_pair *out_pairs, size_t out_cap, size_t *n_out, void *stream)
{
    if (!e || !n_out) return SDV_ERR_BAD_ARG;
    *n_out = 0;
    sdv_audio *t = audio_get(e);
    if (t->rs_mode & RS_DELAY_BITS) return audio_resample_skewed(e, t, pairs, n_pairs, flush, out_pairs, out_cap, n_out, stream);
    if (n_pairs > 0 && !pairs) { set_error(e, "null sample pair buffer"); return SDV_ERR_NULL_LINES; }
    if (n_pairs >= 0x7FFF0000u) { set_error(e, "too many sample pairs in one call"); return SDV_ERR_BAD_ARG; }
    const size_t room = sdv_audio_resample_room(e, n_pairs);
    const bool off = t->rs_mode == SDV_RESAMPLE_OFF, tail_only = n_pairs == 0 && flush && t->rs_seen > 0;
    if (!off && n_pairs == 0 && !tail_only) { if (flush) { t->rs_seen = 0; t->rs_emitted = 0; } return SDV_OK; }
    if (off && n_pairs == 0) { t->rs_seen = 0; t->rs_emitted = 0; return SDV_OK; }
    if (!out_pairs) { set_error(e, "null output buffer"); return SDV_ERR_NULL_BLOCK; }
    if (out_cap < room) {
        set_error(e, "output buffer too small: room for " + std::to_string((unsigned long long)room) + " sample pairs is needed (sdv_audio_resample_room)");
        return SDV_ERR_BAD_ARG;
    }
    if (pairs && (const char *)pairs < (const char *)(out_pairs + out_cap) && (const char *)out_pairs < (const char *)(pairs + n_pairs)) {
        set_error(e, "the output overlaps the input"); return SDV_ERR_BAD_ARG;
    }
    SDV_ON_DEVICE(e);
    rt::stream_t s = (rt::stream_t)stream;
    if (off) {
        RT_CHECK(rt::d2d(out_pairs, pairs, n_pairs * sizeof(sdv_sample_pair), s));
        RT_CHECK(rt::ssync(s));
        t->rs_seen = 0; t->rs_emitted = 0;
        *n_out = n_pairs;
        return SDV_OK;
    }
    const int rc = rs_queue(e, t, pairs, n_pairs, flush, out_pairs, out_cap, s);
    if (rc != SDV_OK) return rc;
    sdva::RsResult res;
    RT_CHECK(rt::d2h(&res, t->d_rs_result, sizeof(res), s));
    if (res.n_out > out_cap) { set_error(e, "internal: the resampler counted more outputs than sdv_audio_resample_room allows"); return SDV_ERR_HIP; }
    t->d_rs_hist.swap(t->d_rs_hist_spare);
    t->rs_seen = res.seen; t->rs_emitted = res.emitted;
    *n_out = (size_t)res.n_out;
    return SDV_OK;
}


/* The chains of the three formats, stage after stage (see include/sdvpcm.h).  Intermediate records live in buffers of the engine. */
int sdv_decode_frames(sdv_engine *e, int pcm_type, const uint8_t *luma, size_t row_stride, size_t frame_stride, int width, int height,
                      int n_frames, uint32_t first_frame_no, unsigned flags,
                      sdv_sample_pair *out_pairs, size_t pairs_cap, size_t *n_pairs, void *out_frames, size_t frames_cap, size_t *n_frames_out,
                      sdv_frame_stats *out_stats, size_t stats_cap,
                      int with_audio, int audio_stop, sdv_audio_purge *out_purges, size_t purges_cap, size_t *n_purges, uint64_t *n_masked, void *stream)
{
    if (!e || !n_pairs || !n_frames_out) { if (e) e->frame_flags_pending = false; return SDV_ERR_BAD_ARG; }
    FrameFlagsConsumed flags_consumed_at_exit(e);       /* (the frame entry called below takes them; a refusal before that must not leave them for a later call) */
    *n_pairs = 0; *n_frames_out = 0;
    if (n_purges) *n_purges = 0;
    if (n_masked) *n_masked = 0;
    if (pcm_type != SDV_PCM_STC007 && pcm_type != SDV_PCM_PCM1 && pcm_type != SDV_PCM_PCM16X0) { set_error(e, "unknown PCM type"); return SDV_ERR_BAD_ARG; }
    if (with_audio && (!n_purges || !n_masked)) { set_error(e, "with_audio needs n_purges and n_masked"); return SDV_ERR_BAD_ARG; }
    if (n_frames < 0 || height <= 0) { set_error(e, "bad frame geometry"); return SDV_ERR_BAD_ARG; }
    rt::stream_t s = (rt::stream_t)stream;
    SDV_ON_DEVICE(e);
    sdv_audio *t = audio_get(e);
    /* line records: the largest of the three layouts is 48 bytes; PCM-16x0 has three records per video line */
    const size_t n_recs = pcm_type == SDV_PCM_PCM16X0 ? sdv_pcm16x0_binarize_records(height, n_frames, flags) : sdv_binarize_records(height, n_frames, flags);
    const size_t rec_bytes = pcm_type == SDV_PCM_STC007 ? sizeof(sdv_line_rec) : pcm_type == SDV_PCM_PCM1 ? sizeof(sdv_pcm1_bin_rec) + sizeof(sdv_pcm1_line_rec) : sizeof(sdv_pcm16x0_bin_rec);
    const size_t stats_n = (size_t)n_frames + ((flags & SDV_FLAG_END_FILE) ? 1 : 0);
    RT_CHECK(t->d_chain_recs.reserve(n_recs * rec_bytes, n_recs * rec_bytes + n_recs * rec_bytes / 8 + 4096));
    if (!out_stats) RT_CHECK(t->d_chain_stats.reserve(stats_n, stats_n + stats_n / 8 + 16));
    sdv_frame_stats *stats = out_stats ? out_stats : t->d_chain_stats.p;
    const size_t stats_room = out_stats ? stats_cap : t->d_chain_stats.cap;
    /* with the audio stage behind it the stitcher writes into a buffer of the engine (the caller's buffer takes the masked stream) */
    sdv_sample_pair *raw = out_pairs; size_t raw_cap = pairs_cap;
    if (with_audio) {
        const size_t want = (size_t)(n_frames + 2) * 1800 + 8192;          /* 1470 pairs per NTSC frame, 1764 per PAL frame, + what waited */
        RT_CHECK(t->d_chain_pairs.reserve(want, want + want / 8));
        raw = t->d_chain_pairs; raw_cap = t->d_chain_pairs.cap;
    }
    int rc;
    size_t got_pairs = 0, got_frames = 0;
    if (pcm_type == SDV_PCM_STC007) {
        sdv_line_rec *recs = (sdv_line_rec *)t->d_chain_recs.p;
        /* frames in the middle of a source: the records are n_frames runs of height + 3, the stitch stage need not look for the frame ends */
        StitchRegular reg; reg.recs_per_frame = (size_t)height + 3; reg.n_frames = (size_t)n_frames;
        const bool plain_frames = !(flags & (SDV_FLAG_NEW_FILE | SDV_FLAG_END_FILE)) && n_frames > 0 && n_recs == reg.recs_per_frame * reg.n_frames;
        /* ... and on a stream that plays the frame kernel puts the frames it captures whole straight into the stitcher's field buffers (32-byte lines in
         * field order, no 48-byte records written or read for them): armed when the stitch call behind will take its pipelined path, which reads no
         * record of those frames.  Should that path not be taken after all, nothing of either stream state has moved: the frames are decoded again, with
         * records. */
        const sdv_v2d_state chain_before = e->chain; const bool worn_before = e->worn_tape;
        const bool flags_pending = e->frame_flags_pending;
        FusedHooks hooks;           /* for the first of the frame calls below */
        memset(&hooks, 0, sizeof(hooks));
        if (plain_frames && !flags_pending) {
            rc = stitch_prepare_direct(e, (size_t)n_frames, reg.recs_per_frame, raw_cap, frames_cap, &hooks.direct_fields, &hooks.direct_frames, &hooks.direct_seg_ofs);
            if (rc != SDV_OK) return rc;
            hooks.direct_pitch = (int)sdvs::FIELD_PITCH; hooks.direct_lines = (int)sdvs::BUF_FIELD;
        }
        /* ... and the stitch stage's kernels are queued right behind the frame kernel's first round, ahead of the host's look at that round (a tape that plays
         * settles in it: the last call did).  Should the round not have been the last, the stitch call is made over. */
        struct Ahead { sdv_engine *e; const sdv_line_rec *recs; size_t n_recs; sdv_sample_pair *raw; size_t raw_cap; sdv_frame_asm *frames; size_t frames_cap; void *stream;
                       const StitchRegular *reg; int rc; } ahead = { e, recs, n_recs, raw, raw_cap, (sdv_frame_asm *)out_frames, frames_cap, stream, &reg, SDV_STITCH_NOT_QUEUED };
        const bool may_queue_ahead = hooks.direct_fields != NULL && e->binarize_settled_at_once && !e->profiling && !dev_env("SDV_NO_QUEUE_AHEAD");
        if (may_queue_ahead) {
            hooks.after_ctx = &ahead;
            hooks.after_first_round = [](void *ctx) -> int {
                Ahead *h = (Ahead *)ctx; size_t np = 0, nf = 0;
                h->rc = stitch_frames_impl(h->e, h->recs, h->n_recs, h->raw, h->raw_cap, &np, h->frames, h->frames_cap, &nf, h->stream, h->reg, STITCH_QUEUE_AHEAD);
                return (h->rc == SDV_STITCH_QUEUED_AHEAD || h->rc == SDV_STITCH_NOT_QUEUED || h->rc == SDV_STITCH_RETRY_WITH_RECORDS) ? SDV_OK : h->rc;
            };
        }
        rc = stc007_binarize_frames_impl(e, luma, row_stride, frame_stride, width, height, n_frames, first_frame_no, flags, recs, n_recs, stats, stats_room, stream, &hooks);
        /* (an error behind the point where the stitch stage's work was queued ahead: that work writes the caller's buffers - nothing of it is left in flight
         * when the call returns) */
        if (rc != SDV_OK) { if (e->stitch) e->stitch->direct_armed = false; if (may_queue_ahead) (void)rt::ssync(s); return rc; }
        e->binarize_settled_at_once = e->info.rounds == 1;
        if (ahead.rc == SDV_STITCH_QUEUED_AHEAD && e->info.rounds == 1)
            rc = stitch_frames_impl(e, recs, n_recs, raw, raw_cap, &got_pairs, (sdv_frame_asm *)out_frames, frames_cap, &got_frames, stream, &reg, STITCH_TAKE_UP);
        else if (ahead.rc == SDV_STITCH_RETRY_WITH_RECORDS) rc = SDV_STITCH_RETRY_WITH_RECORDS;
        else {
            if (ahead.rc == SDV_STITCH_QUEUED_AHEAD) e->stitch->direct_armed = e->stitch->ahead_direct;      /* (what was queued ran on frames that were decoded again since) */
            rc = stitch_frames_impl(e, recs, n_recs, raw, raw_cap, &got_pairs, (sdv_frame_asm *)out_frames, frames_cap, &got_frames, stream, plain_frames ? &reg : NULL);
            if (ahead.rc == SDV_STITCH_QUEUED_AHEAD && rc == SDV_OK) e->stitch->info.pipelined |= 8u;
        }
        if (rc == SDV_STITCH_RETRY_WITH_RECORDS) {
            e->chain = chain_before; e->worn_tape = worn_before;
            if (e->stitch) e->stitch->direct_armed = false;
            rc = sdv_binarize_frames(e, luma, row_stride, frame_stride, width, height, n_frames, first_frame_no, flags, recs, n_recs, stats, stats_room, stream);
            if (rc != SDV_OK) { if (may_queue_ahead) (void)rt::ssync(s); return rc; }
            rc = stitch_frames_impl(e, recs, n_recs, raw, raw_cap, &got_pairs, (sdv_frame_asm *)out_frames, frames_cap, &got_frames, stream, plain_frames ? &reg : NULL);
        }
        if (rc != SDV_OK && may_queue_ahead) (void)rt::ssync(s);
    } else if (pcm_type == SDV_PCM_PCM1) {
        const size_t lines_ofs = (n_recs * sizeof(sdv_pcm1_bin_rec) + 255) & ~(size_t)255;
        RT_CHECK(t->d_chain_recs.reserve(lines_ofs + n_recs * sizeof(sdv_pcm1_line_rec), lines_ofs + n_recs * sizeof(sdv_pcm1_line_rec) + 4096));
        sdv_pcm1_bin_rec *recs = (sdv_pcm1_bin_rec *)t->d_chain_recs.p;
        sdv_pcm1_line_rec *lines = (sdv_pcm1_line_rec *)(t->d_chain_recs + lines_ofs);
        rc = sdv_pcm1_binarize_frames(e, luma, row_stride, frame_stride, width, height, n_frames, first_frame_no, flags, recs, n_recs, stats, stats_room, stream);
        if (rc != SDV_OK) return rc;
        rc = sdv_pcm1_bin_to_line_recs(e, recs, n_recs, lines, stream);
        if (rc != SDV_OK) return rc;
        rc = sdv_pcm1_stitch_frames(e, lines, n_recs, raw, raw_cap, &got_pairs, (sdv_frame_asm_pcm1 *)out_frames, frames_cap, &got_frames, stream);
    } else {
        sdv_pcm16x0_bin_rec *recs = (sdv_pcm16x0_bin_rec *)t->d_chain_recs.p;
        rc = sdv_pcm16x0_binarize_frames(e, luma, row_stride, frame_stride, width, height, n_frames, first_frame_no, flags, recs, n_recs, stats, stats_room, stream);
        if (rc != SDV_OK) return rc;
        rc = sdv_pcm16x0_stitch_frames(e, recs, n_recs, raw, raw_cap, &got_pairs, (sdv_frame_asm_pcm16x0 *)out_frames, frames_cap, &got_frames, stream);
    }
    *n_frames_out = got_frames;
    if (rc != SDV_OK) { *n_pairs = got_pairs; return rc; }
    if (!with_audio) { *n_pairs = got_pairs; return SDV_OK; }
    rc = sdv_audio_process(e, raw, got_pairs, audio_stop, out_pairs, pairs_cap, n_pairs, out_purges, purges_cap, n_purges, n_masked, stream);
    if (rc != SDV_OK || t->de_mode == SDV_DEEMPH_OFF) return rc;
    return sdv_audio_deemphasis(e, out_pairs, *n_pairs, out_pairs, stream);         /* behind the AudioProcessor, where the pairs lie */
}

} // extern "C"

