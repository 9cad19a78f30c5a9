/*
 * audio_engine.inc - host side of sdv_audio_process / sdv_wav_pack / sdv_wav_header (include/sdvpcm.h): the reference's
 * AudioProcessor and the bytes of SamplesToWAV.  Included after pcm16_engine.inc by the same two translation units (product: HIP;
 * tests: SIMT emulator); at its end it includes the stages behind the AudioProcessor and the fused entry, each a file of its own, as engine.inc
 * includes the stages in front of it.
 * A call is: tag positions (one launch + a read-back of a few bytes), the stretch table (host: the tags split the burst into
 * stretches that each start from a purged window), prepare (work array + bitmaps) and the bitmap summary, the plan (one wave per
 * stretch, bitmaps only), a read-back of the per-stretch results, the sample work of the listed windows, a second read-back (mask
 * counts, the plan check), and - unless the caller's buffer was the work array - emit.  The stream state - what waits in the window,
 * the masking mode, the running sample index - is replaced only when the call succeeds.
 */
#include <algorithm>

struct AudioProcessor {
    int mask_mode = SDV_DROP_IGNORE;    /* the constructor's DROP_IGNORE (audioprocessor.cpp:15) */
    rt::DevBuf<sdv_sample_pair> d_carry, d_carry_spare, d_carry_snap; uint32_t n_carry = 0;    /* what waits in the window (at most 512 pairs each) */
    uint64_t next_index = 0;        /* PCMSample::index of the next pair that leaves */
    bool stalled = false;           /* the window is full and its first pairs can never leave: the worker takes no more input (audioprocessor.cpp:108) */
    rt::DevBuf<uint32_t> d_count; rt::DevBuf<uint64_t> d_tags;
    rt::DevBuf<sdva::Stretch> d_st; rt::DevBuf<sdva::StretchResult> d_res;
    rt::DevBuf<sdv_sample_pair> d_w;
    rt::DevBuf<uint64_t> d_bad1, d_bad3, d_v0, d_v1, d_m0, d_m1;
    rt::DevBuf<uint8_t> d_bad2;
    rt::DevBuf<sdva::WinRec> d_wins; rt::DevBuf<uint32_t> d_win_base;
};
/* struct sdv_audio (sdv_engine::audio) holds the AudioProcessor and the state of every stage behind it by value, so it is defined behind the last of them
 * (decode_frames_engine.inc).  A stage's file declares how its own part is reached: `get` makes the whole on first use, `peek`: NULL where none is made. */
static AudioProcessor *audio_get(sdv_engine *e);
static const AudioProcessor *audio_peek(const sdv_engine *e);

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
    AudioProcessor *t = audio_get(e);
    t->n_carry = 0; t->next_index = 0; t->stalled = false;
    return SDV_OK;
}

size_t sdv_audio_pending(const sdv_engine *e) { const AudioProcessor *t = audio_peek(e); return t ? t->n_carry : 0; }
int sdv_audio_stalled(const sdv_engine *e) { const AudioProcessor *t = audio_peek(e); return t && t->stalled ? 1 : 0; }
uint64_t sdv_audio_next_index(const sdv_engine *e) { const AudioProcessor *t = audio_peek(e); return t ? t->next_index : 0; }

} // extern "C"

/* One span of a call: the worker's turns over pairs[0, n_pairs) with the queue running dry behind them.  `split_at`: set to the position
 * of an END_FILE tag that finds fewer than three pairs in the window when there is one - the span then ends in front of it (see
 * sdv_audio_process) - else to n_pairs.  Purge records go out with `out_base` / `in_base` added. */
static int audio_process_span(sdv_engine *e, AudioProcessor *t, const sdv_sample_pair *pairs, size_t n_pairs, int stop, sdv_sample_pair *out_pairs, size_t out_cap,
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
        if (direct && ranges_overlap(pairs, n_pairs * sizeof(sdv_sample_pair), out_pairs, out_cap * sizeof(sdv_sample_pair)))
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
    const int rc_args = stage_check_pairs(e, pairs, n_pairs, NULL, false);
    if (rc_args != SDV_OK) return rc_args;
    rt::stream_t s = (rt::stream_t)stream;
    SDV_ON_DEVICE(e);
    AudioProcessor *t = audio_get(e);
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

} // extern "C"

#include "audio_deemph_engine.inc"       /* sdv_audio_deemphasis */
#include "audio_resample_engine.inc"     /* sdv_audio_resample with its skew stage */
#include "decode_frames_engine.inc"      /* sdv_decode_frames: behind every stage it calls */
