/*
 * pcm16_engine.inc - host side of the PCM-16x0 back half (sdv_pcm16x0_stitch_frames, include/sdvpcm.h); included after
 * pcm16_frames_engine.inc by the same two translation units (product: HIP; tests: SIMT emulator).
 * A call: frame segments (two launches and one small read-back, as for PCM-1), then per batch of frames the kernels of
 * pcm16_stitch_device.h in a row - analyse (all frames at once), choose (frames in order) + finish, carry (in order: what waits in
 * conv_queue, output offsets), ctrl (all at once), flags (in order), emit (all at once).  The stitcher's stream state (padding and Control Bit histories) stays in device memory between the
 * kernels and between calls; a call that fails puts back the copy taken at its start.
 */
#include "stitch_stream.inc"
/* The analysis of a batch does not depend on the decisions of the batch before it: where streams run beside each other (rt::CONCURRENT, the product
 * build) it runs on a stream of its own, ahead of the in-order kernels (which are single waves and leave the chip idle); the emulator build runs
 * everything in order on the caller's stream. */
struct sdv_pcm16_stitcher {
    sdv_pcm16x0_stitch_settings st;
    /* (made by new sdv_pcm16_stitcher(): everything that is not a buffer starts as zero) */
    RecStream<sdv_pcm16x0_bin_rec> rs;          /* the records of the stream and their segments (stitch_stream.inc) */
    rt::DevBuf<uint32_t> d_vblk_ofs, d_vline_ofs, d_field_src;
    VisFeed<sdv_pcm16x0_block_rec> vis_blocks;  /* the visualiser's feed ... */
    VisFeed<sdv_pcm16x0_bin_rec> vis_lines;     /* ... and its assembled sub-lines */
    rt::DevBuf<sdvp16::State16> d_state;               /* [0] the stream's state, [1] its copy at the start of the running call */
    bool state_valid;
    rt::DevBuf<sdvp16::Sub> d_rem, d_rem_slots;       /* conv_queue's remainder: behind the last call (FRAME_SUBS entries) / behind every batch of the running call */
    rt::DevBuf<sdvp16::Ana16> d_ana; rt::DevBuf<sdvp16::Pick16> d_pick; rt::DevBuf<sdvp16::Choice16> d_choice; rt::DevBuf<sdvp16::Dec16> d_dec; rt::DevBuf<sdvp16::Ctrl16> d_ctrl; rt::DevBuf<sdvp16::Sub> d_fields;
    /* a second stream for the analysis kernels, which run ahead of the in-order decisions, and two for the chains behind them.  The last member: it goes
     * first, and its going waits for the side streams - the buffers above go after that */
    rt::SideStreams side;
};
#ifndef SDV_P16_ANA_BATCHES
#define SDV_P16_ANA_BATCHES 3
#endif
#ifndef SDV_P16_STITCH_BATCH
#define SDV_P16_STITCH_BATCH 1024           /* frames per batch (the unit of the hand-over between the analysis and the in-order kernels); 23.5 KB of field buffers per frame */
#endif

extern "C" void sdv_default_pcm16x0_stitch_settings(sdv_pcm16x0_stitch_settings *st);
static sdv_pcm16_stitcher *pcm16_get(sdv_engine *e)
{
    if (e->pcm16) return e->pcm16;
    sdv_pcm16_stitcher *t = new sdv_pcm16_stitcher();
    sdv_default_pcm16x0_stitch_settings(&t->st);
    e->pcm16 = t;
    return t;
}
static void pcm16_free(sdv_engine *e)
{
    sdv_pcm16_stitcher *t = e->pcm16;
    if (!t) return;
    delete t;       /* (rt::SideStreams waits for the side streams ahead of the buffers) */
    e->pcm16 = NULL;
}

extern "C" {

void sdv_default_pcm16x0_stitch_settings(sdv_pcm16x0_stitch_settings *st)     /* PCM16X0DataStitcher ctor + setDefaultFineSettings, pcm16x0datastitcher.cpp:3-33, 5636-5641 */
{
    memset(st, 0, sizeof(*st));
    st->format = SDV_P16_FORMAT_SI; st->field_order = sdvp16::ORDER_TFF; st->p_correction = 1; st->use_ecc = 1; st->mask_seams = 1;
    st->broke_mask = sdvp16::MAX_PAD_EI; st->sample_rate_preset = 1;
}

int sdv_set_pcm16x0_stitch_settings(sdv_engine *e, const sdv_pcm16x0_stitch_settings *st)
{
    if (!e || !st) return SDV_ERR_BAD_ARG;
    if (st->format > SDV_P16_FORMAT_EI) { set_error(e, "unknown PCM-16x0 format"); return SDV_ERR_BAD_ARG; }
    sdv_pcm16_stitcher *t = pcm16_get(e);
    t->st = *st;
    t->rs.n_carry = 0; t->state_valid = false;         /* a fresh stitcher */
    return SDV_OK;
}

/* ---- the stream state as a blob: checkpoints, and the hand-over between the GPUs of a sharded tape (sharded.py) ----------------------
 * What PCM16X0DataStitcher carries from frame to frame are its four statistics rings (paddings, emphasis / code / sample rate of the
 * Control Bits) and the Control Bit values of the last frame; the rings are exported oldest entry first, so that two engines that hold
 * the same history compare equal whatever slot their next push goes to; after a frame of the wrong size (pcm16x0datastitcher.cpp:4699-4703)
 * also the sub-lines that wait in conv_queue for the next frame.  Sub-line records of an unfinished frame are not part of it. */
struct sdv_pcm16_state_blob { uint32_t magic; uint32_t _pad; sdvp16::State16 st; sdvp16::Sub rem[sdvp16::FRAME_SUBS]; };       /* rem: st.rem_n sub-lines still in conv_queue, the rest zero */
static void p16_state_fresh(sdvp16::State16 *st0)          /* resetState (:64-85) */
{
    memset(st0, 0, sizeof(*st0));
    memset(st0->pad_ring, sdvp16::INVALID_PAD, sizeof(st0->pad_ring));
    st0->f1_srate = 44056;
}
static void p16_state_rotate(const sdvp16::State16 &in, sdvp16::State16 *out)
{
    *out = in;
    const int D = sdvp16::STATS_DEPTH;
    const int pp = ((in.pad_pos % D) + D) % D, cp = ((in.ctrl_pos % D) + D) % D;
    for (int i = 0; i < D; i++) {
        out->pad_ring[i] = in.pad_ring[(pp + i) % D];
        out->emph_ring[i] = in.emph_ring[(cp + i) % D]; out->code_ring[i] = in.code_ring[(cp + i) % D]; out->srate_ring[i] = in.srate_ring[(cp + i) % D];
    }
    out->pad_pos = 0; out->ctrl_pos = 0;
}
size_t sdv_pcm16x0_stitch_state_size(void) { return sizeof(sdv_pcm16_state_blob); }
int sdv_get_pcm16x0_stitch_state(sdv_engine *e, void *out, size_t cap)
{
    if (!e || !out || cap < sizeof(sdv_pcm16_state_blob)) return SDV_ERR_BAD_ARG;
    SDV_ON_DEVICE(e);
    sdv_pcm16_stitcher *t = pcm16_get(e);
    sdvp16::State16 cur;
    if (t->d_state && t->state_valid) { RT_CHECK(rt::d2h(&cur, t->d_state, sizeof(cur), (rt::stream_t)0)); }
    else p16_state_fresh(&cur);
    sdv_pcm16_state_blob *b = (sdv_pcm16_state_blob *)out;
    memset(b, 0, sizeof(*b));
    b->magic = 0x36315653u;
    p16_state_rotate(cur, &b->st);
    if (cur.rem_n > 0 && cur.rem_n < (uint32_t)sdvp16::FRAME_SUBS && t->d_rem) RT_CHECK(rt::d2h(b->rem, t->d_rem, cur.rem_n * sizeof(sdvp16::Sub), (rt::stream_t)0));
    return SDV_OK;
}
int sdv_set_pcm16x0_stitch_state(sdv_engine *e, const void *in, size_t n)
{
    if (!e || !in || n < sizeof(sdv_pcm16_state_blob)) return SDV_ERR_BAD_ARG;
    const sdv_pcm16_state_blob *b = (const sdv_pcm16_state_blob *)in;
    if (b->magic != 0x36315653u) { set_error(e, "not a PCM-16x0 stitch state"); return SDV_ERR_BAD_ARG; }
    SDV_ON_DEVICE(e);
    sdv_pcm16_stitcher *t = pcm16_get(e);
    if (b->st.rem_n >= (uint32_t)sdvp16::FRAME_SUBS) { set_error(e, "not a PCM-16x0 stitch state"); return SDV_ERR_BAD_ARG; }
    RT_CHECK(t->d_state.reserve(2));
    RT_CHECK(t->d_rem.reserve(sdvp16::FRAME_SUBS));
    RT_CHECK(rt::h2d(t->d_state, &b->st, sizeof(b->st), (rt::stream_t)0));
    RT_CHECK(rt::h2d(t->d_rem, b->rem, sizeof(b->rem), (rt::stream_t)0));
    RT_CHECK(rt::ssync((rt::stream_t)0));
    t->state_valid = true; t->rs.n_carry = 0;
    return SDV_OK;
}
/* every ring filled with its most frequent entry: for an engine that joined the stream after a short warm-up and is about to compare
 * its state with the true one (on a tape that plays, the true rings hold one value each) */
int sdv_saturate_pcm16x0_stitch_stats(sdv_engine *e)
{
    if (!e) return SDV_ERR_BAD_ARG;
    sdv_pcm16_state_blob b;
    int rc = sdv_get_pcm16x0_stitch_state(e, &b, sizeof(b));
    if (rc != SDV_OK) return rc;
    const int D = sdvp16::STATS_DEPTH;
    auto majority8 = [&](uint8_t *r, int skip) { int best = -1, bc = 0; for (int i = 0; i < D; i++) { if ((int)r[i] == skip) continue; int c = 0; for (int j = 0; j < D; j++) c += r[j] == r[i]; if (c > bc) { bc = c; best = r[i]; } } if (best >= 0) for (int i = 0; i < D; i++) r[i] = (uint8_t)best; };
    majority8(b.st.pad_ring, sdvp16::INVALID_PAD); majority8(b.st.emph_ring, -1); majority8(b.st.code_ring, -1);
    { int best = -1, bc = 0; for (int i = 0; i < D; i++) { int c = 0; for (int j = 0; j < D; j++) c += b.st.srate_ring[j] == b.st.srate_ring[i]; if (c > bc) { bc = c; best = b.st.srate_ring[i]; } } for (int i = 0; i < D; i++) b.st.srate_ring[i] = (uint16_t)best; }
    return sdv_set_pcm16x0_stitch_state(e, &b, sizeof(b));
}

int sdv_set_pcm16x0_stitch_block_output(sdv_engine *e, sdv_pcm16x0_block_rec *out_blocks, size_t blocks_cap) { if (!e) return SDV_ERR_BAD_ARG; pcm16_get(e)->vis_blocks.set(out_blocks, blocks_cap); return SDV_OK; }
size_t sdv_pcm16x0_stitch_block_count(sdv_engine *e) { return e && e->pcm16 ? e->pcm16->vis_blocks.n : 0; }
int sdv_set_pcm16x0_stitch_line_output(sdv_engine *e, sdv_pcm16x0_bin_rec *out_lines, size_t lines_cap) { if (!e) return SDV_ERR_BAD_ARG; pcm16_get(e)->vis_lines.set(out_lines, lines_cap); return SDV_OK; }
size_t sdv_pcm16x0_stitch_line_count(sdv_engine *e) { return e && e->pcm16 ? e->pcm16->vis_lines.n : 0; }

int sdv_pcm16x0_stitch_frames(sdv_engine *e, const sdv_pcm16x0_bin_rec *lines, size_t n_lines, sdv_sample_pair *out_pairs, size_t pairs_cap, size_t *n_pairs,
                              sdv_frame_asm_pcm16x0 *out_frames, size_t frames_cap, size_t *n_frames, void *stream)
{
    if (!e) return SDV_ERR_BAD_ARG;
    rt::stream_t s = (rt::stream_t)stream;
    sdv_pcm16_stitcher *t = pcm16_get(e);
    RecStream<sdv_pcm16x0_bin_rec> &rs = t->rs;
    size_t total = 0;
    { const int rc = rs.check_call(e, lines, n_lines, out_pairs, out_frames, n_pairs, n_frames, "sub-line", &total); if (rc != SDV_OK || total == 0) return rc; }
    SDV_ON_DEVICE(e);
    const sdvp16::RecSrc16 src = rs.src(lines);

    if (!t->d_state) { RT_CHECK(t->d_state.reserve(2)); t->state_valid = false; }
    RT_CHECK(t->d_rem.reserve(sdvp16::FRAME_SUBS));
    if (!t->state_valid) {      /* resetState (:64-85) */
        sdvp16::State16 st0;
        p16_state_fresh(&st0);
        RT_CHECK(rt::h2d(t->d_state, &st0, sizeof(st0), s));
        RT_CHECK(rt::ssync(s));
        t->state_valid = true;
    }
    /* 1. frame segments: positions of the END_FRAME records */
    size_t n_seg = 0;
    { const int rc = rs.segment<sdvp16::SegArgs16>(e, sdv_k_pcm16_segments, sdvp16::SEG_CHUNK16, lines, total, s, &n_seg, t->d_vblk_ofs, t->d_vline_ofs); if (rc != SDV_OK) return rc; }
    /* EI: the analysis makes every frame's padding table for the padding the history held when the call began, and for all 81 only where that one does
     * not pass (pcm16_stitch_device.h, analyse_body).  The in-order pass says so when a frame treated that way needed more - then everything from
     * here on runs once more, with full tables. */
    uint32_t stat[4] = { 0, 0, 0, 0 }; uint64_t tot_pairs = 0; uint32_t tot_frames = 0, last_end = 0;
    for (int attempt = 0;; attempt++) {
    const bool hint_on = attempt == 0 && n_seg > 0 && t->st.format == SDV_P16_FORMAT_EI && !dev_env("SDV_P16_NO_HINT");
    if (n_seg > 0) {
        if (attempt > 0) { const uint32_t again[4] = { 0, 0xFFFFFFFFu, stat[2], 0 }; RT_CHECK(rt::h2d(rs.d_stat, again, sizeof(again), s)); RT_CHECK(rt::ssync(s)); }

        /* 2. output offsets: a running sum the carry kernel of every batch takes on (a frame's count depends on what waits in conv_queue) */
        RT_CHECK(rt::dfill_bytes(rs.d_pair_ofs, 0, sizeof(uint64_t), s));
        RT_CHECK(rt::dfill_bytes(rs.d_frasm_ofs, 0, sizeof(uint32_t), s));
        RT_CHECK(rt::dfill_bytes(t->d_vblk_ofs, 0, sizeof(uint32_t), s));
        RT_CHECK(rt::dfill_bytes(t->d_vline_ofs, 0, sizeof(uint32_t), s));

        /* 3. the frames, a batch at a time; the buffers hold every batch of the call so that the analysis can run ahead */
        const size_t batch = n_seg < (size_t)SDV_P16_STITCH_BATCH ? n_seg : (size_t)SDV_P16_STITCH_BATCH;
        const size_t n_batches = (n_seg + batch - 1) / batch;
        const size_t c = n_seg + n_seg / 8 + 16, per_frame = 2 * sdvp16::SUBLINES_PF;
        RT_CHECK(rt::reserve_all(n_seg, c, t->d_ana, t->d_pick, t->d_choice, t->d_dec, t->d_ctrl));
        RT_CHECK(t->d_fields.reserve(n_seg * per_frame, c * per_frame));
        if (t->vis_lines.p) RT_CHECK(t->d_field_src.reserve(n_seg * per_frame, c * per_frame));
        RT_CHECK(t->d_rem_slots.reserve(n_batches * sdvp16::FRAME_SUBS));
        RT_CHECK(rt::d2d(t->d_state + 1, t->d_state, sizeof(sdvp16::State16), s));
        sdvp16::FrameArgs16s fa; fa.src = src; fa.seg_end = rs.d_seg_end; fa.n_seg = (uint32_t)n_seg;
        fa.cfg.format = t->st.format; fa.cfg.field_order = t->st.field_order; fa.cfg.p_correction = t->st.p_correction; fa.cfg.ignore_crc = t->st.use_ecc == 0;
        fa.cfg.mask_seams = t->st.mask_seams; fa.cfg.broke_mask = t->st.broke_mask; fa.cfg.sample_rate_preset = t->st.sample_rate_preset;
        fa.marks = rs.d_marks; fa.pair_ofs = rs.d_pair_ofs; fa.frasm_ofs = rs.d_frasm_ofs;
        fa.vblk_ofs = t->vis_blocks.p ? t->d_vblk_ofs.p : NULL; fa.out_blocks = t->vis_blocks.p; fa.blocks_cap = t->vis_blocks.cap;
        fa.vline_ofs = t->vis_lines.p ? t->d_vline_ofs.p : NULL; fa.out_lines = t->vis_lines.p; fa.lines_cap = t->vis_lines.cap; fa.field_src = NULL;
        fa.state = t->d_state; fa.state_snap = hint_on ? t->d_state.p : NULL;      /* (the analysis reads the history as it stands while it runs: a hint, checked by what it is used for) */
        fa.out_pairs = out_pairs; fa.pairs_cap = pairs_cap; fa.out_frames = out_frames; fa.frames_cap = (uint32_t)(frames_cap > 0xFFFFFFFFu ? 0xFFFFFFFFu : frames_cap);
        fa.stat = rs.d_stat;
        auto point_at = [&](size_t b0) {
            fa.seg_base = (uint32_t)b0; fa.n_batch = (uint32_t)(n_seg - b0 < batch ? n_seg - b0 : batch);
            fa.ana = t->d_ana + b0; fa.pick = t->d_pick + b0; fa.choice = t->d_choice + b0; fa.dec = t->d_dec + b0; fa.ctrl = t->d_ctrl + b0;
            fa.fields = t->d_fields + b0 * 2 * sdvp16::SUBLINES_PF;
            fa.field_src = t->vis_lines.p ? t->d_field_src + b0 * 2 * sdvp16::SUBLINES_PF : NULL;
            const size_t b = b0 / batch;
            fa.rem_in = b == 0 ? t->d_rem : t->d_rem_slots + (b - 1) * sdvp16::FRAME_SUBS; fa.rem_out = t->d_rem_slots + b * sdvp16::FRAME_SUBS;
        };
        /* The analysis is bound by what the chip holds at once (its LDS staging allows ~1 500 waves, a wave takes ~1.6 ms): it is launched
         * SDV_P16_ANA_BATCHES batches at a time - two fills of the chip - while the in-order kernels follow batch by batch. */
        /* (measured, 10 000 frames: SI 16.0 ms with three batches per launch, 15.2 ms with one - its in-order kernels are the longer chain and want to
         * start early; EI 19.5 ms against 25.3 ms - its analysis is the longer chain and wants full launches) */
        size_t ana_batches = t->st.format == SDV_P16_FORMAT_EI ? (size_t)SDV_P16_ANA_BATCHES : 1;
        if (const char *ab = dev_env("SDV_P16_ANA_BATCHES")) { const int v = atoi(ab); if (v >= 1 && v <= 64) ana_batches = (size_t)v; }      /* developer aid */
        /* With the padding hint (EI) the first batch is analysed alone and the rest waits for its decisions: a stream that starts cold has its
         * history after that batch, and everything behind it gets the short tables. */
        const bool lead = hint_on && n_batches > 2 && n_batches <= (size_t)rt::SIDE_EVENTS;
        const size_t n_ana = lead ? 1 + (n_batches - 1 + ana_batches - 1) / ana_batches : (n_batches + ana_batches - 1) / ana_batches;
        auto group_first = [&](size_t g) -> size_t { return lead ? (g == 0 ? 0 : 1 + (g - 1) * ana_batches) : g * ana_batches; };      /* its first batch */
        auto group_size = [&](size_t g) -> size_t { return lead && g == 0 ? 1 : ana_batches; };                                         /* batches */
        auto launch_groups = [&](size_t g_lo, size_t g_hi) -> int {
            for (size_t g = g_lo; g < g_hi; g++) {
                const size_t b0 = group_first(g) * batch, want = group_size(g) * batch;
                point_at(b0);
                fa.n_batch = (uint32_t)(n_seg - b0 < want ? n_seg - b0 : want);
                RT_LAUNCH64(sdv_k_pcm16_analyse, fa.n_batch, fa, t->side.stream);
                RT_CHECK(rt::record(t->side.done[g], t->side.stream));
            }
            return SDV_OK;
        };
        const bool ahead = rt::CONCURRENT && n_batches > 1 && n_ana <= (size_t)rt::SIDE_EVENTS && !dev_env("SDV_P16_NO_SIDE_STREAM") && t->side.open();
        const bool three_chains = ahead && n_batches <= (size_t)rt::SIDE_EVENTS;        /* (an event per batch) */
        if (ahead) {
            /* the analysis of every batch, back to back on the side stream, behind what this stream has done so far */
            RT_CHECK(rt::record(t->side.start, s));
            RT_CHECK(rt::wait(t->side.stream, t->side.start));
            { const int lrc = launch_groups(0, lead ? 1 : n_ana); if (lrc != SDV_OK) return lrc; }
        }
        for (size_t b = 0; b < n_batches; b++) {
            point_at(b * batch);
            if (!ahead) RT_LAUNCH64(sdv_k_pcm16_analyse, fa.n_batch, fa, s);
            else if (lead ? (b == 0 || (b - 1) % ana_batches == 0) : b % ana_batches == 0)
                RT_CHECK(rt::wait(s, t->side.done[lead ? (b == 0 ? 0 : 1 + (b - 1) / ana_batches) : b / ana_batches]));
            RT_LAUNCH64(sdv_k_pcm16_choose, 1, fa, s);
            /* Three chains of in-order kernels on three members of the state, each on a stream of its own: the padding decisions (this stream: the next
             * batch's need nothing but the padding history), what follows from them per frame and conv_queue's remainder (finish, carry, ctrl), the Control
             * Bit history and the output (flags, emit).  The slowest chain sets the pace of a batch, not their sum. */
            const rt::stream_t s_mid = three_chains ? t->side.mid : s, s_tail = three_chains ? t->side.tail : s;
            if (three_chains) {
                RT_CHECK(rt::record(t->side.chosen[b], s));
                RT_CHECK(rt::wait(s_mid, t->side.chosen[b]));
                if (lead && b == 0) {       /* the first batch's paddings are decided: the history stands, the analysis of all the others may start */
                    RT_CHECK(rt::wait(t->side.stream, t->side.chosen[0]));
                    { const int lrc = launch_groups(1, n_ana); if (lrc != SDV_OK) return lrc; }
                    point_at(0);
                }
            }
            RT_LAUNCH64(sdv_k_pcm16_finish, (fa.n_batch + 63) / 64, fa, s_mid);
            RT_LAUNCH64(sdv_k_pcm16_carry, 1, fa, s_mid);
            RT_LAUNCH64(sdv_k_pcm16_ctrl, fa.n_batch, fa, s_mid);
            if (three_chains) {
                RT_CHECK(rt::record(t->side.decided[b], s_mid));
                RT_CHECK(rt::wait(s_tail, t->side.decided[b]));
            }
            RT_LAUNCH64(sdv_k_pcm16_flags, 1, fa, s_tail);
            RT_LAUNCH64(sdv_k_pcm16_emit, fa.n_batch, fa, s_tail);
            if (t->vis_lines.p) RT_LAUNCH64(sdv_k_pcm16_emit_lines, fa.n_batch, fa, s_tail);
        }
        if (three_chains) {     /* back to one stream */
            RT_CHECK(rt::record(t->side.joined, t->side.tail));
            RT_CHECK(rt::wait(s, t->side.joined));
        }
    }

    /* 4. what the call made */
    RecStream<sdv_pcm16x0_bin_rec>::Tail tail;
    { const int rc = rs.read_tail(e, n_seg, s, &tail); if (rc != SDV_OK) return rc; }
    memcpy(stat, tail.stat, sizeof(stat)); tot_pairs = tail.pairs; tot_frames = tail.frames; last_end = tail.last_end;
    if (dev_env("SDV_P16_HINT_TRACE")) fprintf(stderr, "[p16 hint] attempt %d: hint %s, %zu frames, needs full tables: %u\n", attempt, hint_on ? "on" : "off", n_seg, stat[3]);
    if (hint_on && stat[3] && !stat[0]) {       /* a frame needed more than the one padding: the histories back to where the call began, and once more */
        RT_CHECK(rt::d2d(t->d_state, t->d_state + 1, sizeof(sdvp16::State16), s));
        RT_CHECK(rt::ssync(s));
        continue;
    }
    break;
    }
    *n_pairs = (size_t)tot_pairs; *n_frames = tot_frames;
    t->vis_blocks.n = 0;
    if (n_seg > 0 && t->vis_blocks.p) { uint32_t nb = 0; RT_CHECK(rt::d2h(&nb, t->d_vblk_ofs + n_seg, sizeof(nb), s)); t->vis_blocks.n = nb; }
    t->vis_lines.n = 0;
    if (n_seg > 0 && t->vis_lines.p) { uint32_t nl = 0; RT_CHECK(rt::d2h(&nl, t->d_vline_ofs + n_seg, sizeof(nl), s)); t->vis_lines.n = nl; }
    const bool too_small = tot_pairs > pairs_cap || tot_frames > frames_cap || t->vis_blocks.n > t->vis_blocks.cap || t->vis_lines.n > t->vis_lines.cap;
    if (stat[0] || too_small) {
        /* a failed call leaves the stream where it was: the histories are put back, the lines of the call are not taken */
        if (n_seg > 0) { RT_CHECK(rt::d2d(t->d_state, t->d_state + 1, sizeof(sdvp16::State16), s)); RT_CHECK(rt::ssync(s)); }
        if (stat[0]) {
            std::string why;
            if (stat[0] & sdvp16::FE_FOREIGN) why += " sub-lines of another frame ahead of an END_FRAME;";
            set_error(e, "PCM-16x0 frame " + std::to_string(stat[1]) + " of this call cannot be stitched:" + why);
            return SDV_ERR_UNSUPPORTED;
        }
        set_error(e, "output buffers too small: " + std::to_string((unsigned long long)tot_pairs) + " sample pairs and " + std::to_string(tot_frames) + " frame descriptors are needed" +
                     (t->vis_blocks.p ? ", " + std::to_string(t->vis_blocks.n) + " blocks for the visualiser" : std::string()) +
                     (t->vis_lines.p ? ", " + std::to_string(t->vis_lines.n) + " assembled sub-line records" : std::string()));
        return SDV_ERR_BAD_ARG;
    }
    if (n_seg > 0) {            /* what the last frame left in conv_queue (State16::rem_n says how much of it counts) */
        const size_t n_batches = (n_seg + (size_t)SDV_P16_STITCH_BATCH - 1) / (size_t)SDV_P16_STITCH_BATCH;
        RT_CHECK(rt::d2d(t->d_rem, t->d_rem_slots + (n_batches - 1) * sdvp16::FRAME_SUBS, sdvp16::FRAME_SUBS * sizeof(sdvp16::Sub), s));
    }
    /* records after the last END_FRAME wait for the next call, like sub-lines in the reference's input queue */
    return rs.keep_behind(e, n_seg > 0, last_end, lines, n_lines, s);
}

} // extern "C"
