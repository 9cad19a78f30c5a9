/*
 * decode_frames_engine.inc - host side of sdv_decode_frames (include/sdvpcm.h): the workers of a format back to back - frames to line records, records
 * to sample pairs and frame records, and with with_audio the AudioProcessor and the de-emphasis - with the records that pass from stage to stage in
 * buffers of the engine.  Included by audio_engine.inc behind every stage it calls, which is also why struct sdv_audio, the state of them all, is defined here.  It launches
 * and reads back what those stages do; on an STC-007 stream that plays, the frame kernel writes the stitcher's field buffers directly and the stitch
 * stage's kernels are queued ahead of the host's look at the first round (below).
 */
struct DecodeChain {             /* what passes from stage to stage */
    rt::DevBuf<uint8_t> d_recs; rt::DevBuf<sdv_frame_stats> d_stats; rt::DevBuf<sdv_sample_pair> d_pairs;
};
struct sdv_audio { AudioProcessor proc; AudioDeemph deemph; AudioResample resample; DecodeChain chain; };
static sdv_audio *audio_make(sdv_engine *e) { if (!e->audio) e->audio = new sdv_audio(); return e->audio; }
static void audio_free(sdv_engine *e) { delete e->audio; e->audio = NULL; }
static AudioProcessor *audio_get(sdv_engine *e) { return &audio_make(e)->proc; }
static const AudioProcessor *audio_peek(const sdv_engine *e) { return e && e->audio ? &e->audio->proc : NULL; }
static AudioDeemph *deemph_get(sdv_engine *e) { return &audio_make(e)->deemph; }
static AudioResample *resample_get(sdv_engine *e) { return &audio_make(e)->resample; }
static const AudioResample *resample_peek(const sdv_engine *e) { return e && e->audio ? &e->audio->resample : NULL; }

extern "C" {

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
    DecodeChain *t = &audio_make(e)->chain;
    /* line records: the largest of the three layouts is 48 bytes; PCM-16x0 has three records per video line */
    const size_t n_recs = pcm_type == SDV_PCM_PCM16X0 ? sdv_pcm16x0_binarize_records(height, n_frames, flags) : sdv_binarize_records(height, n_frames, flags);
    const size_t rec_bytes = pcm_type == SDV_PCM_STC007 ? sizeof(sdv_line_rec) : pcm_type == SDV_PCM_PCM1 ? sizeof(sdv_pcm1_bin_rec) + sizeof(sdv_pcm1_line_rec) : sizeof(sdv_pcm16x0_bin_rec);
    const size_t stats_n = (size_t)n_frames + ((flags & SDV_FLAG_END_FILE) ? 1 : 0);
    RT_CHECK(t->d_recs.reserve(n_recs * rec_bytes, n_recs * rec_bytes + n_recs * rec_bytes / 8 + 4096));
    if (!out_stats) RT_CHECK(t->d_stats.reserve(stats_n, stats_n + stats_n / 8 + 16));
    sdv_frame_stats *stats = out_stats ? out_stats : t->d_stats.p;
    const size_t stats_room = out_stats ? stats_cap : t->d_stats.cap;
    /* with the audio stage behind it the stitcher writes into a buffer of the engine (the caller's buffer takes the masked stream) */
    sdv_sample_pair *raw = out_pairs; size_t raw_cap = pairs_cap;
    if (with_audio) {
        const size_t want = (size_t)(n_frames + 2) * 1800 + 8192;          /* 1470 pairs per NTSC frame, 1764 per PAL frame, + what waited */
        RT_CHECK(t->d_pairs.reserve(want, want + want / 8));
        raw = t->d_pairs; raw_cap = t->d_pairs.cap;
    }
    int rc;
    size_t got_pairs = 0, got_frames = 0;
    if (pcm_type == SDV_PCM_STC007) {
        sdv_line_rec *recs = (sdv_line_rec *)t->d_recs.p;
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
        RT_CHECK(t->d_recs.reserve(lines_ofs + n_recs * sizeof(sdv_pcm1_line_rec), lines_ofs + n_recs * sizeof(sdv_pcm1_line_rec) + 4096));
        sdv_pcm1_bin_rec *recs = (sdv_pcm1_bin_rec *)t->d_recs.p;
        sdv_pcm1_line_rec *lines = (sdv_pcm1_line_rec *)(t->d_recs + lines_ofs);
        rc = sdv_pcm1_binarize_frames(e, luma, row_stride, frame_stride, width, height, n_frames, first_frame_no, flags, recs, n_recs, stats, stats_room, stream);
        if (rc != SDV_OK) return rc;
        rc = sdv_pcm1_bin_to_line_recs(e, recs, n_recs, lines, stream);
        if (rc != SDV_OK) return rc;
        rc = sdv_pcm1_stitch_frames(e, lines, n_recs, raw, raw_cap, &got_pairs, (sdv_frame_asm_pcm1 *)out_frames, frames_cap, &got_frames, stream);
    } else {
        sdv_pcm16x0_bin_rec *recs = (sdv_pcm16x0_bin_rec *)t->d_recs.p;
        rc = sdv_pcm16x0_binarize_frames(e, luma, row_stride, frame_stride, width, height, n_frames, first_frame_no, flags, recs, n_recs, stats, stats_room, stream);
        if (rc != SDV_OK) return rc;
        rc = sdv_pcm16x0_stitch_frames(e, recs, n_recs, raw, raw_cap, &got_pairs, (sdv_frame_asm_pcm16x0 *)out_frames, frames_cap, &got_frames, stream);
    }
    *n_frames_out = got_frames;
    if (rc != SDV_OK) { *n_pairs = got_pairs; return rc; }
    if (!with_audio) { *n_pairs = got_pairs; return SDV_OK; }
    rc = sdv_audio_process(e, raw, got_pairs, audio_stop, out_pairs, pairs_cap, n_pairs, out_purges, purges_cap, n_purges, n_masked, stream);
    if (rc != SDV_OK || deemph_get(e)->mode == SDV_DEEMPH_OFF) return rc;
    return sdv_audio_deemphasis(e, out_pairs, *n_pairs, out_pairs, stream);         /* behind the AudioProcessor, where the pairs lie */
}

} // extern "C"
