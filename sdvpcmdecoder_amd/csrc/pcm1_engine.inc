/*
 * pcm1_engine.inc - host side of the PCM-1 back half (sdv_pcm1_stitch_frames, include/sdvpcm.h).
 * Included after stitch_engine.inc by the same two translation units (product: HIP; tests: SIMT emulator).
 * Frames are independent in this format, so a call is four launches in a row (segment count, segment ends + file tags,
 * output offsets, frames) with one small read-back between the first two to size the grid and one at the end for the counts.
 */
#include "stitch_stream.inc"
struct sdv_pcm1_stitcher {
    sdv_pcm1_stitch_settings st;
    /* (made by new sdv_pcm1_stitcher(): everything that is not a buffer starts as zero) */
    RecStream<sdv_pcm1_line_rec> rs;            /* the records of the stream and their segments (stitch_stream.inc) */
    rt::DevBuf<int> d_line_list;                /* PCM-1 line kernel: lines the lean kernel handed on, behind two counters */
    rt::DevBuf<uint8_t> d_prescan;              /* PCM-1 frame driver: prescan results, four per frame, a median per frame behind them (pcm1_frames_engine.inc) */
    /* manual line offsets: the field buffers outlive a frame (pcm1_stitch_device.h, FrameArgs1) */
    rt::DevBuf<uint32_t> d_cnt, d_kept; rt::DevBuf<sdvp1::Line16> d_hist; bool hist_ready;
    /* the visualiser's feeds (caller's buffers) and what the last call made of them */
    VisFeed<sdv_pcm1_block_rec> vis_blocks; VisFeed<sdv_pcm1_asm_line_rec> vis_lines;
};

extern "C" void sdv_default_pcm1_stitch_settings(sdv_pcm1_stitch_settings *st);
static sdv_pcm1_stitcher *pcm1_get(sdv_engine *e)
{
    if (e->pcm1) return e->pcm1;
    sdv_pcm1_stitcher *t = new sdv_pcm1_stitcher();
    sdv_default_pcm1_stitch_settings(&t->st);
    e->pcm1 = t;
    return t;
}
static void pcm1_free(sdv_engine *e)
{
    sdv_pcm1_stitcher *t = e->pcm1;
    if (!t) return;
    delete t;
    e->pcm1 = NULL;
}

extern "C" {

void sdv_default_pcm1_stitch_settings(sdv_pcm1_stitch_settings *st)    /* PCM1DataStitcher ctor, pcm1datastitcher.cpp:18-31 */
{
    memset(st, 0, sizeof(*st));
    st->field_order = sdvp1::ORDER_TFF; st->auto_offset = 1; st->use_ecc = 1;
}

int sdv_set_pcm1_stitch_settings(sdv_engine *e, const sdv_pcm1_stitch_settings *st)
{
    if (!e || !st) return SDV_ERR_BAD_ARG;
    sdv_pcm1_stitcher *t = pcm1_get(e);
    t->st = *st;
    t->hist_ready = false;          /* a fresh stitcher, as constructing the object does: its field buffers hold nothing yet */
    return SDV_OK;
}

int sdv_pcm1_stitch_frames(sdv_engine *e, const sdv_pcm1_line_rec *lines, size_t n_lines, sdv_sample_pair *out_pairs, size_t pairs_cap, size_t *n_pairs,
                           sdv_frame_asm_pcm1 *out_frames, size_t frames_cap, size_t *n_frames, void *stream)
{
    if (!e) return SDV_ERR_BAD_ARG;
    rt::stream_t s = (rt::stream_t)stream;
    sdv_pcm1_stitcher *t = pcm1_get(e);
    RecStream<sdv_pcm1_line_rec> &rs = t->rs;
    size_t total = 0;
    { const int rc = rs.check_call(e, lines, n_lines, out_pairs, out_frames, n_pairs, n_frames, "line", &total); if (rc != SDV_OK || total == 0) return rc; }
    SDV_ON_DEVICE(e);
    const sdvp1::RecSrc1 src = rs.src(lines);

    /* 1. frame segments: positions of the END_FRAME records */
    size_t n_seg = 0;
    { const int rc = rs.segment<sdvp1::SegArgs1>(e, sdv_k_pcm1_segments, sdvp1::SEG_CHUNK1, lines, total, s, &n_seg); if (rc != SDV_OK) return rc; }
    if (n_seg > 0) {
        /* 2. output offsets */
        sdvp1::ScanArgs1 ca; ca.marks = rs.d_marks; ca.n_seg = (uint32_t)n_seg; ca.pair_ofs = rs.d_pair_ofs; ca.frasm_ofs = rs.d_frasm_ofs; ca.stat = rs.d_stat;
        ca.src = src; ca.seg_end = rs.d_seg_end;
        RT_LAUNCH64(sdv_k_pcm1_scan, 1, ca, s);

        /* 3. the frames */
        sdvp1::FrameArgs1 fa; fa.src = src; fa.seg_end = rs.d_seg_end; fa.n_seg = (uint32_t)n_seg;
        fa.cfg.field_order = t->st.field_order; fa.cfg.auto_offset = t->st.auto_offset != 0; fa.cfg.ignore_crc = t->st.use_ecc == 0;
        fa.cfg.odd_offset = t->st.odd_offset; fa.cfg.even_offset = t->st.even_offset;
        fa.marks = rs.d_marks; fa.pair_ofs = rs.d_pair_ofs; fa.frasm_ofs = rs.d_frasm_ofs;
        fa.out_pairs = out_pairs; fa.pairs_cap = pairs_cap; fa.out_frames = out_frames; fa.frames_cap = (uint32_t)(frames_cap > 0xFFFFFFFFu ? 0xFFFFFFFFu : frames_cap);
        fa.stat = rs.d_stat;
        rt::DevBuf<unsigned long long> d_timing;
        if (dev_env("SDV_STITCH_TIMING")) { RT_CHECK(d_timing.reserve(n_seg * 8)); RT_CHECK(rt::dfill_bytes(d_timing, 0, n_seg * 8 * sizeof(unsigned long long), s)); }
        fa.timing = d_timing;
        fa.cnt_out = NULL; fa.kept_out = NULL; fa.cnt_in = NULL; fa.kept_in = NULL; fa.hist = NULL;
        fa.out_blocks = t->vis_blocks.p; fa.blocks_cap = t->vis_blocks.cap; fa.out_asm = t->vis_lines.p; fa.asm_cap = t->vis_lines.cap;
        if (!t->st.auto_offset) {
            /* manual line offsets: a first pass leaves what every frame writes into the field buffers, the frames then look up what they are told to
             * read beyond that (pcm1_stitch_device.h) */
            const size_t c = n_seg + n_seg / 8 + 16;
            RT_CHECK(t->d_cnt.reserve(n_seg, c)); RT_CHECK(t->d_kept.reserve(n_seg * 2 * sdvp1::LINES_PF, c * 2 * sdvp1::LINES_PF));
            RT_CHECK(t->d_hist.reserve(2 * sdvp1::LINES_PF));
            if (!t->hist_ready) { sdv_p1_hist_clear_args ha; ha.hist = t->d_hist; RT_LAUNCH64(sdv_k_pcm1_hist_clear, 1, ha, s); t->hist_ready = true; }
            fa.cnt_out = t->d_cnt; fa.kept_out = t->d_kept;
            RT_LAUNCH64(sdv_k_pcm1_frames, n_seg, fa, s);
            fa.cnt_out = NULL; fa.kept_out = NULL; fa.cnt_in = t->d_cnt; fa.kept_in = t->d_kept; fa.hist = t->d_hist;
        }
        if (fa.out_blocks || fa.out_asm) RT_LAUNCH64(sdv_k_pcm1_frames_vis, n_seg, fa, s);
        else RT_LAUNCH64(sdv_k_pcm1_frames, n_seg, fa, s);
        if (d_timing) {     /* developer aid: mean cycles per phase of a frame */
            std::vector<unsigned long long> tm(n_seg * 8);
            RT_CHECK(rt::d2h(tm.data(), d_timing, tm.size() * sizeof(unsigned long long), s));
            double acc[8] = { 0 };
            for (size_t k = 0; k < n_seg; k++) for (int i = 1; i < 7; i++) acc[i] += (double)(tm[k * 8 + i] - tm[k * 8 + i - 1]);
            fprintf(stderr, "[pcm1 timing] cycles/frame: sweep1 %.0f marks %.0f trim %.0f sweep2 %.0f pad %.0f masks %.0f blocks+pairs %.0f\n", acc[1] / n_seg, 0.0, acc[2] / n_seg, acc[3] / n_seg, acc[4] / n_seg, acc[5] / n_seg, acc[6] / n_seg);
        }
    }

    /* 4. what the call made, then the records after the last END_FRAME, which wait for the next call */
    RecStream<sdv_pcm1_line_rec>::Tail tail;
    { const int rc = rs.read_tail(e, n_seg, s, &tail); if (rc != SDV_OK) return rc; }
    const uint32_t *stat = tail.stat; const uint64_t tot_pairs = tail.pairs; const uint32_t tot_frames = tail.frames;
    *n_pairs = (size_t)tot_pairs; *n_frames = tot_frames;
    {   /* frames that are no file tags: 1470 pairs and one descriptor each (a tag: one of either) */
        const size_t data_frames = (size_t)((tot_pairs - tot_frames) / (uint64_t)(2 * sdvp1::SUBLINES_PF - 1));
        t->vis_blocks.n = t->vis_blocks.p ? data_frames * 16 : 0; t->vis_lines.n = t->vis_lines.p ? data_frames * (size_t)(2 * sdvp1::SUBLINES_PF) : 0;
    }
    /* a failed call leaves the stream where it was (lines that waited for their END_FRAME still wait, this call's lines are not
     * taken): the caller can come again with larger buffers or without the offending frames */
    if (stat[0]) {
        std::string why;
        if (stat[0] & sdvp1::FE_FOREIGN) why += " lines of a later frame ahead of an END_FRAME;";
        if (stat[0] & sdvp1::FE_MARKS) why += " internal: the file tags the frame saw are not the ones its output was laid out for;";
        set_error(e, "PCM-1 frame " + std::to_string(stat[1]) + " of this call cannot be stitched frame by frame:" + why);
        return SDV_ERR_UNSUPPORTED;
    }
    if (tot_pairs > pairs_cap || tot_frames > frames_cap) {
        set_error(e, "output buffers too small: " + std::to_string((unsigned long long)tot_pairs) + " sample pairs and " + std::to_string(tot_frames) + " frame descriptors are needed");
        return SDV_ERR_BAD_ARG;
    }
    if (t->vis_blocks.n > t->vis_blocks.cap || t->vis_lines.n > t->vis_lines.cap) {
        set_error(e, "visualiser buffers too small: " + std::to_string(t->vis_blocks.n) + " blocks / " + std::to_string(t->vis_lines.n) + " sub-lines are needed (sdv_set_pcm1_stitch_block_output / _line_output)");
        return SDV_ERR_BAD_ARG;
    }
    if (n_seg > 0 && !t->st.auto_offset) {      /* the field buffers as this call leaves them */
        sdvp1::HistArgs1 ha; ha.src = src; ha.cnt = t->d_cnt; ha.kept = t->d_kept; ha.n_seg = (uint32_t)n_seg; ha.ignore_crc = t->st.use_ecc == 0; ha.hist = t->d_hist;
        RT_LAUNCH64(sdv_k_pcm1_hist, 1, ha, s);
        RT_CHECK(rt::ssync(s));         /* it reads the caller's records */
    }
    return rs.keep_behind(e, n_seg > 0, tail.last_end, lines, n_lines, s);
}

int sdv_set_pcm1_stitch_block_output(sdv_engine *e, sdv_pcm1_block_rec *out_blocks, size_t blocks_cap) { if (!e) return SDV_ERR_BAD_ARG; pcm1_get(e)->vis_blocks.set(out_blocks, blocks_cap); return SDV_OK; }
size_t sdv_pcm1_stitch_block_count(sdv_engine *e) { return e && e->pcm1 ? e->pcm1->vis_blocks.n : 0; }
int sdv_set_pcm1_stitch_line_output(sdv_engine *e, sdv_pcm1_asm_line_rec *out_lines, size_t lines_cap) { if (!e) return SDV_ERR_BAD_ARG; pcm1_get(e)->vis_lines.set(out_lines, lines_cap); return SDV_OK; }
size_t sdv_pcm1_stitch_line_count(sdv_engine *e) { return e && e->pcm1 ? e->pcm1->vis_lines.n : 0; }

int sdv_pcm1_bin_to_line_recs(sdv_engine *e, const sdv_pcm1_bin_rec *in, size_t n, sdv_pcm1_line_rec *out, void *stream)
{
    if (!e) return SDV_ERR_BAD_ARG;
    if (n == 0) return SDV_OK;
    if (!in) { set_error(e, "null line buffer"); return SDV_ERR_NULL_LINES; }
    if (!out) { set_error(e, "null output buffer"); return SDV_ERR_NULL_BLOCK; }
    SDV_ON_DEVICE(e);
    rt::stream_t s = (rt::stream_t)stream;
    sdvp1::ConvArgs1 a; a.in = in; a.out = out; a.n = n;
    RT_LAUNCH64(sdv_k_pcm1_bin_to_line, (n + 63) / 64, a, s);
    return SDV_OK;
}

} // extern "C"
