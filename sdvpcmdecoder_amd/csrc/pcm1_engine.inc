/*
 * pcm1_engine.inc - host side of the PCM-1 back half (sdv_pcm1_stitch_frames, include/sdvpcm.h).
 * Included after stitch_engine.inc by the same two translation units (product: HIP; tests: SIMT emulator).
 * Frames are independent in this format, so a call is four launches in a row (segment count, segment ends + file tags,
 * output offsets, frames) with one small read-back between the first two to size the grid and one at the end for the counts.
 */
struct sdv_pcm1_stitcher {
    sdv_pcm1_stitch_settings st;
    /* (made by new sdv_pcm1_stitcher(): everything that is not a buffer starts as zero) */
    rt::DevBuf<sdv_pcm1_line_rec> d_carry; size_t n_carry;
    rt::DevBuf<sdv_pcm1_line_rec> d_carry_spare;
    rt::DevBuf<uint32_t> d_blk_count, d_blk_ofs;
    rt::DevBuf<uint8_t> d_svc;
    rt::DevBuf<uint32_t> d_seg_end, d_marks, d_frasm_ofs; rt::DevBuf<uint64_t> d_pair_ofs;
    rt::DevBuf<uint32_t> d_stat;
    rt::DevBuf<int> d_line_list;                /* PCM-1 line kernel: lines the lean kernel handed on, behind two counters */
    rt::DevBuf<uint8_t> d_prescan;              /* PCM-1 frame driver: prescan results, four per frame, a median per frame behind them (pcm1_frames_engine.inc) */
    /* manual line offsets: the field buffers outlive a frame (pcm1_stitch_device.h, FrameArgs1) */
    rt::DevBuf<uint32_t> d_cnt, d_kept; rt::DevBuf<sdvp1::Line16> d_hist; bool hist_ready;
    /* the visualiser's feeds (caller's buffers) and what the last call made of them */
    sdv_pcm1_block_rec *vis_blocks; size_t vis_blocks_cap, vis_blocks_n; sdv_pcm1_asm_line_rec *vis_lines; size_t vis_lines_cap, vis_lines_n;
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
    if (!e || !n_pairs || !n_frames) return SDV_ERR_BAD_ARG;
    *n_pairs = 0; *n_frames = 0;
    if (n_lines > 0 && !lines) { set_error(e, "null line buffer"); return SDV_ERR_NULL_LINES; }
    if (!out_pairs || !out_frames) { set_error(e, "null output buffer"); return SDV_ERR_NULL_BLOCK; }
    rt::stream_t s = (rt::stream_t)stream;
    SDV_ON_DEVICE(e);
    sdv_pcm1_stitcher *t = pcm1_get(e);
    const size_t total = t->n_carry + n_lines;
    if (total == 0) return SDV_OK;
    if (total >= 0x3FFFFFFFu) { set_error(e, "too many line records in one call"); return SDV_ERR_BAD_ARG; }
    sdvp1::RecSrc1 src; src.carry = t->d_carry; src.n_carry = (uint32_t)t->n_carry; src.recs = lines;

    /* 1. frame segments: positions of the END_FRAME records */
    const size_t nblk = (total + sdvp1::SEG_CHUNK1 - 1) / sdvp1::SEG_CHUNK1;
    RT_CHECK(rt::reserve_all(nblk, nblk, t->d_blk_count, t->d_blk_ofs));
    RT_CHECK(t->d_stat.reserve(8));
    RT_CHECK(t->d_svc.reserve(total, total + total / 4 + 4096));
    sdvp1::SegArgs1 sa; sa.src = src; sa.n_recs = (uint32_t)total; sa.svc = t->d_svc; sa.block_count = t->d_blk_count; sa.block_ofs = t->d_blk_ofs;
    sa.seg_end = NULL; sa.n_seg = 0; sa.marks = NULL; sa.stat = t->d_stat; sa.write = 0;
    RT_LAUNCH64(sdv_k_pcm1_segments, nblk, sa, s);
    std::vector<uint32_t> blk(nblk);
    RT_CHECK(rt::d2h(blk.data(), t->d_blk_count, nblk * sizeof(uint32_t), s));
    size_t n_seg = 0;
    for (size_t i = 0; i < nblk; i++) { uint32_t c = blk[i]; blk[i] = (uint32_t)n_seg; n_seg += c; }
    uint32_t last_end = 0;
    if (n_seg > 0) {
        RT_CHECK(rt::reserve_all(n_seg + 1, n_seg + 1 + n_seg / 8 + 16, t->d_seg_end, t->d_marks, t->d_frasm_ofs, t->d_pair_ofs));
        RT_CHECK(rt::h2d(t->d_blk_ofs, blk.data(), nblk * sizeof(uint32_t), s));
        const uint32_t stat0[4] = { 0, 0xFFFFFFFFu, 0, 0 };
        RT_CHECK(rt::h2d(t->d_stat, stat0, sizeof(stat0), s));
        RT_CHECK(rt::dfill_bytes(t->d_marks, 0, (n_seg + 1) * sizeof(uint32_t), s));
        sa.seg_end = t->d_seg_end; sa.n_seg = (uint32_t)n_seg; sa.marks = t->d_marks; sa.write = 1;
        RT_LAUNCH64(sdv_k_pcm1_segments, nblk, sa, s);

        /* 2. output offsets */
        sdvp1::ScanArgs1 ca; ca.marks = t->d_marks; ca.n_seg = (uint32_t)n_seg; ca.pair_ofs = t->d_pair_ofs; ca.frasm_ofs = t->d_frasm_ofs; ca.stat = t->d_stat;
        ca.src = src; ca.seg_end = t->d_seg_end;
        RT_LAUNCH64(sdv_k_pcm1_scan, 1, ca, s);

        /* 3. the frames */
        sdvp1::FrameArgs1 fa; fa.src = src; fa.seg_end = t->d_seg_end; fa.n_seg = (uint32_t)n_seg;
        fa.cfg.field_order = t->st.field_order; fa.cfg.auto_offset = t->st.auto_offset != 0; fa.cfg.ignore_crc = t->st.use_ecc == 0;
        fa.cfg.odd_offset = t->st.odd_offset; fa.cfg.even_offset = t->st.even_offset;
        fa.marks = t->d_marks; fa.pair_ofs = t->d_pair_ofs; fa.frasm_ofs = t->d_frasm_ofs;
        fa.out_pairs = out_pairs; fa.pairs_cap = pairs_cap; fa.out_frames = out_frames; fa.frames_cap = (uint32_t)(frames_cap > 0xFFFFFFFFu ? 0xFFFFFFFFu : frames_cap);
        fa.stat = t->d_stat;
        rt::DevBuf<unsigned long long> d_timing;
        if (dev_env("SDV_STITCH_TIMING")) { RT_CHECK(d_timing.reserve(n_seg * 8)); RT_CHECK(rt::dfill_bytes(d_timing, 0, n_seg * 8 * sizeof(unsigned long long), s)); }
        fa.timing = d_timing;
        fa.cnt_out = NULL; fa.kept_out = NULL; fa.cnt_in = NULL; fa.kept_in = NULL; fa.hist = NULL;
        fa.out_blocks = t->vis_blocks; fa.blocks_cap = t->vis_blocks_cap; fa.out_asm = t->vis_lines; fa.asm_cap = t->vis_lines_cap;
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

    /* 4. records after the last END_FRAME wait for the next call, like lines in the reference's input queue */
    uint32_t stat[4] = { 0, 0, 0, 0 }; uint64_t tot_pairs = 0; uint32_t tot_frames = 0;
    if (n_seg > 0) {        /* status words, totals and the last END_FRAME in one small copy (sdv_k_stitch_tail) */
        sdv_stitch_tail_args ta; ta.stat = t->d_stat; ta.pair_total = t->d_pair_ofs + n_seg; ta.frasm_total = t->d_frasm_ofs + n_seg; ta.last_end = t->d_seg_end + (n_seg - 1);
        RT_LAUNCH64(sdv_k_stitch_tail, 1, ta, s);
        uint32_t res[8];
        RT_CHECK(rt::d2h(res, t->d_stat, sizeof(res), s));
        memcpy(stat, res, sizeof(stat)); tot_pairs = (uint64_t)res[4] | ((uint64_t)res[5] << 32); tot_frames = res[6]; last_end = res[7];
    } else RT_CHECK(rt::ssync(s));
    *n_pairs = (size_t)tot_pairs; *n_frames = tot_frames;
    {   /* frames that are no file tags: 1470 pairs and one descriptor each (a tag: one of either) */
        const size_t data_frames = (size_t)((tot_pairs - tot_frames) / (uint64_t)(2 * sdvp1::SUBLINES_PF - 1));
        t->vis_blocks_n = t->vis_blocks ? data_frames * 16 : 0; t->vis_lines_n = t->vis_lines ? data_frames * (size_t)(2 * sdvp1::SUBLINES_PF) : 0;
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
    if (t->vis_blocks_n > t->vis_blocks_cap || t->vis_lines_n > t->vis_lines_cap) {
        set_error(e, "visualiser buffers too small: " + std::to_string(t->vis_blocks_n) + " blocks / " + std::to_string(t->vis_lines_n) + " sub-lines are needed (sdv_set_pcm1_stitch_block_output / _line_output)");
        return SDV_ERR_BAD_ARG;
    }
    if (n_seg > 0 && !t->st.auto_offset) {      /* the field buffers as this call leaves them */
        sdvp1::HistArgs1 ha; ha.src = src; ha.cnt = t->d_cnt; ha.kept = t->d_kept; ha.n_seg = (uint32_t)n_seg; ha.ignore_crc = t->st.use_ecc == 0; ha.hist = t->d_hist;
        RT_LAUNCH64(sdv_k_pcm1_hist, 1, ha, s);
        RT_CHECK(rt::ssync(s));         /* it reads the caller's records */
    }
    const size_t keep_from = n_seg > 0 ? (size_t)last_end + 1 : 0, n_keep = total - keep_from;
    if (n_keep > 0) {
        RT_CHECK(t->d_carry_spare.reserve(n_keep, n_keep + n_keep / 2 + 1024));
        size_t w = 0;
        if (keep_from < t->n_carry) { RT_CHECK(rt::d2d(t->d_carry_spare, t->d_carry + keep_from, (t->n_carry - keep_from) * sizeof(sdv_pcm1_line_rec), s)); w = t->n_carry - keep_from; }
        const size_t from_lines = keep_from > t->n_carry ? keep_from - t->n_carry : 0;
        if (from_lines < n_lines) RT_CHECK(rt::d2d(t->d_carry_spare + w, lines + from_lines, (n_lines - from_lines) * sizeof(sdv_pcm1_line_rec), s));
        RT_CHECK(rt::ssync(s));
        t->d_carry.swap(t->d_carry_spare);
    }
    t->n_carry = n_keep;
    return SDV_OK;
}

int sdv_set_pcm1_stitch_block_output(sdv_engine *e, sdv_pcm1_block_rec *out_blocks, size_t blocks_cap)
{
    if (!e) return SDV_ERR_BAD_ARG;
    sdv_pcm1_stitcher *t = pcm1_get(e);
    t->vis_blocks = out_blocks; t->vis_blocks_cap = out_blocks ? blocks_cap : 0; t->vis_blocks_n = 0;
    return SDV_OK;
}
size_t sdv_pcm1_stitch_block_count(sdv_engine *e) { return e && e->pcm1 ? e->pcm1->vis_blocks_n : 0; }
int sdv_set_pcm1_stitch_line_output(sdv_engine *e, sdv_pcm1_asm_line_rec *out_lines, size_t lines_cap)
{
    if (!e) return SDV_ERR_BAD_ARG;
    sdv_pcm1_stitcher *t = pcm1_get(e);
    t->vis_lines = out_lines; t->vis_lines_cap = out_lines ? lines_cap : 0; t->vis_lines_n = 0;
    return SDV_OK;
}
size_t sdv_pcm1_stitch_line_count(sdv_engine *e) { return e && e->pcm1 ? e->pcm1->vis_lines_n : 0; }

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

/* ---- PCM-1 front half: Binarizer::processLine with a PCM1Line output, n_lines lines per launch (pcm1_bin_device.h) -------- */
extern "C" int sdv_pcm1_binarize_lines(sdv_engine *e, const uint8_t *luma, size_t row_stride, int width, size_t n_lines,
                                       const sdv_bin_state *presets, uint32_t frame_number, uint16_t first_line, uint16_t line_step,
                                       unsigned flags, int coord_search, sdv_pcm1_bin_rec *out_lines, size_t lines_cap, void *stream)
{
    if (!e) return SDV_ERR_BAD_ARG;
    if (!luma) { set_error(e, "null video"); return SDV_ERR_NULL_VIDEO; }
    if (!out_lines) { set_error(e, "null output"); return SDV_ERR_NULL_PCM; }
    if (width <= 0 || width > SDV_PX_BYTES || row_stride < (size_t)width) { set_error(e, "bad line geometry"); return SDV_ERR_BAD_ARG; }
    if (width < sdvp1b::P1_BITS) { set_error(e, "line shorter than the 94 bit cells of a PCM-1 line"); return SDV_ERR_SHORT_LINE; }
    if (n_lines == 0) return SDV_OK;
    if (lines_cap < n_lines) { set_error(e, "output buffer too small: " + std::to_string(n_lines) + " line records are needed"); return SDV_ERR_BAD_ARG; }
    SDV_ON_DEVICE(e);
    sdvp1b::LineArgs1 a;
    memset(&a, 0, sizeof(a));
    a.luma = luma; a.row_stride = row_stride; a.width = width; a.n_lines = n_lines; a.states = presets;
    a.frame_number = frame_number; a.first_line = first_line; a.line_step = line_step;
    a.doubled = (flags & SDV_FLAG_DOUBLED) ? 1 : 0; a.mode = (uint8_t)e->mode; a.coord_search = coord_search ? 1 : 0;
    a.preset = e->preset; a.out = out_lines;
    rt::stream_t s = (rt::stream_t)stream;
    const size_t full_grid = n_lines < 8192 ? n_lines : 8192;       /* the full kernel walks its lines: 2 x what the chip holds at once */
    if (presets) {
        /* lines that decode from their presets go through the lean kernel; the others end up on a list the full kernel works off */
        sdv_pcm1_stitcher *t = pcm1_get(e);
        RT_CHECK(t->d_line_list.reserve(n_lines + 4, n_lines + n_lines / 4 + 1024));
        a.counters = t->d_line_list; a.list = t->d_line_list + 4;
        RT_CHECK(rt::dfill_bytes(a.counters, 0, 4 * sizeof(int), s));
        RT_LAUNCH64(sdv_k_pcm1_lines_lean, n_lines, a, s);
        if (e->mode == SDV_MODE_INSANE) RT_LAUNCH64(sdv_k_pcm1_lines_insane, full_grid, a, s); else RT_LAUNCH64(sdv_k_pcm1_lines, full_grid, a, s);
    } else {
        a.list = NULL; a.counters = NULL;
        if (e->mode == SDV_MODE_INSANE) RT_LAUNCH64(sdv_k_pcm1_lines_insane, full_grid, a, s); else RT_LAUNCH64(sdv_k_pcm1_lines, full_grid, a, s);
    }
    return SDV_OK;
}

