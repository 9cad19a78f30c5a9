/*
 * vis_engine.inc - host side of the visualiser canvases (sdv_vis_render_lines, include/sdvpcm.h; kernels in vis_device.h).
 * Included after audio_engine.inc by the same two translation units (product: HIP; tests: SIMT emulator).
 * A call is six launches: END_FRAME / row counts per 64 records, (their prefix sums on the host: the one read-back, it also tells how
 * many frames there are), the frames' first rows, the lines, and the two passes that carry over what a frame did not draw.
 */
struct sdv_vis {
    rt::DevBuf<uint32_t> d_canvas[10];  /* per kind: the canvas as the last frame of the last call left it (RenderPCM::img_data) */
    rt::DevBuf<uint32_t> d_cnt, d_base_end, d_base_adv;
    rt::DevBuf<uint32_t> d_frame_adv0, d_wmask;
    rt::DevBuf<uint32_t> d_frame_ofs;
    rt::DevBuf<int32_t> d_last;
};

static sdv_vis *vis_get(sdv_engine *e)
{
    if (e->vis) return e->vis;
    sdv_vis *t = new sdv_vis();
    e->vis = t;
    return t;
}
static void vis_free(sdv_engine *e)
{
    sdv_vis *t = e->vis;
    if (!t) return;
    delete t;
    e->vis = NULL;
}

static int vis_blank(sdv_engine *e, sdv_vis *t, int kind, rt::stream_t s)
{
    const sdvvis::Geometry g = sdvvis::geometry(kind);
    const size_t n_px = (size_t)g.w * g.h;
    RT_CHECK(t->d_canvas[kind].reserve(n_px));
    sdvvis::BlankArgs b; b.canvas = t->d_canvas[kind]; b.n_px = (uint32_t)n_px;
    RT_LAUNCH64(sdv_k_vis_blank, (n_px + 63) / 64, b, s);
    return SDV_OK;
}

extern "C" {

int sdv_vis_canvas_size(int kind, uint32_t *width, uint32_t *height)
{
    kind &= ~SDV_VIS_M2_SAMPLES;            /* (the sample format does not change the canvas) */
    const sdvvis::Geometry g = sdvvis::geometry(kind);
    if (!g.w || !width || !height) return SDV_ERR_BAD_ARG;
    *width = g.w; *height = g.h;
    return SDV_OK;
}

int sdv_vis_reset(sdv_engine *e, int kind, void *stream)
{
    if (!e) return SDV_ERR_BAD_ARG;
    kind &= ~SDV_VIS_M2_SAMPLES;
    if (!sdvvis::geometry(kind).w) { set_error(e, "no such canvas"); return SDV_ERR_BAD_ARG; }
    SDV_ON_DEVICE(e);
    return vis_blank(e, vis_get(e), kind, (rt::stream_t)stream);
}

int sdv_vis_render_lines(sdv_engine *e, int kind, const void *recs, size_t n_recs, uint32_t *out_canvases, size_t canvases_cap, size_t *n_frames, void *stream)
{
    if (!e || !n_frames) return SDV_ERR_BAD_ARG;
    *n_frames = 0;
    const sdvvis::Geometry g = sdvvis::geometry(kind);
    if (!g.w || (kind > SDV_VIS_PCM16X0_LINES && kind != SDV_VIS_PCM1_ASM)) { set_error(e, "no such line canvas"); return SDV_ERR_BAD_ARG; }
    if (n_recs == 0) return SDV_OK;
    if (!recs) { set_error(e, "null line buffer"); return SDV_ERR_NULL_LINES; }
    if (n_recs >= 0x7FFFFFFFu) { set_error(e, "too many line records in one call"); return SDV_ERR_BAD_ARG; }
    rt::stream_t s = (rt::stream_t)stream;
    SDV_ON_DEVICE(e);
    sdv_vis *t = vis_get(e);
    if (!t->d_canvas[kind]) { const int rc = vis_blank(e, t, kind, s); if (rc != SDV_OK) return rc; }

    const size_t n_chunks = (n_recs + 63) / 64;
    RT_CHECK(rt::reserve_all(n_chunks, n_chunks + n_chunks / 4 + 64, t->d_cnt, t->d_base_end, t->d_base_adv));
    sdvvis::VisArgs a;
    memset(&a, 0, sizeof(a));
    a.recs = recs; a.n_recs = (uint32_t)n_recs; a.kind = kind; a.cnt = t->d_cnt; a.base_end = t->d_base_end; a.base_adv = t->d_base_adv;
#define VIS_LAUNCH(what, grid) do { \
        if (kind == SDV_VIS_STC007_LINES) RT_LAUNCH64(sdv_k_vis_##what##_stc007, grid, a, s); \
        else if (kind == SDV_VIS_PCM1_LINES) RT_LAUNCH64(sdv_k_vis_##what##_pcm1, grid, a, s); \
        else if (kind == SDV_VIS_PCM1_ASM) RT_LAUNCH64(sdv_k_vis_##what##_p1asm, grid, a, s); \
        else RT_LAUNCH64(sdv_k_vis_##what##_pcm16x0, grid, a, s); } while (0)
    VIS_LAUNCH(count, n_chunks);
    std::vector<uint32_t> cnt(n_chunks), be(n_chunks), ba(n_chunks);
    RT_CHECK(rt::d2h(cnt.data(), t->d_cnt, n_chunks * sizeof(uint32_t), s));
    uint32_t ends = 0, adv = 0;
    for (size_t c = 0; c < n_chunks; c++) { be[c] = ends; ba[c] = adv; ends += cnt[c] & 0xFFFFu; adv += cnt[c] >> 16; }
    *n_frames = ends;
    if (ends == 0) return SDV_OK;       /* no frame has ended: nothing to hand out (whole frames only, see sdvpcm.h) */
    if (!out_canvases) { set_error(e, "null output buffer"); return SDV_ERR_NULL_BLOCK; }
    if (ends > canvases_cap) { set_error(e, "output buffer too small: " + std::to_string(ends) + " canvases are needed"); return SDV_ERR_BAD_ARG; }
    RT_CHECK(rt::h2d(t->d_base_end, be.data(), n_chunks * sizeof(uint32_t), s));
    RT_CHECK(rt::h2d(t->d_base_adv, ba.data(), n_chunks * sizeof(uint32_t), s));
    RT_CHECK(rt::ssync(s));             /* the host vectors go out of scope with the call */
    const size_t n_cells = (size_t)g.h * g.cells_per_row, stride = (n_cells + 31) / 32;
    RT_CHECK(t->d_frame_adv0.reserve((size_t)ends + 1, (size_t)ends + 1 + ends / 4));
    RT_CHECK(t->d_wmask.reserve((size_t)ends * stride, (size_t)ends * stride + (size_t)ends * stride / 4));
    RT_CHECK(rt::dfill_bytes(t->d_wmask, 0, (size_t)ends * stride * sizeof(uint32_t), s));
    a.frame_adv0 = t->d_frame_adv0; a.n_frames = ends; a.out = out_canvases; a.wmask = t->d_wmask; a.wmask_stride = (uint32_t)stride; a.canvas = t->d_canvas[kind];
    VIS_LAUNCH(index, n_chunks);
    VIS_LAUNCH(draw, n_chunks);
#undef VIS_LAUNCH
    RT_CHECK(t->d_last.reserve(n_cells * (size_t)ends, n_cells * ((size_t)ends + ends / 4 + 1)));
    a.last_drawn = t->d_last; a.n_cells = (uint32_t)n_cells;
    RT_LAUNCH64(sdv_k_vis_last, n_cells, a, s);
    RT_LAUNCH64(sdv_k_vis_fill, (size_t)ends * ((n_cells + 63) / 64), a, s);
    RT_CHECK(rt::d2d(t->d_canvas[kind], out_canvases + (size_t)(ends - 1) * g.w * g.h, (size_t)g.w * g.h * sizeof(uint32_t), s));
    return SDV_OK;
}

/* rows of records, frame by frame: the data blocks (sdv_block_rec) or the assembled lines (sdv_asm_line_rec) */
static int vis_render_rows(sdv_engine *e, int kind, bool asm_lines, const void *blocks, size_t n_blocks, const uint32_t *frame_blocks, size_t n_frames,
                           uint32_t *out_canvases, size_t canvases_cap, void *stream, bool m2 = false)
{
    if (!e) return SDV_ERR_BAD_ARG;
    if (n_frames == 0) return SDV_OK;
    if (!frame_blocks || (n_blocks > 0 && !blocks)) { set_error(e, "null block buffer"); return SDV_ERR_NULL_BLOCK; }
    if (!out_canvases) { set_error(e, "null output buffer"); return SDV_ERR_NULL_BLOCK; }
    if (n_frames > canvases_cap) { set_error(e, "output buffer too small: " + std::to_string(n_frames) + " canvases are needed"); return SDV_ERR_BAD_ARG; }
    if (n_frames >= 0x7FFFFFFFu || n_blocks >= 0xFFFFFFFFu) { set_error(e, "too many frames in one call"); return SDV_ERR_BAD_ARG; }
    std::vector<uint32_t> ofs(n_frames + 1);
    uint64_t at = 0;
    for (size_t f = 0; f < n_frames; f++) { ofs[f] = (uint32_t)at; at += frame_blocks[f]; }
    ofs[n_frames] = (uint32_t)at;
    if (at > n_blocks) { set_error(e, "the frames hold more blocks than were handed over"); return SDV_ERR_BAD_ARG; }
    rt::stream_t s = (rt::stream_t)stream;
    SDV_ON_DEVICE(e);
    sdv_vis *t = vis_get(e);
    if (!t->d_canvas[kind]) { const int rc = vis_blank(e, t, kind, s); if (rc != SDV_OK) return rc; }
    const sdvvis::Geometry g = sdvvis::geometry(kind);
    const size_t n_cells = g.h, stride = (n_cells + 31) / 32, chunks = (g.h + 63) / 64;
    if (at * (kind == SDV_VIS_PCM1_BLOCKS ? (uint64_t)sdvvis::P1BK_ROWS : 1u) >= 0xFFFFFFFFu) { set_error(e, "too many blocks in one call"); return SDV_ERR_BAD_ARG; }
    RT_CHECK(t->d_frame_ofs.reserve(n_frames + 1, n_frames + 1 + n_frames / 4));
    RT_CHECK(t->d_wmask.reserve(n_frames * stride, n_frames * stride + n_frames * stride / 4));
    RT_CHECK(t->d_last.reserve(n_cells * n_frames, n_cells * (n_frames + n_frames / 4 + 1)));
    RT_CHECK(rt::h2d(t->d_frame_ofs, ofs.data(), (n_frames + 1) * sizeof(uint32_t), s));
    RT_CHECK(rt::ssync(s));             /* the host vector goes out of scope with the call */
    RT_CHECK(rt::dfill_bytes(t->d_wmask, 0, n_frames * stride * sizeof(uint32_t), s));
    if (asm_lines) {
        sdvvis::AsmArgs b; b.lines = (const sdv_asm_line_rec *)blocks; b.frame_ofs = t->d_frame_ofs; b.n_frames = (uint32_t)n_frames; b.kind = kind; b.out = out_canvases;
        b.wmask = t->d_wmask; b.wmask_stride = (uint32_t)stride;
        RT_LAUNCH64(sdv_k_vis_draw_asm, n_frames * chunks, b, s);
    } else if (kind == SDV_VIS_PCM16X0_BLOCKS) {
        sdvvis::P16BlkArgs b; b.blocks = (const sdv_pcm16x0_block_rec *)blocks; b.frame_ofs = t->d_frame_ofs; b.n_frames = (uint32_t)n_frames; b.kind = kind; b.out = out_canvases;
        b.wmask = t->d_wmask; b.wmask_stride = (uint32_t)stride;
        RT_LAUNCH64(sdv_k_vis_draw_p16_blocks, n_frames * chunks, b, s);
    } else if (kind == SDV_VIS_PCM1_BLOCKS) {
        sdvvis::P1BlkArgs b; b.blocks = (const sdv_pcm1_block_rec *)blocks; b.frame_ofs = t->d_frame_ofs; b.n_frames = (uint32_t)n_frames; b.kind = kind; b.out = out_canvases;
        b.wmask = t->d_wmask; b.wmask_stride = (uint32_t)stride;
        RT_LAUNCH64(sdv_k_vis_draw_p1_blocks, n_frames * chunks, b, s);
    } else {
        sdvvis::BlkArgs b; b.blocks = (const sdv_block_rec *)blocks; b.frame_ofs = t->d_frame_ofs; b.n_frames = (uint32_t)n_frames; b.kind = kind; b.out = out_canvases;
        b.wmask = t->d_wmask; b.wmask_stride = (uint32_t)stride; b.m2 = m2 ? 1 : 0;
        RT_LAUNCH64(sdv_k_vis_draw_blocks, n_frames * chunks, b, s);
    }
    sdvvis::VisArgs a;
    memset(&a, 0, sizeof(a));
    a.kind = kind; a.n_frames = (uint32_t)n_frames; a.out = out_canvases; a.wmask = t->d_wmask; a.wmask_stride = (uint32_t)stride; a.canvas = t->d_canvas[kind];
    a.last_drawn = t->d_last; a.n_cells = (uint32_t)n_cells;
    RT_LAUNCH64(sdv_k_vis_last, n_cells, a, s);
    RT_LAUNCH64(sdv_k_vis_fill, n_frames * ((n_cells + 63) / 64), a, s);
    RT_CHECK(rt::d2d(t->d_canvas[kind], out_canvases + (n_frames - 1) * (size_t)g.w * g.h, (size_t)g.w * g.h * sizeof(uint32_t), s));
    return SDV_OK;
}

int sdv_vis_render_blocks(sdv_engine *e, int kind, const void *blocks, size_t n_blocks, const uint32_t *frame_blocks, size_t n_frames,
                          uint32_t *out_canvases, size_t canvases_cap, void *stream)
{
    if (!e) return SDV_ERR_BAD_ARG;
    const bool m2 = (kind & SDV_VIS_M2_SAMPLES) != 0;
    kind &= ~SDV_VIS_M2_SAMPLES;
    if (kind != SDV_VIS_STC007_BLOCKS_NTSC && kind != SDV_VIS_STC007_BLOCKS_PAL && kind != SDV_VIS_PCM1_BLOCKS && kind != SDV_VIS_PCM16X0_BLOCKS) { set_error(e, "no such block canvas"); return SDV_ERR_BAD_ARG; }
    if (m2 && kind != SDV_VIS_STC007_BLOCKS_NTSC && kind != SDV_VIS_STC007_BLOCKS_PAL) { set_error(e, "M2 samples are an STC-007 format"); return SDV_ERR_BAD_ARG; }
    return vis_render_rows(e, kind, false, blocks, n_blocks, frame_blocks, n_frames, out_canvases, canvases_cap, stream, m2);
}
int sdv_vis_render_asm_lines(sdv_engine *e, int kind, const sdv_asm_line_rec *lines, size_t n_lines, const uint32_t *frame_lines, size_t n_frames,
                             uint32_t *out_canvases, size_t canvases_cap, void *stream)
{
    if (!e) return SDV_ERR_BAD_ARG;
    if (kind != SDV_VIS_STC007_ASM_NTSC && kind != SDV_VIS_STC007_ASM_PAL) { set_error(e, "no such assembled-lines canvas"); return SDV_ERR_BAD_ARG; }
    return vis_render_rows(e, kind, true, lines, n_lines, frame_lines, n_frames, out_canvases, canvases_cap, stream);
}

} // extern "C"
