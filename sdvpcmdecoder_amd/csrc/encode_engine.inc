/*
 * encode_engine.inc - host side of sdv_encode_geometry / sdv_encode_frames / sdv_reset_encoder (include/sdvpcm.h): the checks, the tape's
 * state and the two launches of encode_device.h.  Included at the end of engine.inc, so by the one translation unit of either build.
 * encode_out_fmt, encode_check_buffers and encode_launch_raster also serve encode_markerless_engine.inc; encode_launch_raster is the one place that
 * chooses between sdv_k_encode_raster (SDV_PIX_GRAY8) and a build of sdv_k_encode_raster_packed (encode_packed_device.h).
 */

enum { ENCODE_MAX_DIM = 32768, ENCODE_MAX_FRAMES = 1 << 24 };

struct sdv_encoder {
    bool fresh = true;                              /* no call since the engine was made or sdv_reset_encoder */
    uint8_t video_standard = 0, resolution = 0, ctrl_block = 0;     /* of the tape: the first call's */
    rt::DevBuf<sdv::EncodeState> d_state, d_state_next;             /* what the next call reads, what this one writes */
    rt::DevBuf<uint32_t> d_lines;                   /* the packed lines of a call */
    rt::DevBuf<uint8_t> d_cell_of;                  /* the cell of every x of a row, and of 16 on either side of it */
};

static void encoder_free(sdv_engine *e) { delete e->enc; e->enc = NULL; }

/* out_fmt of a descriptor (`n` bytes, the first an SDV_PIX_* value, the rest reserved) for rows of `width` pixels: the bytes of a row, or why not */
static int encode_out_fmt(const uint8_t *out_fmt, int n, int width, size_t *row_bytes, std::string *why)
{
    if (out_fmt[0] > SDV_PIX_BGR0) { *why = "unknown output pixel format (out_fmt[0] is an SDV_PIX_* value)"; return SDV_ERR_BAD_ARG; }
    for (int i = 1; i < n; i++) if (out_fmt[i]) { *why = "the reserved bytes of out_fmt are not 0"; return SDV_ERR_BAD_ARG; }
    const size_t w = (size_t)width;
    switch (out_fmt[0]) {
    case SDV_PIX_GRAY8: *row_bytes = w; break;
    case SDV_PIX_UYVY422: case SDV_PIX_YUYV422: *row_bytes = 4 * ((w + 1) / 2); break;
    case SDV_PIX_V210: *row_bytes = 16 * ((w + 5) / 6); break;
    case SDV_PIX_GRAY10LE: *row_bytes = 2 * w; break;
    case SDV_PIX_RGB24: case SDV_PIX_BGR24: *row_bytes = 3 * w; break;
    default: *row_bytes = 4 * w; break;                 /* SDV_PIX_RGB0, SDV_PIX_BGR0 */
    }
    return SDV_OK;
}

struct EncodeGeo { int lpf, lpft; uint32_t fps; size_t row_bytes; };

/* what the descriptor asks for, or why it cannot be had */
static int encode_geo(const sdv_encode_desc *d, EncodeGeo *g, std::string *why)
{
    if (!d) { *why = "null encode descriptor"; return SDV_ERR_BAD_ARG; }
    if (d->video_standard > SDV_ENC_PAL) { *why = "unknown video standard"; return SDV_ERR_BAD_ARG; }
    if (d->resolution > SDV_ENC_16BIT) { *why = "unknown resolution"; return SDV_ERR_BAD_ARG; }
    if (d->ctrl_block > 1) { *why = "ctrl_block is 0 or 1"; return SDV_ERR_BAD_ARG; }
    if (d->ctrl_flags & ~(SDV_ENC_CTRL_COPY_PROHIBITED | SDV_ENC_CTRL_EMPHASIS)) { *why = "unknown control bits (the P word cannot be left out)"; return SDV_ERR_BAD_ARG; }
    if (d->field_order > SDV_ENC_BFF) { *why = "unknown field order"; return SDV_ERR_BAD_ARG; }
    if (d->width <= 0 || d->height <= 0 || d->width > ENCODE_MAX_DIM || d->height > ENCODE_MAX_DIM) {
        *why = "frame size outside 1.." + std::to_string((int)ENCODE_MAX_DIM); return SDV_ERR_BAD_ARG;
    }
    if (d->data_stop <= d->data_start) { *why = "data_stop is not behind data_start"; return SDV_ERR_BAD_ARG; }
    if (d->white <= d->black) { *why = "white is not above black"; return SDV_ERR_BAD_ARG; }
    g->lpf = d->video_standard == SDV_ENC_PAL ? 294 : 245;          /* config.h:80-81 */
    g->lpft = g->lpf + d->ctrl_block;
    g->fps = d->video_standard == SDV_ENC_PAL ? 50 : 60;
    if (d->tc_index > 63 || d->tc_hour > 15 || d->tc_minute > 59 || d->tc_second > 59 || d->tc_field >= g->fps) { *why = "time code out of range"; return SDV_ERR_BAD_ARG; }
    return encode_out_fmt(d->out_fmt, 3, d->width, &g->row_bytes, why);
}

/* The pointers and strides of a call that makes n_frames frames of `height` rows of row_bytes bytes (the out_fmt's) from at most call_pairs pairs -
 * the checks of sdv_encode_frames and sdv_encode_markerless_frames behind those of their descriptors.  *used_pairs: the pairs the call reads. */
static int encode_check_buffers(sdv_engine *e, size_t row_bytes, int height, const int16_t *pcm, size_t n_pairs, uint64_t call_pairs, int n_frames,
                                const uint8_t *dst, size_t dst_row_stride, size_t dst_frame_stride, size_t *used_pairs)
{
    if (!pcm && n_pairs > 0) { set_error(e, "null pcm"); return SDV_ERR_NULL_PCM; }
    if (!dst) { set_error(e, "null video"); return SDV_ERR_NULL_VIDEO; }
    const size_t max_stride = (size_t)1 << 32;          /* (keeps the spans below inside 64 bits) */
    if (dst_row_stride > max_stride || (n_frames > 1 && dst_frame_stride > max_stride)) { set_error(e, "stride above 4 GiB"); return SDV_ERR_BAD_ARG; }
    const size_t dst_frame = (size_t)(height - 1) * dst_row_stride + row_bytes;
    if (dst_row_stride < row_bytes) { set_error(e, "dst_row_stride smaller than the " + std::to_string(row_bytes) + " bytes of a row"); return SDV_ERR_BAD_ARG; }
    if (n_frames > 1 && dst_frame_stride < dst_frame) { set_error(e, "dst_frame_stride smaller than one frame"); return SDV_ERR_BAD_ARG; }
    *used_pairs = n_pairs < call_pairs ? n_pairs : (size_t)call_pairs;
    const uintptr_t s0 = (uintptr_t)pcm, s1 = s0 + 4 * *used_pairs;
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (size_t)(n_frames - 1) * dst_frame_stride + dst_frame;
    if (*used_pairs && s0 < d1 && d0 < s1) { set_error(e, "pcm and destination overlap"); return SDV_ERR_BAD_ARG; }
    return SDV_OK;
}

/* what the raster shows: the packed lines and the cell table of `t`, lpft lines a field with `cells` cells each */
struct EncodeRaster { int width, height, top_line, lpft, cells; int64_t span; bool bff; uint8_t black, white; uint8_t out_fmt; size_t row_bytes; };

/* the build of sdv_k_encode_raster_packed for a format family: `threads` threads, a grid stride walks the rest (encode_packed_body) */
template <int FAM> static inline rt::status_t launch_encode_packed(sdv::EncodePackedArgs &p, uint64_t rows, rt::stream_t s)
{
    sdv::EncodeRasterArgs &a = p.r;
    a.slots = sdv::EncodePackedShape<FAM>::slots(a.width);
    const uint32_t threads = rt::grid_stride_threads(rows * (uint64_t)a.slots);
    const rt::StrideSteps st = rt::stride_steps(threads, (uint32_t)a.height, (uint32_t)a.slots);
    a.step_f = st.step_f; a.step_r = st.step_r; a.step_c = st.step_c;
    return RT_LAUNCH_ITEMS((sdv_k_encode_raster_packed<FAM>), (sdv::encode_packed_body<FAM>), 0u, threads, 256, s, p);
}

/* the raster launch of a call: the same for every tape format; SDV_PIX_GRAY8 by encode_raster_body, any other out_fmt by its family's encode_packed_body */
static int encode_launch_raster(sdv_engine *e, sdv_encoder *t, const EncodeRaster &r, int n_frames, uint8_t *dst, size_t dst_row_stride, size_t dst_frame_stride,
                                rt::stream_t s)
{
    sdv::EncodeRasterArgs a;
    a.lines = t->d_lines; a.cell_of = t->d_cell_of.p + sdv::ENC_TABLE_PAD;
    a.dst = dst; a.dst_row_stride = dst_row_stride; a.dst_frame_stride = dst_frame_stride;
    a.n_frames = n_frames; a.width = r.width; a.height = r.height; a.line_rows = r.height & ~1;
    a.lpft = r.lpft; a.bff = r.bff;
    /* any top_line at or beyond these bounds leaves no row with a line, as the bound itself does: no overflow in the kernel */
    a.top_line = r.top_line < -ENCODE_MAX_DIM ? -ENCODE_MAX_DIM : r.top_line > r.lpft ? r.lpft : r.top_line;
    a.black4 = 0x01010101u * r.black; a.white4 = 0x01010101u * r.white;
    /* cells 15 pixels apart are at most 15 * cells / span, rounded up, apart, and a step more at a window edge: beyond 31 the raster's window does not hold them */
    a.narrow = (15 * (int64_t)r.cells) / r.span + 2 > 31;
    if (r.out_fmt != SDV_PIX_GRAY8) {
        sdv::EncodePackedArgs p;
        p.r = a; p.row_bytes = (uint32_t)r.row_bytes;
        p.narrow_quad = ((sdv::ENCP_QUAD_PX - 1) * (int64_t)r.cells) / r.span + 2 > 31;         /* the same rule for the 64 pixels the lanes of a quad share */
        const uint64_t rows = (uint64_t)n_frames * (uint64_t)r.height;
        switch (r.out_fmt) {
        case SDV_PIX_UYVY422: RT_CHECK(launch_encode_packed<sdv::ENCP_UYVY>(p, rows, s)); break;
        case SDV_PIX_YUYV422: RT_CHECK(launch_encode_packed<sdv::ENCP_YUYV>(p, rows, s)); break;
        case SDV_PIX_V210: RT_CHECK(launch_encode_packed<sdv::ENCP_V210>(p, rows, s)); break;
        case SDV_PIX_GRAY10LE: RT_CHECK(launch_encode_packed<sdv::ENCP_GRAY10>(p, rows, s)); break;
        case SDV_PIX_RGB24: case SDV_PIX_BGR24: RT_CHECK(launch_encode_packed<sdv::ENCP_RGB3>(p, rows, s)); break;
        case SDV_PIX_RGB0: case SDV_PIX_BGR0: RT_CHECK(launch_encode_packed<sdv::ENCP_RGB4>(p, rows, s)); break;
        default: set_error(e, "no raster kernel for this out_fmt"); return SDV_ERR_BAD_ARG;      /* (encode_out_fmt has refused it) */
        }
        return SDV_OK;
    }
    a.slots = (r.width + 30) / 16;
    /* threads of the raster launch: a grid stride walks the rest (encode_raster_body) */
    const uint32_t threads = rt::grid_stride_threads((uint64_t)n_frames * (uint64_t)r.height * (uint64_t)a.slots);
    const rt::StrideSteps st = rt::stride_steps(threads, (uint32_t)r.height, (uint32_t)a.slots);
    a.step_f = st.step_f; a.step_r = st.step_r; a.step_c = st.step_c;
    RT_CHECK(RT_LAUNCH_ITEMS(sdv_k_encode_raster, sdv::encode_raster_body, 0u, threads, 256, s, a));
    return SDV_OK;
}

extern "C" {

int sdv_encode_geometry(const sdv_encode_desc *d, size_t *pairs_per_frame, int *lines_per_field, size_t *row_bytes)
{
    EncodeGeo g; std::string why;
    const int rc = encode_geo(d, &g, &why);
    if (rc != SDV_OK) { set_error(NULL, "sdv_encode_geometry: " + why); return rc; }
    if (pairs_per_frame) *pairs_per_frame = (size_t)g.lpf * 6;
    if (lines_per_field) *lines_per_field = g.lpft;
    if (row_bytes) *row_bytes = g.row_bytes;
    return SDV_OK;
}

int sdv_reset_encoder(sdv_engine *e)
{
    if (!e) return SDV_ERR_BAD_ARG;
    if (e->enc) e->enc->fresh = true;
    return SDV_OK;
}

int sdv_encode_frames(sdv_engine *e, const sdv_encode_desc *d, const int16_t *pcm, size_t n_pairs, int n_frames,
                      uint8_t *dst, size_t dst_row_stride, size_t dst_frame_stride, void *stream)
{
    if (!e) return SDV_ERR_BAD_ARG;
    if (n_frames < 0) { set_error(e, "negative frame count"); return SDV_ERR_BAD_ARG; }
    if (n_frames == 0) return SDV_OK;
    if (n_frames > ENCODE_MAX_FRAMES) { set_error(e, "more than " + std::to_string((int)ENCODE_MAX_FRAMES) + " frames in one call"); return SDV_ERR_BAD_ARG; }
    EncodeGeo g; std::string why;
    const int rc = encode_geo(d, &g, &why);
    if (rc != SDV_OK) { set_error(e, why); return rc; }
    const uint64_t n_fields = 2 * (uint64_t)n_frames, n_data = n_fields * (uint64_t)g.lpf, n_lines = n_fields * (uint64_t)g.lpft;
    size_t used_pairs = 0;                              /* the pairs the call reads */
    const int rc_buf = encode_check_buffers(e, g.row_bytes, d->height, pcm, n_pairs, 3 * n_data, n_frames, dst, dst_row_stride, dst_frame_stride, &used_pairs);
    if (rc_buf != SDV_OK) return rc_buf;
    sdv_encoder *t = e->enc;
    if (t && !t->fresh && (t->video_standard != d->video_standard || t->resolution != d->resolution || t->ctrl_block != d->ctrl_block)) {
        set_error(e, "video standard, resolution and control block stay as the tape began: sdv_reset_encoder starts another tape"); return SDV_ERR_BAD_ARG;
    }
    SDV_ON_DEVICE(e);
    if (!t) t = e->enc = new sdv_encoder();
    RT_CHECK(rt::reserve_all(1, 1, t->d_state, t->d_state_next));
    RT_CHECK(t->d_lines.reserve((size_t)n_lines * sdv::ENC_REC_DWORDS));
    RT_CHECK(t->d_cell_of.reserve((size_t)d->width + 2 * sdv::ENC_TABLE_PAD, ENCODE_MAX_DIM + 2 * sdv::ENC_TABLE_PAD));
    const rt::stream_t s = (rt::stream_t)stream;

    sdv::EncodeWordsArgs w;
    w.pcm = (const uint8_t *)pcm; w.n_pairs = used_pairs;
    w.st_in = t->d_state; w.st_out = t->d_state_next;
    w.lines = t->d_lines;
    w.cell_of = t->d_cell_of; w.width = d->width; w.data_start = d->data_start; w.span = (int64_t)d->data_stop - (int64_t)d->data_start;
    w.n_lines = n_lines; w.n_data = n_data; w.lpf = g.lpf; w.lpft = g.lpft;
    w.fps = g.fps; w.tc_wrap = 16u * 3600u * g.fps;
    w.tc0 = (((uint32_t)d->tc_hour * 60u + d->tc_minute) * 60u + d->tc_second) * g.fps + d->tc_field;
    w.addr1_index = (uint16_t)(d->tc_index << 8);
    /* CTRL_COPY_MASK 8, CTRL_EN_Q_MASK 2 (set: no Q word, 16 bit), CTRL_EMPH_MASK 1 (set: no emphasis), stc007line.h:143-152 */
    w.ctrl_word = (uint16_t)((d->ctrl_flags & SDV_ENC_CTRL_COPY_PROHIBITED ? 8 : 0) | (d->resolution == SDV_ENC_16BIT ? 2 : 0) | (d->ctrl_flags & SDV_ENC_CTRL_EMPHASIS ? 0 : 1));
    w.ctrl = d->ctrl_block; w.res16 = d->resolution == SDV_ENC_16BIT; w.fresh = t->fresh;
    const uint64_t word_threads = n_lines + (uint64_t)d->width + 2 * sdv::ENC_TABLE_PAD;      /* a line or an entry of the cell table each */
    RT_CHECK(RT_LAUNCH_ITEMS(sdv_k_encode_words, sdv::encode_words_body, 0, word_threads, 256, s, w));

    const EncodeRaster r = { d->width, d->height, d->top_line, g.lpft, sdv::ENC_CELLS, w.span, d->field_order == SDV_ENC_BFF, d->black, d->white, d->out_fmt[0], g.row_bytes };
    const int rc_raster = encode_launch_raster(e, t, r, n_frames, dst, dst_row_stride, dst_frame_stride, s);
    if (rc_raster != SDV_OK) return rc_raster;

    t->d_state.swap(t->d_state_next);
    t->video_standard = d->video_standard; t->resolution = d->resolution; t->ctrl_block = d->ctrl_block; t->fresh = false;
    return SDV_OK;
}

} /* extern "C" */
