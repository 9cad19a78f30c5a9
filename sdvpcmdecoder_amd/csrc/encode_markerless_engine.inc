/*
 * encode_markerless_engine.inc - host side of sdv_encode_markerless_geometry / sdv_encode_markerless_frames (include/sdvpcm.h): the checks and the
 * two launches - the format's words kernel of encode_markerless_device.h, then the raster of encode_device.h or, for a packed out_fmt, of
 * encode_packed_device.h.  Included at the end of engine.inc behind
 * encode_engine.inc, whose buffer checks, raster launch and device buffers it uses; the tape state of sdv_encode_frames is neither read nor written.
 */

struct MlencGeo { int cells, lpft; size_t row_bytes; };

/* what the descriptor asks for, or why it cannot be had */
static int mlenc_geo(const sdv_encode_markerless_desc *d, MlencGeo *g, std::string *why)
{
    if (!d) { *why = "null encode descriptor"; return SDV_ERR_BAD_ARG; }
    if (d->format > SDV_ENC_FMT_PCM16X0_EI) { *why = "unknown format"; return SDV_ERR_BAD_ARG; }
    if (d->field_order > SDV_ENC_BFF) { *why = "unknown field order"; return SDV_ERR_BAD_ARG; }
    const bool pcm1 = d->format == SDV_ENC_FMT_PCM1;
    if (d->header_lines > sdv::MLENC_MAX_HEADER) { *why = "more than " + std::to_string((int)sdv::MLENC_MAX_HEADER) + " header lines"; return SDV_ERR_BAD_ARG; }
    if (!pcm1 && d->header_lines) { *why = "PCM-16x0 has no header lines"; return SDV_ERR_BAD_ARG; }
    if (d->ctrl_flags & ~(SDV_ENC_ML_EMPHASIS | SDV_ENC_ML_RATE_44100 | SDV_ENC_ML_CODE)) { *why = "unknown control bits"; return SDV_ERR_BAD_ARG; }
    if (pcm1 && d->ctrl_flags) { *why = "PCM-1 has no control bits"; return SDV_ERR_BAD_ARG; }
    if (d->width <= 0 || d->height <= 0 || d->width > ENCODE_MAX_DIM || d->height > ENCODE_MAX_DIM) {
        *why = "frame size outside 1.." + std::to_string((int)ENCODE_MAX_DIM); return SDV_ERR_BAD_ARG;
    }
    if (d->data_stop <= d->data_start) { *why = "data_stop is not behind data_start"; return SDV_ERR_BAD_ARG; }
    if (d->white <= d->black) { *why = "white is not above black"; return SDV_ERR_BAD_ARG; }
    g->cells = pcm1 ? sdv::MLENC_PCM1_CELLS : sdv::MLENC_PCM16_CELLS;
    g->lpft = sdv::MLENC_LINES + d->header_lines;
    return encode_out_fmt(d->out_fmt, 2, d->width, &g->row_bytes, why);
}

extern "C" {

int sdv_encode_markerless_geometry(const sdv_encode_markerless_desc *d, size_t *pairs_per_frame, int *lines_per_field, size_t *row_bytes)
{
    MlencGeo g; std::string why;
    const int rc = mlenc_geo(d, &g, &why);
    if (rc != SDV_OK) { set_error(NULL, "sdv_encode_markerless_geometry: " + why); return rc; }
    if (pairs_per_frame) *pairs_per_frame = 2 * (size_t)sdv::MLENC_FIELD_PAIRS;
    if (lines_per_field) *lines_per_field = g.lpft;
    if (row_bytes) *row_bytes = g.row_bytes;
    return SDV_OK;
}

int sdv_encode_markerless_frames(sdv_engine *e, const sdv_encode_markerless_desc *d, const int16_t *pcm, size_t n_pairs, int n_frames,
                                 uint8_t *dst, size_t dst_row_stride, size_t dst_frame_stride, void *stream)
{
    if (!e) return SDV_ERR_BAD_ARG;
    if (n_frames < 0) { set_error(e, "negative frame count"); return SDV_ERR_BAD_ARG; }
    if (n_frames == 0) return SDV_OK;
    if (n_frames > ENCODE_MAX_FRAMES) { set_error(e, "more than " + std::to_string((int)ENCODE_MAX_FRAMES) + " frames in one call"); return SDV_ERR_BAD_ARG; }
    MlencGeo g; std::string why;
    const int rc = mlenc_geo(d, &g, &why);
    if (rc != SDV_OK) { set_error(e, why); return rc; }
    const uint64_t n_fields = 2 * (uint64_t)n_frames, n_lines = n_fields * (uint64_t)g.lpft;
    size_t used_pairs = 0;                              /* the pairs the call reads */
    const int rc_buf = encode_check_buffers(e, g.row_bytes, d->height, pcm, n_pairs, n_fields * sdv::MLENC_FIELD_PAIRS, n_frames, dst, dst_row_stride, dst_frame_stride,
                                            &used_pairs);
    if (rc_buf != SDV_OK) return rc_buf;
    SDV_ON_DEVICE(e);
    sdv_encoder *t = e->enc;
    if (!t) t = e->enc = new sdv_encoder();             /* (its buffers; the tape of sdv_encode_frames stays fresh, or where it is) */
    RT_CHECK(t->d_lines.reserve((size_t)n_lines * sdv::ENC_REC_DWORDS));
    RT_CHECK(t->d_cell_of.reserve((size_t)d->width + 2 * sdv::ENC_TABLE_PAD, ENCODE_MAX_DIM + 2 * sdv::ENC_TABLE_PAD));
    const rt::stream_t s = (rt::stream_t)stream;

    sdv::MlencWordsArgs w;
    w.pcm = (const uint8_t *)pcm; w.n_pairs = used_pairs;
    w.lines = t->d_lines;
    w.cell_of = t->d_cell_of; w.width = d->width; w.data_start = d->data_start; w.span = (int64_t)d->data_stop - (int64_t)d->data_start;
    w.n_lines = n_lines; w.lpft = g.lpft; w.header = d->header_lines; w.cells = g.cells;
    w.ei = d->format == SDV_ENC_FMT_PCM16X0_EI; w.ctrl_flags = d->ctrl_flags;
    const uint64_t word_threads = n_lines + (uint64_t)d->width + 2 * sdv::ENC_TABLE_PAD;      /* a line or an entry of the cell table each */
    if (d->format == SDV_ENC_FMT_PCM1) RT_CHECK(RT_LAUNCH_ITEMS(sdv_k_mlenc_pcm1_words, sdv::mlenc_pcm1_words_body, 0, word_threads, 256, s, w));
    else RT_CHECK(RT_LAUNCH_ITEMS(sdv_k_mlenc_pcm16_words, sdv::mlenc_pcm16_words_body, 0, word_threads, 256, s, w));

    const EncodeRaster r = { d->width, d->height, d->top_line, g.lpft, g.cells, w.span, d->field_order == SDV_ENC_BFF, d->black, d->white, d->out_fmt[0], g.row_bytes };
    return encode_launch_raster(e, t, r, n_frames, dst, dst_row_stride, dst_frame_stride, s);
}

} /* extern "C" */
