/*
 * ingest_engine.inc - host side of sdv_ingest_geometry / sdv_ingest_frames (include/sdvpcm.h): the checks, the geometry and the launch of
 * sdv_k_ingest (ingest_device.h).  Included at the end of engine.inc, so by the one translation unit of either build.
 *
 * The crop, plane and doubling rules are the reference's (vid_preset_t.h:30-45, ffmpegwrapper.cpp:847-869, :199-251, :254-300); the sample
 * values are the header's integer formulas, not libswscale's.
 */

/* the build of sdv_k_ingest for a format family, with or without the doubling: `threads` threads, a grid stride walks the rest (ingest_body) */
template <int FAM> static inline rt::status_t launch_ingest_fam(const sdv::IngestArgs &a, bool dbl, uint32_t threads, rt::stream_t s)
{
    if (dbl) return RT_LAUNCH_ITEMS((sdv_k_ingest<FAM, true>), (sdv::ingest_body<FAM, true>), 0u, threads, 256, s, a);
    return RT_LAUNCH_ITEMS((sdv_k_ingest<FAM, false>), (sdv::ingest_body<FAM, false>), 0u, threads, 256, s, a);
}
static inline rt::status_t launch_ingest(const sdv::IngestArgs &a, int fam, bool dbl, uint32_t threads, rt::stream_t s)
{
    switch (fam) {
    case sdv::ING_GRAY8: return launch_ingest_fam<sdv::ING_GRAY8>(a, dbl, threads, s);
    case sdv::ING_UYVY: return launch_ingest_fam<sdv::ING_UYVY>(a, dbl, threads, s);
    case sdv::ING_YUYV: return launch_ingest_fam<sdv::ING_YUYV>(a, dbl, threads, s);
    case sdv::ING_V210: return launch_ingest_fam<sdv::ING_V210>(a, dbl, threads, s);
    case sdv::ING_GRAY10: return launch_ingest_fam<sdv::ING_GRAY10>(a, dbl, threads, s);
    case sdv::ING_RGB3: return launch_ingest_fam<sdv::ING_RGB3>(a, dbl, threads, s);
    default: return launch_ingest_fam<sdv::ING_RGB4>(a, dbl, threads, s);
    }
}

enum { INGEST_MAX_DIM = 32768, INGEST_MAX_LINES = 640 /* LINES_PER_FRAME_MAX */ };

struct IngestGeo {
    int fam, crop_bottom, kept_w, out_w, out_h, doubled;
    size_t row_bytes;
    uint32_t wt[3];
};

/* what the descriptor asks for, or why it cannot be had: SDV_OK, SDV_ERR_BAD_ARG or SDV_ERR_UNSUPPORTED */
static int ingest_geo(const sdv_ingest_desc *d, IngestGeo *g, std::string *why)
{
    if (!d) { *why = "null ingest descriptor"; return SDV_ERR_BAD_ARG; }
    if (d->pix_fmt > SDV_PIX_BGR0) { *why = "unknown pixel format"; return SDV_ERR_BAD_ARG; }
    if (d->colors > SDV_COLOR_B) { *why = "unknown colour channel"; return SDV_ERR_BAD_ARG; }
    if (d->double_width > SDV_INGEST_DOUBLE_AUTO) { *why = "unknown doubling mode"; return SDV_ERR_BAD_ARG; }
    if (d->src_width <= 0 || d->src_height <= 0 || d->src_width > INGEST_MAX_DIM || d->src_height > INGEST_MAX_DIM) {
        *why = "source frame size outside 1.." + std::to_string((int)INGEST_MAX_DIM); return SDV_ERR_BAD_ARG;
    }
    const bool rgb = d->pix_fmt >= SDV_PIX_RGB24;
    if (d->colors != SDV_COLOR_BW && !rgb) {
        /* the reference would have swscale convert YUV to GBR planes (ffmpegwrapper.cpp:199-251); PCM video carries no chroma to select from */
        *why = "a colour channel can only be picked from an RGB format"; return SDV_ERR_UNSUPPORTED;
    }
    const size_t w = (size_t)d->src_width;
    switch (d->pix_fmt) {
    case SDV_PIX_GRAY8: g->fam = sdv::ING_GRAY8; g->row_bytes = w; break;
    case SDV_PIX_UYVY422: g->fam = sdv::ING_UYVY; g->row_bytes = 4 * ((w + 1) / 2); break;
    case SDV_PIX_YUYV422: g->fam = sdv::ING_YUYV; g->row_bytes = 4 * ((w + 1) / 2); break;
    case SDV_PIX_V210: g->fam = sdv::ING_V210; g->row_bytes = 16 * ((w + 5) / 6); break;
    case SDV_PIX_GRAY10LE: g->fam = sdv::ING_GRAY10; g->row_bytes = 2 * w; break;
    case SDV_PIX_RGB24: case SDV_PIX_BGR24: g->fam = sdv::ING_RGB3; g->row_bytes = 3 * w; break;
    default: g->fam = sdv::ING_RGB4; g->row_bytes = 4 * w; break;
    }
    g->wt[0] = g->wt[1] = g->wt[2] = 0;
    if (rgb) {
        const bool bgr = d->pix_fmt == SDV_PIX_BGR24 || d->pix_fmt == SDV_PIX_BGR0;
        const int at_r = bgr ? 2 : 0, at_b = bgr ? 0 : 2;
        if (d->colors == SDV_COLOR_BW) { g->wt[at_r] = 77; g->wt[1] = 150; g->wt[at_b] = 29; }
        else g->wt[d->colors == SDV_COLOR_R ? at_r : d->colors == SDV_COLOR_G ? 1 : at_b] = 256;
    }
    /* more lines than a frame can have: the bottom goes, whatever was asked for (ffmpegwrapper.cpp:850-854) */
    g->crop_bottom = d->src_height > INGEST_MAX_LINES ? d->src_height - INGEST_MAX_LINES : (int)d->crop_bottom;
    g->kept_w = d->src_width - (int)d->crop_left - (int)d->crop_right;
    g->out_h = d->src_height - (int)d->crop_top - g->crop_bottom;
    if (g->kept_w <= 0 || g->out_h <= 0) { *why = "the crop leaves nothing of the frame"; return SDV_ERR_BAD_ARG; }
    /* doubling is decided on the cropped width (keepFrameInCheck, ffmpegwrapper.cpp:279-285) */
    g->doubled = d->double_width == SDV_INGEST_DOUBLE_AUTO ? sdv_needs_double_width(g->kept_w) : d->double_width == SDV_INGEST_DOUBLE_ON;
    g->out_w = g->doubled ? 2 * g->kept_w : g->kept_w;
    return SDV_OK;
}

extern "C" {

int sdv_ingest_geometry(const sdv_ingest_desc *d, int *out_width, int *out_height, int *doubled, size_t *src_row_bytes)
{
    IngestGeo g; std::string why;
    const int rc = ingest_geo(d, &g, &why);
    if (rc != SDV_OK) { set_error(NULL, "sdv_ingest_geometry: " + why); return rc; }
    if (out_width) *out_width = g.out_w;
    if (out_height) *out_height = g.out_h;
    if (doubled) *doubled = g.doubled;
    if (src_row_bytes) *src_row_bytes = g.row_bytes;
    return SDV_OK;
}

int sdv_ingest_frames(sdv_engine *e, const sdv_ingest_desc *d, const void *src, size_t src_row_stride, size_t src_frame_stride,
                      int n_frames, uint8_t *dst, size_t dst_row_stride, size_t dst_frame_stride, void *stream)
{
    if (!e) return SDV_ERR_BAD_ARG;
    if (n_frames < 0) { set_error(e, "negative frame count"); return SDV_ERR_BAD_ARG; }
    if (n_frames == 0) return SDV_OK;
    IngestGeo g; std::string why;
    const int rc = ingest_geo(d, &g, &why);
    if (rc != SDV_OK) { set_error(e, why); return rc; }
    if (!src) { set_error(e, "null video"); return SDV_ERR_NULL_VIDEO; }
    if (!dst) { set_error(e, "null output"); return SDV_ERR_NULL_PCM; }
    const size_t max_stride = (size_t)1 << 32;          /* (keeps the spans below inside 64 bits) */
    if (src_row_stride > max_stride || dst_row_stride > max_stride || (n_frames > 1 && (src_frame_stride > max_stride || dst_frame_stride > max_stride))) {
        set_error(e, "stride above 4 GiB"); return SDV_ERR_BAD_ARG;
    }
    const size_t src_frame = (size_t)(d->src_height - 1) * src_row_stride + g.row_bytes, dst_frame = (size_t)(g.out_h - 1) * dst_row_stride + (size_t)g.out_w;
    if (src_row_stride < g.row_bytes) { set_error(e, "src_row_stride smaller than the " + std::to_string(g.row_bytes) + " bytes of a source row"); return SDV_ERR_BAD_ARG; }
    if (dst_row_stride < (size_t)g.out_w) { set_error(e, "dst_row_stride smaller than the " + std::to_string(g.out_w) + " bytes of a destination row"); return SDV_ERR_BAD_ARG; }
    if (n_frames > 1 && src_frame_stride < src_frame) { set_error(e, "src_frame_stride smaller than one frame"); return SDV_ERR_BAD_ARG; }
    if (n_frames > 1 && dst_frame_stride < dst_frame) { set_error(e, "dst_frame_stride smaller than one frame"); return SDV_ERR_BAD_ARG; }
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (size_t)(n_frames - 1) * src_frame_stride + src_frame;
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (size_t)(n_frames - 1) * dst_frame_stride + dst_frame;
    if (s0 < d1 && d0 < s1) { set_error(e, "source and destination overlap"); return SDV_ERR_BAD_ARG; }
    SDV_ON_DEVICE(e);
    sdv::IngestArgs a;
    a.src = (const uint8_t *)src; a.src_row_stride = src_row_stride; a.src_frame_stride = src_frame_stride;
    a.dst = dst; a.dst_row_stride = dst_row_stride; a.dst_frame_stride = dst_frame_stride;
    a.n_frames = n_frames; a.out_w = g.out_w; a.out_h = g.out_h; a.crop_left = d->crop_left; a.crop_top = d->crop_top;
    a.src_row_bytes = (uint32_t)g.row_bytes;
    a.slots = (g.out_w + 30) / 16;
    a.wt[0] = g.wt[0]; a.wt[1] = g.wt[1]; a.wt[2] = g.wt[2];
    const uint32_t threads = rt::grid_stride_threads((uint64_t)n_frames * (uint64_t)g.out_h * (uint64_t)a.slots);
    const rt::StrideSteps st = rt::stride_steps(threads, (uint32_t)g.out_h, (uint32_t)a.slots);
    a.step_f = st.step_f; a.step_r = st.step_r; a.step_c = st.step_c;
    RT_CHECK(launch_ingest(a, g.fam, g.doubled != 0, threads, (rt::stream_t)stream));
    return SDV_OK;
}

} /* extern "C" */
