/*
 * pcm1_frames_engine.inc - sdv_pcm1_binarize_frames (include/sdvpcm.h): what the scheduler of markerless_frames_engine.inc is told about PCM-1;
 * behind it the host side of sdv_pcm1_binarize_lines.  Included after pcm1_engine.inc by the same two translation units.
 */
#include "markerless_frames_engine.inc"

struct Pcm1Frames {
    typedef sdv_pcm1_bin_rec Rec;
    typedef sdv_v2d_state State;
    typedef sdvp1f::FrameArgs1 Args;
    enum { MIN_WIDTH = sdvp1b::P1_BITS, LINES_PER_ROW = 1 };
    static constexpr const char *TRACE_TAG = "sched1";
    static const char *short_line() { return "line shorter than the 94 bit cells of a PCM-1 line"; }
    static const char *rec_noun() { return "line records"; }
    static size_t records_needed(int height, int n_frames, unsigned flags) { return sdv_binarize_records(height, n_frames, flags); }
    static State &chain(sdv_engine *e) { return e->chain; }
    static rt::DevBuf<State> &states_in(sdv_engine *e) { return e->d_states_in; }
    static rt::DevBuf<State> &states_out(sdv_engine *e) { return e->d_states_out; }
    static rt::status_t reserve_states(sdv_engine *, size_t) { return rt::OK; }        /* (ensure_capacity has) */
    static rt::DevBuf<uint8_t> &prescan_buf(sdv_engine *e) { return pcm1_get(e)->d_prescan; }
    static void bind(Args &a, State *in, State *out, Rec *recs) { a.f.states_in = in; a.f.states_out = out; a.recs1 = recs; }
    static constexpr auto k_prescan = sdv_k_pcm1_prescan, k_prescan_insane = sdv_k_pcm1_prescan_insane, k_lean = sdv_k_pcm1_frames_lean,
                          k_bin = sdv_k_pcm1_frames_bin, k_bin_insane = sdv_k_pcm1_frames_bin_insane;
    static constexpr auto k_predict = sdv_k_pcm1_predict;
    static constexpr auto k_repair = sdv_k_pcm1_repair;
    static constexpr auto k_verify = sdv_k_pcm1_verify;
};

extern "C" int sdv_pcm1_binarize_frames(sdv_engine *e, const uint8_t *luma, size_t row_stride, size_t frame_stride, int width, int height,
                                        int n_frames, uint32_t first_frame_no, unsigned flags, sdv_pcm1_bin_rec *out_lines, size_t lines_cap,
                                        sdv_frame_stats *out_stats, size_t stats_cap, void *stream)
{
    return markerless_binarize_frames<Pcm1Frames>(e, luma, row_stride, frame_stride, width, height, n_frames, first_frame_no, flags, out_lines, lines_cap, out_stats, stats_cap, stream);
}

/* ---- PCM-1 front half: Binarizer::processLine with a PCM1Line output, n_lines lines per launch (pcm1_bin_device.h) -------- */
extern "C" int sdv_pcm1_binarize_lines(sdv_engine *e, const uint8_t *luma, size_t row_stride, int width, size_t n_lines,
                                       const sdv_bin_state *presets, uint32_t frame_number, uint16_t first_line, uint16_t line_step,
                                       unsigned flags, int coord_search, sdv_pcm1_bin_rec *out_lines, size_t lines_cap, void *stream)
{
    bool todo = false;
    { const int rc = check_lines_call<Pcm1Frames>(e, luma, row_stride, width, n_lines, out_lines, lines_cap, &todo); if (rc != SDV_OK || !todo) return rc; }
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
