/*
 * pcm16_frames_engine.inc - sdv_pcm16x0_binarize_frames (include/sdvpcm.h): what the scheduler of markerless_frames_engine.inc is told about
 * PCM-16x0; behind it the host side of sdv_pcm16x0_binarize_lines.
 */
#include "markerless_frames_engine.inc"

struct Pcm16Frames {
    typedef sdv_pcm16x0_bin_rec Rec;
    typedef sdvp16f::State16 State;
    typedef sdvp16f::FrameArgs16 Args;
    enum { MIN_WIDTH = sdvp16::P16_BITS, LINES_PER_ROW = 3 };          /* coordinate lists: three sub-lines per line */
    static constexpr const char *TRACE_TAG = "sched16";
    static const char *short_line() { return "line shorter than the 193 bit cells of a PCM-16x0 line"; }
    static const char *rec_noun() { return "sub-line records"; }
    static size_t records_needed(int height, int n_frames, unsigned flags) { return sdv_pcm16x0_binarize_records(height, n_frames, flags); }
    static State &chain(sdv_engine *e) { return e->chain16; }
    static rt::DevBuf<State> &states_in(sdv_engine *e) { return e->d_states16_in; }
    static rt::DevBuf<State> &states_out(sdv_engine *e) { return e->d_states16_out; }
    static rt::status_t reserve_states(sdv_engine *e, size_t n) { return rt::reserve_all(n, n, e->d_states16_in, e->d_states16_out); }
    static rt::DevBuf<uint8_t> &prescan_buf(sdv_engine *e) { return e->d_prescan16; }
    static void bind(Args &a, State *in, State *out, Rec *recs) { a.states_in = in; a.states_out = out; a.recs16 = recs; }
    static constexpr auto k_prescan = sdv_k_pcm16_prescan, k_prescan_insane = sdv_k_pcm16_prescan_insane, k_lean = sdv_k_pcm16_frames_lean,
                          k_bin = sdv_k_pcm16_frames_bin, k_bin_insane = sdv_k_pcm16_frames_bin_insane;
    static constexpr auto k_predict = sdv_k_pcm16_predict;
    static constexpr auto k_repair = sdv_k_pcm16_repair;
    static constexpr auto k_verify = sdv_k_pcm16_verify;
};

extern "C" int sdv_pcm16x0_binarize_frames(sdv_engine *e, const uint8_t *luma, size_t row_stride, size_t frame_stride, int width, int height,
                                           int n_frames, uint32_t first_frame_no, unsigned flags, sdv_pcm16x0_bin_rec *out_lines, size_t lines_cap,
                                           sdv_frame_stats *out_stats, size_t stats_cap, void *stream)
{
    return markerless_binarize_frames<Pcm16Frames>(e, luma, row_stride, frame_stride, width, height, n_frames, first_frame_no, flags, out_lines, lines_cap, out_stats, stats_cap, stream);
}

/* ---- PCM-16x0 front half, line by line: Binarizer::processLine with a PCM16X0SubLine output, the three passes of n_lines video lines per launch (pcm16_bin_device.h) ---- */
extern "C" int sdv_pcm16x0_binarize_lines(sdv_engine *e, const uint8_t *luma, size_t row_stride, int width, size_t n_lines,
                                          const sdv_bin_state *presets, uint32_t frame_number, uint16_t first_line, uint16_t line_step,
                                          unsigned flags, int coord_search, sdv_pcm16x0_bin_rec *out_lines, size_t lines_cap, uint8_t *out_scan_done, void *stream)
{
    bool todo = false;
    { const int rc = check_lines_call<Pcm16Frames>(e, luma, row_stride, width, n_lines, out_lines, lines_cap, &todo); if (rc != SDV_OK || !todo) return rc; }
    SDV_ON_DEVICE(e);
    sdvp16::LineArgs16 a;
    memset(&a, 0, sizeof(a));
    a.luma = luma; a.row_stride = row_stride; a.width = width; a.n_lines = n_lines; a.states = presets;
    a.frame_number = frame_number; a.first_line = first_line; a.line_step = line_step;
    a.doubled = (flags & SDV_FLAG_DOUBLED) ? 1 : 0; a.mode = (uint8_t)e->mode; a.coord_search = coord_search ? 1 : 0;
    a.preset = e->preset; a.out = out_lines; a.scan_done = out_scan_done;
    rt::stream_t s = (rt::stream_t)stream;
    const size_t grid = n_lines < 8192 ? n_lines : 8192;            /* the kernel walks its lines: 2 x what the chip holds at once */
    if (e->mode == SDV_MODE_INSANE) RT_LAUNCH64(sdv_k_pcm16_lines_insane, grid, a, s); else RT_LAUNCH64(sdv_k_pcm16_lines, grid, a, s);
    return SDV_OK;
}
