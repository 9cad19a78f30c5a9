/*
 * pcm1_frames_engine.inc - sdv_pcm1_binarize_frames (include/sdvpcm.h): what the scheduler of markerless_frames_engine.inc is told about PCM-1.
 * Included after pcm1_engine.inc by the same two translation units.
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
