/*
 * markerless_frames_engine.inc - the host side of the two marker-less frame drivers, sdv_pcm1_binarize_frames and sdv_pcm16x0_binarize_frames
 * (include/sdvpcm.h): the PCM-1 / PCM-16x0 branch of VideoToDigital::doBinarize for a batch of whole frames.  One scheduler, written on what
 * differs between the formats (Fmt: pcm1_frames_engine.inc, pcm16_frames_engine.inc, which include this file ahead of themselves).
 *
 * Scheduling (the chain speculation of engine.inc in its plain form): the prescan of every frame is a pure function of its pixels
 * and runs first, for all frames at once; the incoming states of the frames are predicted from the stream's state and the prescan
 * results (markerless_chain_device.h, predict_state); all frames are decoded; every frame has checked the link to its successor itself.
 * Then, round by round, the frame behind every broken link is given what its predecessor really handed on and is decoded again,
 * until every link holds: frame 0 starts from the true state, so after round r the first r frames are final, and the loop ends with
 * every frame decoded from exactly its predecessor's final state - the sequential result.  A tape that plays: one round.
 *
 * Fmt: the record, state and argument types, the refusals' wording, where the engine keeps the stream's state and the per-frame buffers, the kernels.
 */
#pragma once
#include "markerless_chain_device.h"

/* one of the model's kernels over the indices [lo, hi), a thread each (markerless_chain_device.h, SDV_CHAIN_KERNEL: under the emulator such a kernel is
 * the loop over its range, so item i is its range [i, i + 1)) */
template <class K, class A> static inline rt::status_t launch_chain_range(K kernel, const A &a, int lo, int hi, rt::stream_t s)
{
    return RT_LAUNCH_ITEMS(kernel, ([&](const A &x, int i) { kernel(x, i, i + 1); }), lo, hi - lo, 256, s, a, lo, hi);
}

/* the argument checks of sdv_pcm1_binarize_lines and sdv_pcm16x0_binarize_lines (the line-by-line front halves); *todo: there are lines to decode */
template <class Fmt>
static int check_lines_call(sdv_engine *e, const uint8_t *luma, size_t row_stride, int width, size_t n_lines, const void *out_lines, size_t lines_cap, bool *todo)
{
    *todo = false;
    if (!e) return SDV_ERR_BAD_ARG;
    if (!luma) { set_error(e, "null video"); return SDV_ERR_NULL_VIDEO; }
    if (!out_lines) { set_error(e, "null output"); return SDV_ERR_NULL_PCM; }
    if (width <= 0 || width > SDV_PX_BYTES || row_stride < (size_t)width) { set_error(e, "bad line geometry"); return SDV_ERR_BAD_ARG; }
    if (width < Fmt::MIN_WIDTH) { set_error(e, Fmt::short_line()); return SDV_ERR_SHORT_LINE; }
    if (n_lines == 0) return SDV_OK;
    if (lines_cap / Fmt::LINES_PER_ROW < n_lines) { set_error(e, "output buffer too small: " + std::to_string(Fmt::LINES_PER_ROW * n_lines) + " " + Fmt::rec_noun() + " are needed"); return SDV_ERR_BAD_ARG; }
    *todo = true;
    return SDV_OK;
}

template <class Fmt>
static int markerless_binarize_frames(sdv_engine *e, const uint8_t *luma, size_t row_stride, size_t frame_stride, int width, int height,
                                      int n_frames, uint32_t first_frame_no, unsigned flags, typename Fmt::Rec *out_lines, size_t lines_cap,
                                      sdv_frame_stats *out_stats, size_t stats_cap, void *stream)
{
    typedef typename Fmt::State State;
    using sdvmf::COORD_CHECK_LINES;
    using sdvmf::PrescanRes;
    if (!e) return SDV_ERR_BAD_ARG;
    FrameFlagsConsumed flags_consumed(e);
    int rc = check_frame_call(e, luma, out_lines, out_stats, row_stride, frame_stride, width, height, n_frames, flags, lines_cap, stats_cap,
                              SDV_PX_BYTES, Fmt::MIN_WIDTH, Fmt::short_line(), Fmt::records_needed(height, n_frames, flags), Fmt::rec_noun());
    if (rc != SDV_OK) return rc;
    rt::stream_t s = (rt::stream_t)stream;
    SDV_ON_DEVICE(e);
    const int n_real = n_frames;
    if (flags & SDV_FLAG_END_FILE) n_frames++;
    const int n = n_frames;
    rc = ensure_capacity(e, (size_t)n, (size_t)height * Fmt::LINES_PER_ROW);
    if (rc != SDV_OK) return rc;
    RT_CHECK(Fmt::reserve_states(e, (size_t)n));
    rt::DevBuf<uint8_t> &prescan_buf = Fmt::prescan_buf(e);
    const size_t prescan_bytes = 2 * COORD_CHECK_LINES * sizeof(PrescanRes) + sizeof(uint2);      /* per frame: two variants of every prescan line (pcm1_frames_device.h, PrescanRes), a median */
    RT_CHECK(prescan_buf.reserve((size_t)n * prescan_bytes));
    State *const d_in = Fmt::states_in(e), *const d_out = Fmt::states_out(e);

    typename Fmt::Args a;
    memset(&a, 0, sizeof(a));
    a.f.luma = luma; a.f.frame_stride = frame_stride; a.f.row_stride = row_stride; a.f.width = width; a.f.height = height;
    a.f.first_frame_no = first_frame_no;
    a.f.new_file_frame = (flags & SDV_FLAG_NEW_FILE) ? 0 : -1;
    a.f.end_file_frame = (flags & SDV_FLAG_END_FILE) ? n_real : -1;
    a.f.doubled = (flags & SDV_FLAG_DOUBLED) ? 1 : 0;
    a.f.mode = (uint8_t)e->mode; a.f.check_line_copy = (uint8_t)e->check_line_dup; a.f.coordinate_damper = (uint8_t)e->coordinate_damper;
    a.f.preset = e->preset;
    a.f.stats = out_stats; a.f.scratch = e->d_scratch; a.f.flag = e->d_flag; a.f.n_total = n;
    rc = take_frame_flags(e, (size_t)n, s, &a.f.frame_flags); if (rc != SDV_OK) return rc;
    Fmt::bind(a, d_in, d_out, out_lines);
    a.prescan = (PrescanRes *)prescan_buf.p;
    a.frame_med = (uint2 *)(a.prescan + prescan_buf.cap / prescan_bytes * 2 * COORD_CHECK_LINES);       /* behind the prescan results of all the frames the buffer has room for */

    memset(&e->info, 0, sizeof(e->info));
    e->info.frames = (uint32_t)n;
    RT_CHECK(rt::h2d(d_in, &Fmt::chain(e), sizeof(State), s));
    if (e->profiling) RT_CHECK(e->timer.start(s));
    /* the prescan lines of every frame */
    a.f.frame_list = NULL; a.f.frame_lo = 0; a.f.frame_hi = n;
    const bool insane = e->mode == SDV_MODE_INSANE;         /* its own build of the two kernels (pcm1_bin_device.h, process_line_p1) */
    if (insane) RT_LAUNCH64(Fmt::k_prescan_insane, (size_t)n * COORD_CHECK_LINES, a, s); else RT_LAUNCH64(Fmt::k_prescan, (size_t)n * COORD_CHECK_LINES, a, s);
    /* predicted incoming states, then all frames */
    sdvml::PredictArgs<State> pa; pa.states = d_in; pa.prescan = a.prescan; pa.f = a.f;
    RT_CHECK(launch_chain_range(Fmt::k_predict, pa, 1, n, s));
    /* first the lean build of the frame kernel (a tape that plays needs nothing else); the frames it gives up - a line (PCM-16x0: a part) that does
     * not read from what it inherits, frames without pixels - go to the full build, from the same states */
    RT_LAUNCH64(Fmt::k_lean, n, a, s);
    e->info.rounds = 1; e->info.frames_launched = (uint32_t)n;

    std::vector<uint8_t> flag((size_t)n);
    {
        RT_CHECK(rt::d2h(flag.data(), e->d_flag, (size_t)n, s));
        std::vector<int> given_up;
        for (int k = 0; k < n; k++) if (flag[(size_t)k] == sdv::VF_ABORTED) given_up.push_back(k);
        if (!given_up.empty()) {
            RT_CHECK(rt::h2d(e->d_list_full, given_up.data(), given_up.size() * sizeof(int), s));
            a.f.frame_list = e->d_list_full;
            if (insane) RT_LAUNCH64(Fmt::k_bin_insane, given_up.size(), a, s); else RT_LAUNCH64(Fmt::k_bin, given_up.size(), a, s);
            a.f.frame_list = NULL;
            e->info.frames_launched += (uint32_t)given_up.size(); e->info.frames_general += (uint32_t)given_up.size();
            RT_CHECK(rt::ssync(s));         /* (the list's source is this block's vector) */
        }
    }
    std::vector<int> list, head_of, others, others_head;
    std::vector<uint8_t> sticky, predicted_again((size_t)n, 0);      /* frames the model has had its second say on */
    for (unsigned iter = 0; ; iter++) {
        if (iter > (unsigned)n + 2u) { set_error(e, "chain speculation did not settle"); return SDV_ERR_HIP; }
        RT_CHECK(rt::d2h(flag.data(), e->d_flag, (size_t)n, s));
        /* runs of broken links: the frame behind the first link of a run (its head) takes its predecessor's real outcome; the frames further
         * into the run were started from descendants of a state now known to be wrong - they are predicted again from the run's head, once,
         * and where the model has nothing new to say (or has had its say) they take their own predecessor's outcome: on a tape the
         * model cannot follow (jitter, dropouts in DRAFT mode) the rounds then do not grow with the number of frames, because what a
         * frame hands on depends little on what it was handed (markerless_chain_device.h, repair_body).  Heads first in the list (a head
         * is its own head_of), then the frames further into the runs */
        list.clear(); head_of.clear(); others.clear(); others_head.clear();
        int cur_head = -1;
        for (int k = 0; k + 1 < n; k++) {
            const bool broken = flag[(size_t)k] == sdv::VF_BREAK;
            if (iter == 0) {
                /* first repair: what the frames up to the first broken link handed on is final; every frame behind it was started from
                 * a premise that is now known to be wrong, even where its own links hold (a chain of wrong states can be consistent in
                 * itself) - all of them are predicted again from the first repaired frame, with the coordinates the stream really
                 * carries (the sticky model) */
                if (cur_head < 0) { if (broken) { cur_head = k + 1; list.push_back(k + 1); head_of.push_back(k + 1); } }
                else { others.push_back(k + 1); others_head.push_back(cur_head); predicted_again[(size_t)k + 1] = 1; }
                continue;
            }
            if (!broken) { cur_head = -1; continue; }
            if (cur_head < 0) { cur_head = k + 1; list.push_back(k + 1); head_of.push_back(k + 1); }
            else if (e->mode == SDV_MODE_DRAFT && predicted_again[(size_t)k + 1]) { list.push_back(k + 1); head_of.push_back(k + 1); }      /* DRAFT: Jacobi step */
            else { others.push_back(k + 1); others_head.push_back(cur_head); if (predicted_again[(size_t)k + 1] < 2) predicted_again[(size_t)k + 1]++; }
        }
        if (list.empty()) break;
        if (dev_env("SDV_SCHED_TRACE")) {        /* developer aid: the first broken link, what was handed on and what the successor was started from */
            const int k = list[0] - 1;
            State so, si;
            RT_CHECK(rt::d2h(&so, &d_out[k], sizeof(so), s)); RT_CHECK(rt::d2h(&si, &d_in[k + 1], sizeof(si), s));
            fprintf(stderr, "[%s] round %u: %zu heads + %zu others; link %d -> %d:", Fmt::TRACE_TAG, iter, list.size(), others.size(), k, k + 1);
            const uint8_t *x = (const uint8_t *)&so, *y = (const uint8_t *)&si;
            for (size_t i = 0; i < sizeof(so); i++) if (x[i] != y[i]) fprintf(stderr, " [%zu] %u != %u", i, x[i], y[i]);
            fprintf(stderr, "\n");
        }
        const int n_heads = (int)list.size();
        list.insert(list.end(), others.begin(), others.end());
        head_of.insert(head_of.end(), others_head.begin(), others_head.end());
        sticky.assign(list.size(), 0);
        for (size_t i = (size_t)n_heads; i < list.size(); i++) sticky[i] = predicted_again[(size_t)list[i]] == 1;       /* the model has its say once */
        RT_CHECK(e->d_sticky16.reserve(list.size(), (size_t)n));
        RT_CHECK(rt::h2d(e->d_sticky16, sticky.data(), sticky.size(), s));
        RT_CHECK(rt::h2d(e->d_list_full, list.data(), list.size() * sizeof(int), s));
        RT_CHECK(rt::h2d(e->d_first_of, head_of.data(), head_of.size() * sizeof(int), s));
        /* the heads in a launch of their own, ahead of the others, which read the states the heads were given.  (A head's link is not marked as
         * holding here, as sdv_k_anchor would: this round's verify launch writes the flag of every link.) */
        sdvml::RepairArgs<State> ra; ra.p = pa; ra.states_out = d_out; ra.list = e->d_list_full; ra.head = e->d_first_of; ra.sticky = e->d_sticky16; ra.frame_med = a.frame_med;
        RT_CHECK(launch_chain_range(Fmt::k_repair, ra, 0, n_heads, s));
        RT_CHECK(launch_chain_range(Fmt::k_repair, ra, n_heads, (int)list.size(), s));
        a.f.frame_list = e->d_list_full;
        if (insane) RT_LAUNCH64(Fmt::k_bin_insane, list.size(), a, s); else RT_LAUNCH64(Fmt::k_bin, list.size(), a, s);
        a.f.frame_list = NULL;
        {   /* the frames that were not decoded again have not looked at their links again: all links, once */
            sdvml::VerifyArgs<State> va; va.f = a.f; va.states_in = d_in; va.states_out = d_out;
            RT_CHECK(launch_chain_range(Fmt::k_verify, va, 0, n - 1, s));
        }
        e->info.rounds++; e->info.frames_launched += (uint32_t)list.size();
    }
    if (e->profiling) {
        RT_CHECK(e->timer.stop(s));
        RT_CHECK(e->timer.elapsed_ms(&e->info.kernel_ms));      /* (once per call) */
    }
    RT_CHECK(rt::d2h(&Fmt::chain(e), &d_out[n - 1], sizeof(State), s));
    return SDV_OK;
}
