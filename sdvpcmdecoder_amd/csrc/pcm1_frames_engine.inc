/*
 * pcm1_frames_engine.inc - host side of sdv_pcm1_binarize_frames (include/sdvpcm.h): the PCM-1 branch of
 * VideoToDigital::doBinarize for a batch of whole frames.  Included after pcm1_engine.inc by the same two translation units.
 *
 * Scheduling (the chain speculation of engine.inc in its plain form): the prescan of every frame is a pure function of its pixels
 * and runs first, for all frames at once; the incoming states of the frames are predicted from the stream's state and the prescan
 * results (pcm1_frames_device.h, predict_body1); all frames are decoded; every frame has checked the link to its successor itself.
 * Then, round by round, the frame behind every broken link is given what its predecessor really handed on and is decoded again,
 * until every link holds: frame 0 starts from the true state, so after round r the first r frames are final, and the loop ends with
 * every frame decoded from exactly its predecessor's final state - the sequential result.  A tape that plays: one round.
 */
extern "C" int sdv_pcm1_binarize_frames(sdv_engine *e, const uint8_t *luma, size_t row_stride, size_t frame_stride, int width, int height,
                                        int n_frames, uint32_t first_frame_no, unsigned flags, sdv_pcm1_bin_rec *out_lines, size_t lines_cap,
                                        sdv_frame_stats *out_stats, size_t stats_cap, void *stream)
{
    if (!e) return SDV_ERR_BAD_ARG;
    FrameFlagsConsumed flags_consumed(e);
    if (!luma) { set_error(e, "null video"); return SDV_ERR_NULL_VIDEO; }
    if (!out_lines || !out_stats) { set_error(e, "null output"); return SDV_ERR_NULL_PCM; }
    if (n_frames <= 0 || height < 2 || height > SDV_MAX_HEIGHT || width <= 0 || width > SDV_PX_BYTES || row_stride < (size_t)width) {
        set_error(e, "bad frame geometry"); return SDV_ERR_BAD_ARG;
    }
    if (width < sdvp1b::P1_BITS) { set_error(e, "line shorter than the 94 bit cells of a PCM-1 line"); return SDV_ERR_SHORT_LINE; }
    if (n_frames > 1 && frame_stride < (size_t)(height - 1) * row_stride + (size_t)width) { set_error(e, "frame_stride smaller than one frame"); return SDV_ERR_BAD_ARG; }
    {
        const size_t need_lines = sdv_binarize_records(height, n_frames, flags), need_stats = (size_t)n_frames + ((flags & SDV_FLAG_END_FILE) ? 1 : 0);
        if (lines_cap < need_lines || stats_cap < need_stats) {
            set_error(e, "output buffers too small: " + std::to_string(need_lines) + " line records and " + std::to_string(need_stats) + " frame descriptors are needed");
            return SDV_ERR_BAD_ARG;
        }
    }
    rt::stream_t s = (rt::stream_t)stream;
    SDV_ON_DEVICE(e);
    const int n_real = n_frames;
    if (flags & SDV_FLAG_END_FILE) n_frames++;
    const int n = n_frames;
    int rc = ensure_capacity(e, (size_t)n, (size_t)height);
    if (rc != SDV_OK) return rc;
    sdv_pcm1_stitcher *t = pcm1_get(e);
    const size_t prescan_bytes = 2 * sdvp1f::COORD_CHECK_LINES * sizeof(sdvp1f::PrescanRes) + sizeof(uint2);      /* per frame: two variants of every prescan line (pcm1_frames_device.h, PrescanRes), a median */
    RT_CHECK(t->d_prescan.reserve((size_t)n * prescan_bytes));

    sdvp1f::FrameArgs1 a;
    memset(&a, 0, sizeof(a));
    a.f.luma = luma; a.f.frame_stride = frame_stride; a.f.row_stride = row_stride; a.f.width = width; a.f.height = height;
    a.f.first_frame_no = first_frame_no;
    a.f.new_file_frame = (flags & SDV_FLAG_NEW_FILE) ? 0 : -1;
    a.f.end_file_frame = (flags & SDV_FLAG_END_FILE) ? n_real : -1;
    a.f.doubled = (flags & SDV_FLAG_DOUBLED) ? 1 : 0;
    a.f.mode = (uint8_t)e->mode; a.f.check_line_copy = (uint8_t)e->check_line_dup; a.f.coordinate_damper = (uint8_t)e->coordinate_damper;
    a.f.preset = e->preset;
    a.f.states_in = e->d_states_in; a.f.states_out = e->d_states_out;
    a.f.stats = out_stats; a.f.scratch = e->d_scratch; a.f.flag = e->d_flag; a.f.n_total = n;
    rc = take_frame_flags(e, (size_t)n, s, &a.f.frame_flags); if (rc != SDV_OK) return rc;
    a.recs1 = out_lines; a.prescan = (sdvp1f::PrescanRes *)t->d_prescan.p;
    a.frame_med = (uint2 *)(a.prescan + t->d_prescan.cap / prescan_bytes * 2 * sdvp1f::COORD_CHECK_LINES);       /* behind the prescan results of all the frames the buffer has room for */

    memset(&e->info, 0, sizeof(e->info));
    e->info.frames = (uint32_t)n;
    RT_CHECK(rt::h2d(e->d_states_in, &e->chain, sizeof(sdv_v2d_state), s));
#ifndef SDV_EMU
    if (e->profiling) {
        if (!e->have_events) { RT_CHECK(hipEventCreate(&e->ev0)); RT_CHECK(hipEventCreate(&e->ev1)); e->have_events = true; }
        RT_CHECK(hipEventRecord(e->ev0, s));
    }
#endif
    /* the prescan lines of every frame */
    a.f.frame_list = NULL; a.f.frame_lo = 0; a.f.frame_hi = n;
    const bool insane = e->mode == SDV_MODE_INSANE;         /* its own build of the two kernels (pcm1_bin_device.h, process_line_p1) */
    if (insane) RT_LAUNCH64(sdv_k_pcm1_prescan_insane, (size_t)n * sdvp1f::COORD_CHECK_LINES, a, s); else RT_LAUNCH64(sdv_k_pcm1_prescan, (size_t)n * sdvp1f::COORD_CHECK_LINES, a, s);
    /* predicted incoming states, then all frames */
    {
        sdvp1f::PredictArgs1 pa; pa.states = e->d_states_in; pa.prescan = a.prescan; pa.first = 0; pa.hi = n; pa.first_of = NULL; pa.f = a.f;
#ifndef SDV_EMU
        if (n > 1) { hipLaunchKernelGGL(sdv_k_pcm1_predict, dim3((unsigned)((n - 1 + 255) / 256)), dim3(256), 0, s, pa); RT_CHECK(hipGetLastError()); }
#else
        for (int k = 1; k < n; k++) sdvp1f::predict_body1(pa, k);
#endif
    }
    /* first the lean build of the frame kernel (a tape that plays needs nothing else); the frames it gives up - a line that does not read from what
     * it inherits, frames without pixels - go to the full build, from the same states */
    RT_LAUNCH64(sdv_k_pcm1_frames_lean, n, a, s);
    e->info.rounds = 1; e->info.frames_launched = (uint32_t)n;

    std::vector<uint8_t> flag((size_t)n);
    {
        RT_CHECK(rt::d2h(flag.data(), e->d_flag, (size_t)n, s));
        std::vector<int> given_up;
        for (int k = 0; k < n; k++) if (flag[(size_t)k] == sdv::VF_ABORTED) given_up.push_back(k);
        if (!given_up.empty()) {
            RT_CHECK(rt::h2d(e->d_list_full, given_up.data(), given_up.size() * sizeof(int), s));
            a.f.frame_list = e->d_list_full;
            if (insane) RT_LAUNCH64(sdv_k_pcm1_frames_bin_insane, given_up.size(), a, s); else RT_LAUNCH64(sdv_k_pcm1_frames_bin, given_up.size(), a, s);
            a.f.frame_list = NULL;
            e->info.frames_launched += (uint32_t)given_up.size(); e->info.frames_general += (uint32_t)given_up.size();
#ifndef SDV_EMU
            RT_CHECK(rt::ssync(s));         /* (the list's source is this block's vector) */
#endif
        }
    }
    std::vector<int> heads, others, head_of, redo;
    std::vector<uint8_t> predicted_again((size_t)n, 0);      /* frames the model has had its second say on */
    sdvp1f::PredictArgs1 pa; pa.states = e->d_states_in; pa.prescan = a.prescan; pa.first = 0; pa.hi = n; pa.first_of = NULL; pa.f = a.f;
    for (unsigned iter = 0; ; iter++) {
        if (iter > (unsigned)n + 2u) { set_error(e, "chain speculation did not settle"); return SDV_ERR_HIP; }
        RT_CHECK(rt::d2h(flag.data(), e->d_flag, (size_t)n, s));
        /* runs of broken links: the frame behind the first link of a run takes its predecessor's real outcome; the frames further into
         * the run were started from descendants of a state now known to be wrong - they are predicted again from the run's head, once,
         * and where the model has nothing new to say (or has had its say) they take their own predecessor's outcome: on a tape the
         * model cannot follow (jitter, dropouts in DRAFT mode) the rounds then do not grow with the number of frames, because what a
         * frame hands on depends little on what it was handed (pcm1_frames_device.h, repair_body1) */
        heads.clear(); others.clear(); head_of.clear();
        int cur_head = -1;
        for (int k = 0; k + 1 < n; k++) {
            const bool broken = flag[(size_t)k] == sdv::VF_BREAK;
            if (iter == 0) {
                /* first repair: what the frames up to the first broken link handed on is final; every frame behind it was started from
                 * a premise that is now known to be wrong, even where its own links hold (a chain of wrong states can be consistent in
                 * itself) - all of them are predicted again from the first repaired frame, with the coordinates the stream really
                 * carries (the sticky model) */
                if (cur_head < 0) { if (broken) { cur_head = k + 1; heads.push_back(k + 1); } }
                else { others.push_back(k + 1); head_of.push_back(cur_head); predicted_again[(size_t)k + 1] = 1; }
                continue;
            }
            if (!broken) { cur_head = -1; continue; }
            if (cur_head < 0) { cur_head = k + 1; heads.push_back(k + 1); }
            else if (e->mode == SDV_MODE_DRAFT && predicted_again[(size_t)k + 1]) heads.push_back(k + 1);       /* DRAFT: Jacobi step */
            else { others.push_back(k + 1); head_of.push_back(cur_head); if (predicted_again[(size_t)k + 1] < 2) predicted_again[(size_t)k + 1]++; }
        }
        if (heads.empty()) break;
        RT_CHECK(rt::h2d(e->d_anchors, heads.data(), heads.size() * sizeof(int), s));
        sdv::AnchorArgs aa; aa.states_in = e->d_states_in; aa.states_out = e->d_states_out; aa.list = e->d_anchors; aa.n = (int)heads.size(); aa.flag = e->d_flag;
        RT_CHECK(rt::launch_anchor(aa, s));
        if (!others.empty()) {
            RT_CHECK(rt::h2d(e->d_list_lean, others.data(), others.size() * sizeof(int), s));
            RT_CHECK(rt::h2d(e->d_first_of, head_of.data(), head_of.size() * sizeof(int), s));
            std::vector<uint8_t> sticky(others.size());
            for (size_t i = 0; i < others.size(); i++) sticky[i] = predicted_again[(size_t)others[i]] == 1;       /* the model has its say once */
            RT_CHECK(e->d_sticky16.reserve(others.size(), (size_t)n));
            RT_CHECK(rt::h2d(e->d_sticky16, sticky.data(), sticky.size(), s));
            sdvp1f::RepairArgs1 ra; ra.p = pa; ra.states_out = e->d_states_out; ra.list = e->d_list_lean; ra.head = e->d_first_of; ra.sticky = e->d_sticky16; ra.n = (int)others.size(); ra.frame_med = a.frame_med;
#ifndef SDV_EMU
            hipLaunchKernelGGL(sdv_k_pcm1_repair, dim3((unsigned)((ra.n + 255) / 256)), dim3(256), 0, s, ra); RT_CHECK(hipGetLastError());
#else
            for (int i = 0; i < ra.n; i++) sdvp1f::repair_body1(ra, i);
#endif
        }
        redo = heads; redo.insert(redo.end(), others.begin(), others.end());
        RT_CHECK(rt::h2d(e->d_list_full, redo.data(), redo.size() * sizeof(int), s));
        a.f.frame_list = e->d_list_full;
        if (insane) RT_LAUNCH64(sdv_k_pcm1_frames_bin_insane, redo.size(), a, s); else RT_LAUNCH64(sdv_k_pcm1_frames_bin, redo.size(), a, s);
        a.f.frame_list = NULL;
        {   /* the frames that were not decoded again have not looked at their links again: all links, once */
            sdvp1f::VerifyArgs1 va; va.f = a.f;
#ifndef SDV_EMU
            hipLaunchKernelGGL(sdv_k_pcm1_verify, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, va); RT_CHECK(hipGetLastError());
#else
            for (int k = 0; k + 1 < n; k++) sdvp1f::verify_body1(va, k);
#endif
        }
        e->info.rounds++; e->info.frames_launched += (uint32_t)redo.size();
    }
#ifndef SDV_EMU
    if (e->profiling) {
        float ms = 0.f;
        RT_CHECK(hipEventRecord(e->ev1, s)); RT_CHECK(hipEventSynchronize(e->ev1));
        RT_CHECK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
        e->info.kernel_ms = ms;
    }
#endif
    RT_CHECK(rt::d2h(&e->chain, &e->d_states_out[n - 1], sizeof(sdv_v2d_state), s));
    return SDV_OK;
}
