/*
 * pcm16_frames_engine.inc - host side of sdv_pcm16x0_binarize_frames (include/sdvpcm.h): the PCM-16x0 branch of
 * VideoToDigital::doBinarize for a batch of whole frames.  Scheduling as for PCM-1 (pcm1_frames_engine.inc): prescan of all frames,
 * incoming states predicted from the stream's state and the prescan results, all frames decoded, then the frames behind broken links
 * repaired round by round until every link holds.
 */
extern "C" int sdv_pcm16x0_binarize_frames(sdv_engine *e, const uint8_t *luma, size_t row_stride, size_t frame_stride, int width, int height,
                                           int n_frames, uint32_t first_frame_no, unsigned flags, sdv_pcm16x0_bin_rec *out_lines, size_t lines_cap,
                                           sdv_frame_stats *out_stats, size_t stats_cap, void *stream)
{
    if (!e) return SDV_ERR_BAD_ARG;
    FrameFlagsConsumed flags_consumed(e);
    if (!luma) { set_error(e, "null video"); return SDV_ERR_NULL_VIDEO; }
    if (!out_lines || !out_stats) { set_error(e, "null output"); return SDV_ERR_NULL_PCM; }
    if (n_frames <= 0 || height < 2 || height > SDV_MAX_HEIGHT || width <= 0 || width > SDV_PX_BYTES || row_stride < (size_t)width) {
        set_error(e, "bad frame geometry"); return SDV_ERR_BAD_ARG;
    }
    if (width < sdvp16::P16_BITS) { set_error(e, "line shorter than the 193 bit cells of a PCM-16x0 line"); return SDV_ERR_SHORT_LINE; }
    if (n_frames > 1 && frame_stride < (size_t)(height - 1) * row_stride + (size_t)width) { set_error(e, "frame_stride smaller than one frame"); return SDV_ERR_BAD_ARG; }
    {
        const size_t need_lines = sdv_pcm16x0_binarize_records(height, n_frames, flags), need_stats = (size_t)n_frames + ((flags & SDV_FLAG_END_FILE) ? 1 : 0);
        if (lines_cap < need_lines || stats_cap < need_stats) {
            set_error(e, "output buffers too small: " + std::to_string(need_lines) + " sub-line records and " + std::to_string(need_stats) + " frame descriptors are needed");
            return SDV_ERR_BAD_ARG;
        }
    }
    rt::stream_t s = (rt::stream_t)stream;
    SDV_ON_DEVICE(e);
    const int n_real = n_frames;
    if (flags & SDV_FLAG_END_FILE) n_frames++;
    const int n = n_frames;
    int rc = ensure_capacity(e, (size_t)n, (size_t)height * 3);          /* coordinate lists: three sub-lines per line */
    if (rc != SDV_OK) return rc;
    RT_CHECK(rt::reserve_all((size_t)n, (size_t)n, e->d_states16_in, e->d_states16_out));
    const size_t prescan_bytes = 2 * sdvp16f::COORD_CHECK_LINES * sizeof(sdvp1f::PrescanRes) + sizeof(uint2);     /* per frame: two variants of every prescan line (pcm1_frames_device.h, PrescanRes), a median */
    RT_CHECK(e->d_prescan16.reserve((size_t)n * prescan_bytes));

    sdvp16f::FrameArgs16 a;
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
    a.states_in = e->d_states16_in; a.states_out = e->d_states16_out;
    a.recs16 = out_lines; a.prescan = (sdvp1f::PrescanRes *)e->d_prescan16.p;
    a.frame_med = (uint2 *)(a.prescan + e->d_prescan16.cap / prescan_bytes * 2 * sdvp16f::COORD_CHECK_LINES);    /* behind the prescan results of all the frames the buffer has room for */

    memset(&e->info, 0, sizeof(e->info));
    e->info.frames = (uint32_t)n;
    RT_CHECK(rt::h2d(e->d_states16_in, &e->chain16, sizeof(sdvp16f::State16), s));
#ifndef SDV_EMU
    if (e->profiling) {
        if (!e->have_events) { RT_CHECK(hipEventCreate(&e->ev0)); RT_CHECK(hipEventCreate(&e->ev1)); e->have_events = true; }
        RT_CHECK(hipEventRecord(e->ev0, s));
    }
#endif
    a.f.frame_list = NULL; a.f.frame_lo = 0; a.f.frame_hi = n;
    const bool insane = e->mode == SDV_MODE_INSANE;         /* its own build of the two kernels (pcm1_bin_device.h, process_line_p1) */
    if (insane) RT_LAUNCH64(sdv_k_pcm16_prescan_insane, (size_t)n * sdvp16f::COORD_CHECK_LINES, a, s); else RT_LAUNCH64(sdv_k_pcm16_prescan, (size_t)n * sdvp16f::COORD_CHECK_LINES, a, s);
    /* predicted incoming states.  This format has no Header lines: the first line of a field is always marked bad and the worker falls
     * back on its coordinate history behind it, so a stream keeps the coordinates it carries (the sticky model, predict_state16) */
    sdvp16f::PredictArgs16 pa; pa.states = e->d_states16_in; pa.prescan = a.prescan; pa.first = 0; pa.hi = n; pa.f = a.f;
#ifndef SDV_EMU
    if (n > 1) { hipLaunchKernelGGL(sdv_k_pcm16_predict, dim3((unsigned)((n - 1 + 255) / 256)), dim3(256), 0, s, pa); RT_CHECK(hipGetLastError()); }
#else
    for (int k = 1; k < n; k++) pa.states[k] = sdvp16f::predict_state16(pa, k, 0, true);
#endif
    std::vector<uint8_t> flag((size_t)n), predicted_again((size_t)n, 0);
    std::vector<int> list, head_of;
    /* first the lean build of the frame kernel (a tape that plays needs nothing else); the frames it gives up - a part that does not read from what it
     * inherits, frames without pixels - go to the full build, from the same states */
    RT_LAUNCH64(sdv_k_pcm16_frames_lean, n, a, s);
    e->info.rounds = 1; e->info.frames_launched = (uint32_t)n;
    {
        RT_CHECK(rt::d2h(flag.data(), e->d_flag, (size_t)n, s));
        std::vector<int> given_up;
        for (int k = 0; k < n; k++) if (flag[(size_t)k] == sdv::VF_ABORTED) given_up.push_back(k);
        if (!given_up.empty()) {
            RT_CHECK(rt::h2d(e->d_list_full, given_up.data(), given_up.size() * sizeof(int), s));
            a.f.frame_list = e->d_list_full;
            if (insane) RT_LAUNCH64(sdv_k_pcm16_frames_bin_insane, given_up.size(), a, s); else RT_LAUNCH64(sdv_k_pcm16_frames_bin, given_up.size(), a, s);
            a.f.frame_list = NULL;
            e->info.frames_launched += (uint32_t)given_up.size(); e->info.frames_general += (uint32_t)given_up.size();
#ifndef SDV_EMU
            RT_CHECK(rt::ssync(s));         /* (the list's source is this block's vector) */
#endif
        }
    }
    for (unsigned iter = 0; ; iter++) {
        if (iter > (unsigned)n + 2u) { set_error(e, "chain speculation did not settle"); return SDV_ERR_HIP; }
        RT_CHECK(rt::d2h(flag.data(), e->d_flag, (size_t)n, s));
        /* runs of broken links (see pcm1_frames_engine.inc): heads first in the list, then the frames further into the runs */
        list.clear(); head_of.clear();
        std::vector<int> others, others_head;
        std::vector<uint8_t> sticky;
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
            sdvp16f::State16 so, si;
            RT_CHECK(rt::d2h(&so, &e->d_states16_out[k], sizeof(so), s)); RT_CHECK(rt::d2h(&si, &e->d_states16_in[k + 1], sizeof(si), s));
            fprintf(stderr, "[sched16] round %u: %zu heads + %zu others; link %d -> %d:", iter, list.size(), others.size(), k, k + 1);
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
        sdvp16f::RepairArgs16 ra; ra.p = pa; ra.states_out = e->d_states16_out; ra.list = e->d_list_full; ra.head = e->d_first_of; ra.sticky = e->d_sticky16; ra.n = (int)list.size(); ra.frame_med = a.frame_med;
#ifndef SDV_EMU
        hipLaunchKernelGGL(sdv_k_pcm16_repair, dim3((unsigned)((n_heads + 255) / 256)), dim3(256), 0, s, ra, 0, n_heads); RT_CHECK(hipGetLastError());
        if (ra.n > n_heads) { hipLaunchKernelGGL(sdv_k_pcm16_repair, dim3((unsigned)((ra.n - n_heads + 255) / 256)), dim3(256), 0, s, ra, n_heads, ra.n); RT_CHECK(hipGetLastError()); }
#else
        for (int i = 0; i < ra.n; i++) sdvp16f::repair_body16(ra, i);
#endif
        a.f.frame_list = e->d_list_full;
        if (insane) RT_LAUNCH64(sdv_k_pcm16_frames_bin_insane, list.size(), a, s); else RT_LAUNCH64(sdv_k_pcm16_frames_bin, list.size(), a, s);
        a.f.frame_list = NULL;
        {
            sdvp16f::VerifyArgs16 va; va.f = a.f; va.states_in = e->d_states16_in; va.states_out = e->d_states16_out;
#ifndef SDV_EMU
            hipLaunchKernelGGL(sdv_k_pcm16_verify, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, va); RT_CHECK(hipGetLastError());
#else
            for (int k = 0; k + 1 < n; k++) sdvp16f::verify_body16(va, k);
#endif
        }
        e->info.rounds++; e->info.frames_launched += (uint32_t)list.size();
    }
#ifndef SDV_EMU
    if (e->profiling) {
        float ms = 0.f;
        RT_CHECK(hipEventRecord(e->ev1, s)); RT_CHECK(hipEventSynchronize(e->ev1));
        RT_CHECK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
        e->info.kernel_ms = ms;
    }
#endif
    RT_CHECK(rt::d2h(&e->chain16, &e->d_states16_out[n - 1], sizeof(sdvp16f::State16), s));
    return SDV_OK;
}

/* ---- PCM-16x0 front half, line by line: Binarizer::processLine with a PCM16X0SubLine output, the three passes of n_lines video lines per launch (pcm16_bin_device.h) ---- */
extern "C" int sdv_pcm16x0_binarize_lines(sdv_engine *e, const uint8_t *luma, size_t row_stride, int width, size_t n_lines,
                                          const sdv_bin_state *presets, uint32_t frame_number, uint16_t first_line, uint16_t line_step,
                                          unsigned flags, int coord_search, sdv_pcm16x0_bin_rec *out_lines, size_t lines_cap, uint8_t *out_scan_done, void *stream)
{
    if (!e) return SDV_ERR_BAD_ARG;
    if (!luma) { set_error(e, "null video"); return SDV_ERR_NULL_VIDEO; }
    if (!out_lines) { set_error(e, "null output"); return SDV_ERR_NULL_PCM; }
    if (width <= 0 || width > SDV_PX_BYTES || row_stride < (size_t)width) { set_error(e, "bad line geometry"); return SDV_ERR_BAD_ARG; }
    if (width < sdvp16::P16_BITS) { set_error(e, "line shorter than the 193 bit cells of a PCM-16x0 line"); return SDV_ERR_SHORT_LINE; }
    if (n_lines == 0) return SDV_OK;
    if (lines_cap / 3 < n_lines) { set_error(e, "output buffer too small: " + std::to_string(3 * n_lines) + " sub-line records are needed"); return SDV_ERR_BAD_ARG; }
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
