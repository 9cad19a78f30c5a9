/*
 * pcm_condition_engine.inc - host side of sdv_pcm_preemphasis and sdv_pcm_resample (include/sdvpcm.h): what a 44 100 Hz WAV file needs ahead of
 * the encoders - the 15/50 us pre-emphasis network (pcm_preemph_device.h) and the 1000 / 1001 resampler to 44 056 Hz (pcm_resample_device.h),
 * both on interleaved int16 PCM.  Included at the end of engine.inc, so by the one translation unit of either build.  Each call is one launch
 * and reads nothing back: the pre-emphasis keeps its state and its counter of clipped words on the device, the resampler keeps its counters on
 * the host - the number of outputs follows from the number of pairs alone - and its last 127 pairs on the device.  (The buffer checks, the tap row and
 * the table upload: stage_common.inc.)
 */

struct sdv_pcm_cond {
    /* sdv_pcm_preemphasis: pe_idle - the state on the device is not looked at, the next call starts the filter; pe_zero - nor is the counter, the next
     * call clears it first */
    bool pe_idle = true, pe_zero = true;
    rt::DevBuf<sdvc::PeState> d_pe_state, d_pe_state_spare;
    rt::DevBuf<unsigned long long> d_pe_clipped;
    /* sdv_pcm_resample: pairs the open stream has seen, outputs it has emitted; its last PR_HIST pairs; the tap table ([k][phase]) here and there */
    uint64_t rs_seen = 0, rs_emitted = 0;
    rt::DevBuf<uint32_t> d_rs_hist, d_rs_hist_spare;
    std::vector<double> rs_table; rt::DevBuf<double> d_rs_taps; bool rs_taps_ready = false;
};

static void pcm_cond_free(sdv_engine *e) { delete e->cond; e->cond = NULL; }
static sdv_pcm_cond *pcm_cond_get(sdv_engine *e) { if (!e->cond) e->cond = new sdv_pcm_cond(); return e->cond; }

/* outputs m of a stream whose x[i0], i0 = m + floor(m / 1000), lies in front of position j: i0 takes every value but 1000, 2001, 3002, ... */
static uint64_t pcm_rs_outputs_before(uint64_t j) { return j - j / SDV_PCM_RESAMPLE_M; }

extern "C" {

/* ---- pre-emphasis ------------------------------------------------------------------------------------------------------------------------ */
void sdv_preemphasis_coeffs(uint16_t sample_rate, double c[3])
{
    double d[3];
    sdv_deemphasis_coeffs(sample_rate, d);
    c[0] = 1.0 / d[0]; c[1] = d[2] / d[0]; c[2] = d[1] / d[0];
}

int sdv_reset_preemphasis(sdv_engine *e)
{
    if (!e) return SDV_ERR_BAD_ARG;
    if (e->cond) { e->cond->pe_idle = true; e->cond->pe_zero = true; }
    return SDV_OK;
}

int sdv_pcm_preemphasis(sdv_engine *e, const int16_t *pcm, size_t n_pairs, uint16_t sample_rate, int16_t *out_pcm, void *stream)
{
    if (!e) return SDV_ERR_BAD_ARG;
    if (n_pairs == 0) return SDV_OK;
    if (!pcm) { set_error(e, "null pcm buffer"); return SDV_ERR_NULL_LINES; }
    if (!out_pcm) { set_error(e, "null output buffer"); return SDV_ERR_NULL_BLOCK; }
    if (n_pairs >= STAGE_MAX_PAIRS) { set_error(e, "too many sample pairs in one call"); return SDV_ERR_BAD_ARG; }
    const int rc = stage_check_pcm(e, pcm, n_pairs, out_pcm, n_pairs);
    if (rc != SDV_OK) return rc;
    SDV_ON_DEVICE(e);
    sdv_pcm_cond *t = pcm_cond_get(e);
    const rt::stream_t s = (rt::stream_t)stream;
    RT_CHECK(rt::reserve_all(1, 1, t->d_pe_state, t->d_pe_state_spare));
    RT_CHECK(t->d_pe_clipped.reserve(1));
    if (t->pe_zero) RT_CHECK(rt::dfill_bytes(t->d_pe_clipped, 0, sizeof(unsigned long long), s));
    t->pe_zero = false;
    sdvc::PeArgs a; memset(&a, 0, sizeof(a));
    a.in = (const uint32_t *)pcm; a.out = (uint32_t *)out_pcm; a.n = n_pairs;
    a.state_in = t->d_pe_state; a.state_out = t->d_pe_state_spare; a.clipped = t->d_pe_clipped;
    sdv_preemphasis_coeffs(sample_rate, a.c);
    a.key = sample_rate == 44056 ? sdvc::PE_KEY_44056 : sdvc::PE_KEY_44100;
    a.head_idle = t->pe_idle ? 1 : 0; a.vec_in = ((uintptr_t)pcm & 15u) == 0; a.vec_out = ((uintptr_t)out_pcm & 15u) == 0;
    RT_LAUNCH64(sdv_k_preemph, (n_pairs + sdvc::PE_TILE - 1) / sdvc::PE_TILE, a, s);
    t->d_pe_state.swap(t->d_pe_state_spare);
    t->pe_idle = false;
    return SDV_OK;
}

int sdv_pcm_preemphasis_clipped(sdv_engine *e, void *stream, uint64_t *count)
{
    if (!e || !count) return SDV_ERR_BAD_ARG;
    *count = 0;
    SDV_ON_DEVICE(e);
    const rt::stream_t s = (rt::stream_t)stream;
    sdv_pcm_cond *t = e->cond;
    if (!t || t->pe_zero) { RT_CHECK(rt::ssync(s)); return SDV_OK; }
    unsigned long long n = 0;
    RT_CHECK(rt::d2h(&n, t->d_pe_clipped, sizeof(n), s));
    *count = n;
    return SDV_OK;
}

/* ---- resampling 44 100 Hz -> 44 056 Hz ----------------------------------------------------------------------------------------------------- */
void sdv_pcm_resample_taps(int phase, double taps[128])
{
    if (phase < 0 || phase >= SDV_PCM_RESAMPLE_L) { for (int k = 0; k < 128; k++) taps[k] = 0.0; return; }
    kaiser_sinc_row((double)phase / (double)SDV_PCM_RESAMPLE_L, taps);
}

int sdv_reset_pcm_resample(sdv_engine *e)
{
    if (!e) return SDV_ERR_BAD_ARG;
    if (e->cond) { e->cond->rs_seen = 0; e->cond->rs_emitted = 0; }
    return SDV_OK;
}

size_t sdv_pcm_resample_pending(const sdv_engine *e)
{
    if (!e || !e->cond) return 0;
    return (size_t)(e->cond->rs_seen < (uint64_t)sdvc::PR_HALF ? e->cond->rs_seen : (uint64_t)sdvc::PR_HALF);
}

size_t sdv_pcm_resample_room(const sdv_engine *e, size_t n_pairs)
{
    /* what a flush behind the call's last pair would leave emitted, less what is emitted */
    const uint64_t seen = e && e->cond ? e->cond->rs_seen : 0, emitted = e && e->cond ? e->cond->rs_emitted : 0;
    return (size_t)(pcm_rs_outputs_before(seen + n_pairs) - emitted);
}

int sdv_pcm_resample(sdv_engine *e, const int16_t *pcm, size_t n_pairs, int flush, int16_t *out_pcm, size_t out_cap, size_t *n_out, void *stream)
{
    if (!e || !n_out) return SDV_ERR_BAD_ARG;
    *n_out = 0;
    if (n_pairs > 0 && !pcm) { set_error(e, "null pcm buffer"); return SDV_ERR_NULL_LINES; }
    if (n_pairs >= STAGE_MAX_PAIRS) { set_error(e, "too many sample pairs in one call"); return SDV_ERR_BAD_ARG; }
    const uint64_t seen0 = e->cond ? e->cond->rs_seen : 0, emitted0 = e->cond ? e->cond->rs_emitted : 0, seen1 = seen0 + n_pairs;
    if (seen1 == 0) return SDV_OK;                      /* nothing open, nothing new */
    /* without flush: the outputs whose x[i0 + 64] has been seen */
    const uint64_t emitted1 = flush ? pcm_rs_outputs_before(seen1) : seen1 > (uint64_t)sdvc::PR_HALF ? pcm_rs_outputs_before(seen1 - sdvc::PR_HALF) : 0;
    const uint64_t count = emitted1 - emitted0;
    if (n_pairs > 0 && !out_pcm) { set_error(e, "null output buffer"); return SDV_ERR_NULL_BLOCK; }
    const size_t room = sdv_pcm_resample_room(e, n_pairs);
    if (out_cap < room) {
        set_error(e, "output buffer too small: room for " + std::to_string((unsigned long long)room) + " sample pairs is needed (sdv_pcm_resample_room)");
        return SDV_ERR_BAD_ARG;
    }
    if (count > 0 && !out_pcm) { set_error(e, "null output buffer"); return SDV_ERR_NULL_BLOCK; }
    const int rc = stage_check_pcm(e, pcm, n_pairs, out_pcm, out_pcm ? out_cap : 0);
    if (rc != SDV_OK) return rc;
    SDV_ON_DEVICE(e);
    sdv_pcm_cond *t = pcm_cond_get(e);
    const rt::stream_t s = (rt::stream_t)stream;
    const int rc_taps = stage_upload_taps(e, sdv_pcm_resample_taps, 0, SDV_PCM_RESAMPLE_L, sdvc::PR_PITCH, t->rs_table, t->d_rs_taps, t->rs_taps_ready, s);
    if (rc_taps != SDV_OK) return rc_taps;
    RT_CHECK(rt::reserve_all(sdvc::PR_HIST, sdvc::PR_HIST, t->d_rs_hist, t->d_rs_hist_spare));
    sdvc::PrArgs a; memset(&a, 0, sizeof(a));
    a.in = (const uint32_t *)pcm; a.out = (uint32_t *)out_pcm; a.hist = t->d_rs_hist; a.hist_out = t->d_rs_hist_spare; a.taps = t->d_rs_taps;
    a.seen0 = seen0; a.seen1 = seen1; a.m_lo = emitted0; a.m_hi = emitted1;
    const uint64_t tile0 = emitted0 / sdvc::PR_TILE, n_tiles = count ? (emitted1 - 1) / sdvc::PR_TILE - tile0 + 1 : 0;
    a.row0 = tile0 * sdvc::PR_G; a.n_blocks = (uint32_t)(n_tiles * sdvc::PR_QUARTERS); a.keep_hist = flush ? 0 : 1;
    RT_LAUNCH64(sdv_k_pcmrs, (size_t)a.n_blocks + (flush ? 0 : 1), a, s);
    if (flush) { t->rs_seen = 0; t->rs_emitted = 0; }
    else { t->d_rs_hist.swap(t->d_rs_hist_spare); t->rs_seen = seen1; t->rs_emitted = emitted1; }
    *n_out = (size_t)count;
    return SDV_OK;
}

} /* extern "C" */
