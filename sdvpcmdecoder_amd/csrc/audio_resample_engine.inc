/*
 * audio_resample_engine.inc - host side of sdv_audio_resample (include/sdvpcm.h; no reference equivalent): 44 056 Hz -> 44 100 Hz on the pair stream
 * (audio_resample_device.h) and, with a delay bit in the mode, the half-sample skew stage behind it (audio_skew_device.h).  Included by
 * audio_engine.inc after audio_deemph_engine.inc.  A call runs stage A - off (mode 0: a copy and a sync), the resampler's three launches, or nothing (a delay bit alone: the
 * skew stage reads the caller's pairs where they lie) - then, with a delay bit, the skew stage's one launch, which takes the resampler's count from
 * device memory, and reads back once, behind whatever ran: RsResult, or SkResult with the resampler's result in it.  The open segments - counters here,
 * the last pairs of each stage on the device - move only when the read-back has succeeded and the counts fit the room.
 */
struct AudioSkew {
    /* the pairs its open segment has seen (SK_MANY: more than its history holds), its last SK_HIST pairs (on the device), the half-sample row here and
     * there, the resampler's output where the stage follows it, the call's result */
    uint32_t seen = 0;
    rt::DevBuf<sdv_sample_pair> d_hist, d_hist_spare, d_mid;
    std::vector<double> taps; rt::DevBuf<double> d_taps; bool taps_ready = false;
    rt::DevBuf<sdva::SkResult> d_result;
};
struct AudioResample {
    /* the mode; the open segment between two calls - pairs seen, outputs emitted, its last RS_HIST pairs (on the device) -;
     * the tap table ([k][phase], made on first use) here and there, a summary and a start per tile, the call's result */
    int mode = SDV_RESAMPLE_OFF; uint64_t seen = 0, emitted = 0;
    rt::DevBuf<sdv_sample_pair> d_hist, d_hist_spare;
    std::vector<double> taps; rt::DevBuf<double> d_taps; bool taps_ready = false;
    rt::DevBuf<sdva::RsSum> d_sums; rt::DevBuf<sdva::RsStart> d_starts; rt::DevBuf<sdva::RsResult> d_result;
    AudioSkew skew;                 /* its skew stage (a delay bit in the mode) */
};
static AudioResample *resample_get(sdv_engine *e);         /* its place is in sdv_audio (decode_frames_engine.inc) */
static const AudioResample *resample_peek(const sdv_engine *e);
enum { RS_DELAY_BITS = SDV_RESAMPLE_DELAY_RIGHT | SDV_RESAMPLE_DELAY_LEFT };
static size_t sk_waiting(const AudioResample *t) { return (size_t)std::min<uint32_t>(t->skew.seen, (uint32_t)sdva::SK_WAIT); }
/* outputs the first j pairs of a segment own (sdva::rs_owned) */
static uint64_t rs_owned_host(uint64_t j) { return j == 0 ? 0 : j + (j - 1) / SDV_RESAMPLE_M; }

extern "C" {

void sdv_resample_taps(int phase, double taps[128])
{
    if (phase != SDV_RESAMPLE_PHASE_HALF && (phase < 0 || phase >= SDV_RESAMPLE_L)) { for (int k = 0; k < 128; k++) taps[k] = 0.0; return; }
    kaiser_sinc_row(phase == SDV_RESAMPLE_PHASE_HALF ? 0.5 : (double)phase / (double)SDV_RESAMPLE_L, taps);
}

int sdv_set_resample(sdv_engine *e, int mode)
{
    if (!e) return SDV_ERR_BAD_ARG;
    const int delay = mode & RS_DELAY_BITS;
    if (mode < 0 || (mode & ~(SDV_RESAMPLE_TO_44100 | RS_DELAY_BITS)) || delay == RS_DELAY_BITS) { set_error(e, "no such resampling mode"); return SDV_ERR_BAD_ARG; }
    AudioResample *t = resample_get(e);
    if (delay != (t->mode & RS_DELAY_BITS) && t->skew.seen > 0) {
        set_error(e, "the skew stage holds waiting pairs of the delay that is set: flush (sdv_audio_resample) or reset (sdv_reset_resample) first");
        return SDV_ERR_BAD_ARG;
    }
    t->mode = mode;
    return SDV_OK;
}

int sdv_reset_resample(sdv_engine *e)
{
    if (!e) return SDV_ERR_BAD_ARG;
    AudioResample *t = resample_get(e);
    t->seen = 0; t->emitted = 0; t->skew.seen = 0;
    return SDV_OK;
}

size_t sdv_audio_resample_pending(const sdv_engine *e)
{
    const AudioResample *t = resample_peek(e);
    return t ? (size_t)std::min<uint64_t>(t->seen, (uint64_t)SDV_RESAMPLE_HALF) + sk_waiting(t) : 0;
}

size_t sdv_audio_resample_room(const sdv_engine *e, size_t n_pairs)
{
    const AudioResample *t = resample_peek(e);
    if (!t || t->mode == SDV_RESAMPLE_OFF) return n_pairs;
    /* (the skew stage puts out one pair per pair it is given, and what waited in it) */
    if (!(t->mode & SDV_RESAMPLE_TO_44100)) return n_pairs + sk_waiting(t);
    /* what the open segment owes when it ends, and per new pair one output and one more per thousand (a segment of n new pairs owns
     * n + floor((n - 1) / 1000); n pairs that continue the open one at most ceil(n 1001 / 1000) more than it owes) */
    return (size_t)(rs_owned_host(t->seen) - t->emitted) + n_pairs + n_pairs / SDV_RESAMPLE_M + 2 + sk_waiting(t);
}

/* The resampler's three launches for one call, its result left in d_result (the caller reads it back, or the skew stage does on the device). */
static int rs_queue(sdv_engine *e, AudioResample *t, const sdv_sample_pair *pairs, size_t n_pairs, int flush, sdv_sample_pair *out_pairs, size_t out_cap, rt::stream_t s)
{
    const int rc = stage_upload_taps(e, sdv_resample_taps, 0, SDV_RESAMPLE_L, sdva::RS_PITCH, t->taps, t->d_taps, t->taps_ready, s);
    if (rc != SDV_OK) return rc;
    const size_t n_tiles = (n_pairs + sdva::RS_TILE - 1) / sdva::RS_TILE;
    RT_CHECK(rt::reserve_all(sdva::RS_HIST, sdva::RS_HIST, t->d_hist, t->d_hist_spare));
    RT_CHECK(t->d_result.reserve(1));
    RT_CHECK(t->d_sums.reserve(n_tiles + 1, n_tiles + n_tiles / 8 + 64));
    RT_CHECK(t->d_starts.reserve(n_tiles + 1, n_tiles + n_tiles / 8 + 64));
    sdva::RsArgs a; memset(&a, 0, sizeof(a));
    a.in = pairs; a.out = out_pairs; a.n = (int64_t)n_pairs; a.out_cap = out_cap; a.hist = t->d_hist; a.hist_out = t->d_hist_spare;
    a.taps = t->d_taps; a.sums = t->d_sums; a.starts = t->d_starts; a.result = t->d_result;
    a.seen0 = t->seen; a.emitted0 = t->emitted; a.n_tiles = (uint32_t)n_tiles; a.flush = flush ? 1 : 0;
    RT_LAUNCH64(sdv_k_resample_classify, n_tiles, a, s);
    RT_LAUNCH64(sdv_k_resample_scan, 1, a, s);
    RT_LAUNCH64(sdv_k_resample_emit, n_tiles ? n_tiles : 1, a, s);
    return SDV_OK;
}

int sdv_audio_resample(sdv_engine *e, const sdv_sample_pair *pairs, size_t n_pairs, int flush, sdv_sample_pair *out_pairs, size_t out_cap, size_t *n_out, void *stream)
{
    if (!e || !n_out) return SDV_ERR_BAD_ARG;
    *n_out = 0;
    AudioResample *t = resample_get(e); AudioSkew *k = &t->skew;
    /* stage A: the resampler (it also runs for the tail alone), or with no bit set the copy; the skew stage behind it: for pairs, or for its own tail */
    const bool to_44100 = (t->mode & SDV_RESAMPLE_TO_44100) != 0, delayed = (t->mode & RS_DELAY_BITS) != 0;
    const bool run_a = to_44100 && (n_pairs > 0 || (flush && t->seen > 0)), copy = t->mode == SDV_RESAMPLE_OFF && n_pairs > 0;
    const bool run_skew = delayed && (run_a || n_pairs > 0 || (flush && k->seen > 0));
    if (!run_a && !copy && !run_skew) {
        /* nothing in and no tail to put out: the call only ends what it ends (a flush; a mode without the resampler ends the resampler's segment) */
        if (flush || !to_44100) { t->seen = 0; t->emitted = 0; }
        if (flush) k->seen = 0;
        return SDV_OK;
    }
    int rc = stage_check_pairs(e, pairs, n_pairs, out_pairs, true);
    if (rc != SDV_OK) return rc;
    const size_t room = sdv_audio_resample_room(e, n_pairs), room_a = room - sk_waiting(t);
    if (out_cap < room) {
        set_error(e, "output buffer too small: room for " + std::to_string((unsigned long long)room) + " sample pairs is needed (sdv_audio_resample_room)");
        return SDV_ERR_BAD_ARG;
    }
    rc = stage_check_apart(e, pairs, n_pairs * sizeof(sdv_sample_pair), out_pairs, out_cap * sizeof(sdv_sample_pair), "the output overlaps the input");
    if (rc != SDV_OK) return rc;
    SDV_ON_DEVICE(e);
    rt::stream_t s = (rt::stream_t)stream;
    sdva::SkResult res; memset(&res, 0, sizeof(res));
    if (copy) {
        RT_CHECK(rt::d2d(out_pairs, pairs, n_pairs * sizeof(sdv_sample_pair), s));
        RT_CHECK(rt::ssync(s));
        res.n_out = n_pairs;
    }
    if (run_skew) {
        rc = stage_upload_taps(e, sdv_resample_taps, SDV_RESAMPLE_PHASE_HALF, 1, 1, k->taps, k->d_taps, k->taps_ready, s);
        if (rc != SDV_OK) return rc;
        RT_CHECK(rt::reserve_all(sdva::SK_HIST, sdva::SK_HIST, k->d_hist, k->d_hist_spare));
        RT_CHECK(k->d_result.reserve(1));
        if (run_a) RT_CHECK(k->d_mid.reserve(room_a, room_a + room_a / 8 + 4096));
    }
    if (run_a) rc = run_skew ? rs_queue(e, t, pairs, n_pairs, flush, k->d_mid, room_a, s) : rs_queue(e, t, pairs, n_pairs, flush, out_pairs, out_cap, s);
    if (rc != SDV_OK) return rc;
    if (run_skew) {
        sdva::SkArgs a; memset(&a, 0, sizeof(a));
        a.in = pairs; a.n = (int64_t)n_pairs;
        if (run_a) { a.in = k->d_mid; a.n = (int64_t)room_a; a.a_result = t->d_result; }
        a.out = out_pairs; a.out_cap = out_cap; a.hist = k->d_hist; a.hist_out = k->d_hist_spare; a.taps = k->d_taps; a.result = k->d_result;
        a.seen0 = k->seen; a.flush = flush ? 1 : 0; a.channel = (t->mode & SDV_RESAMPLE_DELAY_RIGHT) ? 1 : 0;
        const size_t n_tiles = ((size_t)a.n + sdva::SK_TILE - 1) / sdva::SK_TILE;
        RT_LAUNCH64(sdv_k_skew, n_tiles ? n_tiles : 1, a, s);
    }
    /* one read-back, behind whatever ran */
    if (run_skew) RT_CHECK(rt::d2h(&res, k->d_result, sizeof(res), s));
    else if (run_a) { RT_CHECK(rt::d2h(&res.a, t->d_result, sizeof(res.a), s)); res.n_out = res.a.n_out; }
    if (res.n_out > out_cap || (run_a && res.a.n_out > (run_skew ? room_a : out_cap))) { set_error(e, "internal: the resampler counted more outputs than sdv_audio_resample_room allows"); return SDV_ERR_HIP; }
    /* the open segments move: a resampler that did not run keeps its segment unless the call ends it (a flush; a mode without the resampler) */
    if (run_a) { t->d_hist.swap(t->d_hist_spare); t->seen = res.a.seen; t->emitted = res.a.emitted; }
    else if (flush || !to_44100) { t->seen = 0; t->emitted = 0; }
    if (run_skew) { k->d_hist.swap(k->d_hist_spare); k->seen = res.seen; }
    *n_out = (size_t)res.n_out;
    return SDV_OK;
}

} // extern "C"
