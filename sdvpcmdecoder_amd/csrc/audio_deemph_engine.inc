/*
 * audio_deemph_engine.inc - host side of sdv_audio_deemphasis (include/sdvpcm.h; no reference equivalent): 50/15 us de-emphasis of the pair stream
 * (audio_deemph_device.h).  Included by audio_engine.inc, at its end.  A call is two launches - the state in front of every tile from the input alone, then
 * the tiles - and reads nothing back: the filter between two calls stays on the device.
 */
struct AudioDeemph {
    /* the mode, the filter between two calls (on the device; idle: not looked at, the next call starts idle), a record per tile */
    int mode = SDV_DEEMPH_OFF; bool idle = true;
    rt::DevBuf<sdva::DeState> d_state, d_tiles;
};
static AudioDeemph *deemph_get(sdv_engine *e);             /* its place is in sdv_audio (decode_frames_engine.inc) */

extern "C" {
void sdv_deemphasis_coeffs(uint16_t sample_rate, double c[3])
{
    const double fs = sample_rate == 44056 ? 44056.0 : 44100.0, K = 2.0 * fs, T1 = 50e-6, T2 = 15e-6;
    c[0] = (1.0 + K * T2) / (1.0 + K * T1);
    c[1] = (1.0 - K * T2) / (1.0 + K * T1);
    c[2] = (1.0 - K * T1) / (1.0 + K * T1);
}

int sdv_set_deemphasis(sdv_engine *e, int mode)
{
    if (!e) return SDV_ERR_BAD_ARG;
    if (mode != SDV_DEEMPH_OFF && mode != SDV_DEEMPH_AUTO && mode != SDV_DEEMPH_FORCE) { set_error(e, "no such de-emphasis mode"); return SDV_ERR_BAD_ARG; }
    deemph_get(e)->mode = mode;
    return SDV_OK;
}

int sdv_reset_deemphasis(sdv_engine *e)
{
    if (!e) return SDV_ERR_BAD_ARG;
    deemph_get(e)->idle = true;
    return SDV_OK;
}

int sdv_audio_deemphasis(sdv_engine *e, const sdv_sample_pair *pairs, size_t n, sdv_sample_pair *out_pairs, void *stream)
{
    if (!e) return SDV_ERR_BAD_ARG;
    AudioDeemph *t = deemph_get(e);
    if (n == 0) { if (t->mode == SDV_DEEMPH_OFF) t->idle = true; return SDV_OK; }
    int rc = stage_check_pairs(e, pairs, n, out_pairs, true);
    if (rc == SDV_OK && out_pairs != pairs) rc = stage_check_apart(e, pairs, n * sizeof(sdv_sample_pair), out_pairs, n * sizeof(sdv_sample_pair), "the output overlaps the input without being the input");
    if (rc != SDV_OK) return rc;
    SDV_ON_DEVICE(e);
    rt::stream_t s = (rt::stream_t)stream;
    if (t->mode == SDV_DEEMPH_OFF) {
        if (out_pairs != pairs) RT_CHECK(rt::d2d(out_pairs, pairs, n * sizeof(sdv_sample_pair), s));
        t->idle = true;
        return SDV_OK;
    }
    const size_t n_tiles = (n + sdva::DE_TILE - 1) / sdva::DE_TILE;
    RT_CHECK(t->d_state.reserve(1));
    RT_CHECK(t->d_tiles.reserve(n_tiles, n_tiles + n_tiles / 8 + 64));
    sdva::DeArgs a; memset(&a, 0, sizeof(a));
    a.in = pairs; a.out = out_pairs; a.n = n; a.tiles = t->d_tiles; a.state = t->d_state;
    sdv_deemphasis_coeffs(44056, a.c[0]); sdv_deemphasis_coeffs(44100, a.c[1]);
    a.force = t->mode == SDV_DEEMPH_FORCE ? 1 : 0; a.head_idle = t->idle ? 1 : 0;
    /* the state in front of every tile from the input alone, then the tiles: the second pass reads nothing another tile writes (a call in place) */
    RT_LAUNCH64(sdv_k_deemph_warm, n_tiles, a, s);
    RT_LAUNCH64(sdv_k_deemph, n_tiles, a, s);
    t->idle = false;
    return SDV_OK;
}

} // extern "C"
