/*
 * stage_common.inc - what the host files of the sample-stream stages share (pcm_condition_engine.inc, audio_engine.inc and the stage files behind
 * it): the limit of a call, the checks of a call's buffers, the Kaiser-sinc row of the two resamplers and the skew stage, and the upload of a table
 * of such rows.  Included by engine.inc in front of the first of them.  It launches nothing and reads nothing back.
 * Naming: state that a launch writes lies in a second buffer, <name>_spare, grown with the first (rt::reserve_all) and swapped with it once the call
 * has succeeded.
 */
enum : uint32_t { STAGE_MAX_PAIRS = 0x7FFF0000u };      /* a call takes fewer pairs than this: positions and counts fit the kernels' 32-bit fields */

/* do the byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte? */
static inline bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) { return (const char *)a < (const char *)b + b_bytes && (const char *)b < (const char *)a + a_bytes; }
static int stage_check_apart(sdv_engine *e, const void *in, size_t in_bytes, const void *out, size_t out_bytes, const char *text)
{
    if (!ranges_overlap(in, in_bytes, out, out_bytes)) return SDV_OK;
    set_error(e, text); return SDV_ERR_BAD_ARG;
}
/* the pair buffers of a stage's call: n pairs in (none: no buffer is asked for) and, with `need_out`, a buffer to write to.  Whether the two may
 * share bytes is the stage's to say (stage_check_apart, with its own text). */
static int stage_check_pairs(sdv_engine *e, const sdv_sample_pair *pairs, size_t n, const sdv_sample_pair *out, bool need_out)
{
    if (n > 0 && !pairs) { set_error(e, "null sample pair buffer"); return SDV_ERR_NULL_LINES; }
    if (n >= STAGE_MAX_PAIRS) { set_error(e, "too many sample pairs in one call"); return SDV_ERR_BAD_ARG; }
    if (need_out && !out) { set_error(e, "null output buffer"); return SDV_ERR_NULL_BLOCK; }
    return SDV_OK;
}
/* the two interleaved int16 PCM buffers of a call (4 bytes per pair): 4-byte aligned, apart */
static int stage_check_pcm(sdv_engine *e, const int16_t *pcm, size_t n_in, const int16_t *out, size_t n_out)
{
    if ((((uintptr_t)pcm) | ((uintptr_t)out)) & 3u) { set_error(e, "a pcm buffer is not 4-byte aligned"); return SDV_ERR_BAD_ARG; }
    return n_in && n_out ? stage_check_apart(e, pcm, 4 * n_in, out, 4 * n_out, "the output overlaps the input") : SDV_OK;
}

/* ---- the Kaiser-windowed sinc (beta = 12.0, SDV_RESAMPLE_HALF taps on each side: include/sdvpcm.h) ------------------------------------------ */
static double bessel_i0(double x)
{
    const double q = x * x / 4.0;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; k++) { term *= q / ((double)k * (double)k); sum += term; if (term < 1e-18 * sum) break; }
    return sum;
}
/* the row for an output that lies `frac` of a sample behind input SDV_RESAMPLE_HALF - 1 of the 128 it reads */
static void kaiser_sinc_row(double frac, double taps[128])
{
    const double beta = 12.0, pi = 3.14159265358979323846, i0_beta = bessel_i0(beta);
    long double sum = 0.0L;             /* (the normalisation must not cost the rows their gain of 1 at DC) */
    for (int k = 0; k < 128; k++) {
        const double d = (double)(k - (SDV_RESAMPLE_HALF - 1)) - frac;
        double r = 1.0 - (d / SDV_RESAMPLE_HALF) * (d / SDV_RESAMPLE_HALF);
        if (r < 0.0) r = 0.0;
        const double w = bessel_i0(beta * sqrt(r)) / i0_beta, x = pi * d;
        taps[k] = (d == 0.0 ? 1.0 : sin(x) / x) * w;
        sum += (long double)taps[k];
    }
    const double total = (double)sum;
    for (int k = 0; k < 128; k++) taps[k] /= total;
}

/* The rows `row_of` gives for the phases [phase0, phase0 + n_phases), transposed - table[tap][phase - phase0], `pitch` doubles per tap: the 64 lanes of
 * a wave walk neighbouring phases of one tap - and on the device: made on a stage's first call.  `table` belongs to the stage's state and lives as long
 * as the engine, so the upload is only queued: nothing here waits for the stream. */
static int stage_upload_taps(sdv_engine *e, void (*row_of)(int, double *), int phase0, int n_phases, size_t pitch, std::vector<double> &table, rt::DevBuf<double> &d_taps, bool &ready, rt::stream_t s)
{
    if (ready) return SDV_OK;
    table.assign(128 * pitch, 0.0);
    double row[128];
    for (int p = 0; p < n_phases; p++) { row_of(phase0 + p, row); for (int k = 0; k < 128; k++) table[(size_t)k * pitch + p] = row[k]; }
    RT_CHECK(d_taps.reserve(table.size()));
    RT_CHECK(rt::h2d(d_taps, table.data(), table.size() * sizeof(double), s));
    ready = true;
    return SDV_OK;
}
