/*
 * pcm_resample_device.h - device side of sdv_pcm_resample (include/sdvpcm.h): 44 100 Hz interleaved int16 PCM to 44 056 Hz by the 1000 / 1001
 * polyphase filter, for gfx950.  Included by engine.inc behind pcm_preemph_device.h; compiled by hipcc into the product and by g++ on the SIMT
 * emulator for the CPU tests (tests/emu).  The reference has no such stage: the definition is the one in the header.
 *
 * Output m of a stream reads the pairs i0 - 63 .. i0 + 64, i0 = m + floor(m / 1000), with the taps of phase m mod 1000.  Outputs 1000 apart share
 * their phase and lie 1001 pairs apart in the input, so the outputs are tiled by their index in the stream, not in the call: a tile is PR_G = 4
 * rows of 1000 outputs, row = floor(m / 1000), and a workgroup (one wave) takes a quarter of the phases, 256, of the tile's four rows.  Lane l of
 * round r owns the phase 256 q + 64 r + l in every row: a tap is loaded once - from the [tap][phase] transposed table, a round's loads of tap k
 * one run of 64 doubles - and used for PR_G outputs.  That is a quarter of the table traffic of a lane per output (audio_resample_device.h).
 * The pairs a quarter reads, 256 + 127 per row, go through LDS as one dword per pair, converted once to two floats (an int16 is exact in a
 * float); positions are clamped on the way in (to the stream's first pair, to the last one seen: the edge hold), the sums run without a test.
 * A call emits the outputs [m_lo, m_hi) of the stream - the host knows both ahead of the launch - and the lanes whose output lies outside
 * drop it; rounds with no output in the range are skipped.  Pairs in front of the call come from the engine's history, the last 127 pairs;
 * the workgroup behind the last quarter writes the next call's history to the spare buffer.  No atomics, no scratch; nothing is written that
 * another wave of the launch reads.  The 128-term sums run in double, k ascending.
 */
#pragma once
#include "pcm_preemph_device.h"

namespace sdvc {

enum { PR_G = 4,                        /* rows of 1000 outputs per tile (not part of the ABI: no output depends on it) */
       PR_PHASES = SDV_PCM_RESAMPLE_L, PR_STEP = SDV_PCM_RESAMPLE_M, PR_TILE = PR_G * PR_PHASES,
       PR_HALF = 64, PR_TAPS = 2 * PR_HALF, PR_HIST = PR_TAPS - 1,
       PR_SPAN = 256, PR_QUARTERS = (PR_PHASES + PR_SPAN - 1) / PR_SPAN, PR_ROUNDS = PR_SPAN / 64,
       PR_WIN = PR_SPAN + PR_TAPS,      /* pairs of a row a quarter reads (the last one is never used) */
       PR_PITCH = 1024 };               /* doubles per row of the transposed table; the phases 1000 .. 1023 hold zeros */
static_assert(PR_STEP == PR_PHASES + 1 && PR_PITCH >= PR_QUARTERS * PR_SPAN && PR_WIN % 64 == 0, "the geometry include/sdvpcm.h documents");

struct PrPair { float l, r; };
struct PrArgs {
    const uint32_t *in; uint32_t *out;
    const uint32_t *hist; uint32_t *hist_out;           /* PR_HIST pairs: the positions seen - PR_HIST .. seen - 1 */
    const double *taps;                                 /* [PR_TAPS][PR_PITCH] */
    uint64_t seen0, seen1;                              /* pairs of the stream in front of the call, and behind it (seen1 >= 1 where anything is emitted) */
    uint64_t m_lo, m_hi;                                /* the outputs of the stream the call emits; out[0] is output m_lo */
    uint64_t row0;                                      /* the first tile's first row */
    uint32_t n_blocks;                                  /* tiles x PR_QUARTERS; workgroup n_blocks writes the history */
    int keep_hist;
};
struct PrLds { PrPair x[PR_G * PR_WIN]; };

__device__ __forceinline__ uint32_t pr_fetch(const PrArgs &a, int64_t pos)      /* seen0 - PR_HIST <= pos < seen1, pos >= 0 */
{
    const int64_t i = pos - (int64_t)a.seen0;
    return i >= 0 ? a.in[i] : a.hist[PR_HIST + i];
}

__device__ inline void pcm_resample_body(const PrArgs &a, uint32_t block, PrLds &lds, int lane)
{
    if (block >= a.n_blocks) {
        if (a.keep_hist)
            for (int k = lane; k < PR_HIST; k += 64) {
                const int64_t pos = (int64_t)a.seen1 - PR_HIST + k;
                if (pos >= 0) a.hist_out[k] = pr_fetch(a, pos);
            }
        return;
    }
    const uint64_t row = a.row0 + (uint64_t)(block / PR_QUARTERS) * PR_G;
    const uint32_t p0 = (block % PR_QUARTERS) * PR_SPAN;
    /* what exists: no emitted output reads in front of the history */
    const int64_t first = a.seen0 > (uint64_t)PR_HIST ? (int64_t)(a.seen0 - PR_HIST) : 0, last = (int64_t)a.seen1 - 1;
#pragma unroll
    for (int g = 0; g < PR_G; g++) {
        const int64_t w0 = (int64_t)((row + g) * PR_STEP) + p0 - (PR_HALF - 1);
        for (int j = lane; j < PR_WIN; j += 64) {
            int64_t pos = w0 + j; pos = pos < first ? first : pos; pos = pos > last ? last : pos;
            const uint32_t w = pr_fetch(a, pos);
            PrPair v; v.l = (float)(int16_t)(uint16_t)(w & 0xFFFFu); v.r = (float)(int16_t)(uint16_t)(w >> 16);
            lds.x[g * PR_WIN + j] = v;
        }
    }
    __syncthreads();
    for (int r = 0; r < PR_ROUNDS; r++) {
        const uint32_t pr = p0 + 64u * r;               /* the round's first phase */
        if (pr >= (uint32_t)PR_PHASES) break;
        bool any = false;                               /* (the same for every lane) */
#pragma unroll
        for (int g = 0; g < PR_G; g++) { const uint64_t m0 = (row + g) * PR_PHASES + pr; any = any || (m0 + 64 > a.m_lo && m0 < a.m_hi); }
        if (!any) continue;
        const uint32_t p = pr + (uint32_t)lane;         /* (phases 1000 .. 1023 of the last round: zeros of the table, nothing stored) */
        const double *h = a.taps + p;
        const PrPair *x = lds.x + 64 * r + lane;
        double y[PR_G][2];
#pragma unroll
        for (int g = 0; g < PR_G; g++) y[g][0] = y[g][1] = 0.0;
#pragma unroll 8
        for (int k = 0; k < PR_TAPS; k++) {
            const double c = h[(size_t)k * PR_PITCH];
#pragma unroll
            for (int g = 0; g < PR_G; g++) { const PrPair v = x[g * PR_WIN + k]; y[g][0] += c * (double)v.l; y[g][1] += c * (double)v.r; }
        }
        if (p >= (uint32_t)PR_PHASES) continue;
#pragma unroll
        for (int g = 0; g < PR_G; g++) {
            const uint64_t m = (row + g) * PR_PHASES + p;
            int clipped = 0;
            if (m >= a.m_lo && m < a.m_hi) a.out[m - a.m_lo] = pcm_round(y[g][0], clipped) | (pcm_round(y[g][1], clipped) << 16);
        }
    }
}

} // namespace sdvc

__global__ void __launch_bounds__(64) sdv_k_pcmrs(sdvc::PrArgs a)
{
    __shared__ sdvc::PrLds lds;
    sdvc::pcm_resample_body(a, blockIdx.x, lds, (int)threadIdx.x);
}
