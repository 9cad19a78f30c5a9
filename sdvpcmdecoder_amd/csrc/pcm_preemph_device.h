/*
 * pcm_preemph_device.h - device side of sdv_pcm_preemphasis (include/sdvpcm.h): the 15/50 us pre-emphasis network on interleaved int16 PCM,
 * for gfx950.  Included by engine.inc; compiled by hipcc into the product and by g++ on the SIMT emulator for the CPU tests (tests/emu).
 * The reference has no such stage: the definition is the one in the header.
 *
 * The filter is y[i] = c0 x[i] + c1 x[i-1] - c2 y[i-1] per channel, on every pair of the call at one rate.  Its pole is -c2 = 0.139, and
 * 0.139^32 = 3e-28: what a state owes to the pairs more than PE_WARM = 32 back is far below the rounding of a double.  So nothing is scanned:
 * a lane owns PE_R = 16 consecutive pairs and runs the recurrence itself from the pair PE_WARM in front of its first (where it starts as a
 * stream does, y = x), 48 steps for 16 words - three times the arithmetic of a walk, in one pass, with no wave waiting for another.  The lanes
 * whose warm-up would begin in front of the call's first pair begin at that pair, from the state the stream's last call left: exact.
 * A tile is one wave's: 64 lanes x PE_R pairs.  A pair is one dword (L | R << 16); the tile and the PE_WARM pairs in front of it cross global
 * memory as rows of 16 bytes per lane where the buffer is 16-byte aligned (dwords else, and at the ragged ends) and are regrouped per lane
 * through LDS, a lane's run PE_R + 1 dwords from the next (odd: no bank conflicts).  The state behind the call's last pair goes to a second
 * record (the host swaps the two): no wave reads what another writes.  Clipped words are counted per lane, summed over the wave bit by bit
 * with ballots and added to the counter once per wave: integers, so the total does not depend on the order.  All arithmetic is in double.
 */
#pragma once
#include <math.h>

namespace sdvc {

enum { PE_R = 16, PE_TILE = 64 * PE_R, PE_WARM = 32, PE_STAGE = PE_WARM + PE_TILE, PE_RUN = PE_WARM + PE_R, PE_LDS_PITCH = PE_R + 1,
       PE_IN_ROWS = (PE_STAGE / 4 + 63) / 64, PE_OUT_ROWS = PE_TILE / 4 / 64 };
static_assert(PE_TILE == SDV_PREEMPH_TILE && PE_WARM == SDV_PREEMPH_WARMUP && PE_WARM % PE_R == 0 && PE_WARM % 4 == 0, "the tile geometry include/sdvpcm.h documents");
enum { PE_KEY_IDLE = 0, PE_KEY_44056 = 1, PE_KEY_44100 = 2 };

/* The filter between two calls: the rate it ran at (PE_KEY_*), the last pair's input words and unrounded outputs.  All zero = idle. */
struct PeState { double x[2], y[2]; uint32_t key, _pad; };
struct PeArgs {
    const uint32_t *in; uint32_t *out; uint64_t n;      /* pairs */
    const PeState *state_in; PeState *state_out;        /* of the stream: read by the lanes that begin at the call's first pair (unless head_idle), written behind the last */
    unsigned long long *clipped;
    double c[3];                                        /* 1 / b0, a1 / b0, b1 / b0 at the call's rate (sdv_preemphasis_coeffs) */
    uint32_t key;                                       /* PE_KEY_44056 / PE_KEY_44100 */
    uint8_t head_idle, vec_in, vec_out;                 /* vec_*: the buffer is 16-byte aligned */
};
struct PeLds { uint32_t w[PE_STAGE + PE_STAGE / PE_R]; };
typedef uint32_t PeRow __attribute__((vector_size(16)));       /* four pairs: one 16-byte load or store of a lane (a vector type, so that it stays one) */

__device__ __forceinline__ double pcm_x(uint32_t w, int ch) { return (double)(int16_t)(uint16_t)(ch ? w >> 16 : w & 0xFFFFu); }
/* y rounded to nearest (halves to even) and clamped to the 16-bit range; clipped: the clamp changed it */
__device__ __forceinline__ uint32_t pcm_round(double y, int &clipped)
{
    double r = rint(y);
    if (r < -32768.0) { r = -32768.0; clipped++; } else if (r > 32767.0) { r = 32767.0; clipped++; }
    return (uint32_t)(uint16_t)(int16_t)(int)r;
}
__device__ __forceinline__ uint32_t pe_slot(uint32_t q) { return q + q / (uint32_t)PE_R; }     /* stage position -> LDS dword */

__device__ inline void preemph_body(const PeArgs &a, uint32_t tile, PeLds &lds, int lane)
{
    const uint64_t base = (uint64_t)tile * PE_TILE;
    const uint32_t n_tile = a.n - base < (uint64_t)PE_TILE ? (uint32_t)(a.n - base) : (uint32_t)PE_TILE;
    /* stage position q is pair base - PE_WARM + q of the call; [lo, hi) exist */
    const uint32_t lo = tile == 0 ? (uint32_t)PE_WARM : 0u, hi = (uint32_t)PE_WARM + n_tile;
    {
        PeRow v[PE_IN_ROWS];
#pragma unroll
        for (int j = 0; j < PE_IN_ROWS; j++) {
            const uint32_t q = 4u * ((uint32_t)j * 64u + (uint32_t)lane);
            v[j] = PeRow{ 0u, 0u, 0u, 0u };
            if (q >= (uint32_t)PE_STAGE || q < lo || q >= hi) continue;         /* (lo and q are multiples of 4: a row of four lies on one side of lo) */
            const uint32_t *src = a.in + (base + q - (uint32_t)PE_WARM);
            if (a.vec_in && q + 4u <= hi) v[j] = *reinterpret_cast<const PeRow *>(src);
            else for (uint32_t k = 0; k < 4u && q + k < hi; k++) v[j][k] = src[k];
        }
#pragma unroll
        for (int j = 0; j < PE_IN_ROWS; j++) {
            const uint32_t q = 4u * ((uint32_t)j * 64u + (uint32_t)lane);
            if (q >= (uint32_t)PE_STAGE) continue;
            const uint32_t s = pe_slot(q);              /* (q is a multiple of 4: the four dwords lie side by side) */
            lds.w[s] = v[j][0]; lds.w[s + 1] = v[j][1]; lds.w[s + 2] = v[j][2]; lds.w[s + 3] = v[j][3];
        }
    }
    __syncthreads();
    /* the lane's run: its PE_R pairs at d[PE_WARM ..], the PE_WARM pairs in front of them at d[0 ..] */
    uint32_t d[PE_RUN];
#pragma unroll
    for (int k = 0; k < PE_RUN; k++) d[k] = lds.w[lane * PE_LDS_PITCH + k + k / PE_R];
    __syncthreads();                    /* (the words go back where later lanes' warm-up pairs lay) */
    const int first = lane * PE_R, cnt = (int)n_tile - first < 0 ? 0 : (int)n_tile - first > PE_R ? PE_R : (int)n_tile - first;
    /* where the lane begins: PE_WARM pairs back as a stream begins, or at the call's first pair from the stream's state */
    const bool at_head = tile == 0 && first <= PE_WARM;
    const int k0 = at_head ? PE_WARM - first : 0;
    bool run = false;
    double xp0 = 0.0, xp1 = 0.0, y0 = 0.0, y1 = 0.0;
    if (at_head && !a.head_idle && cnt > 0) {
        const PeState s = *a.state_in;
        run = s.key == a.key; xp0 = s.x[0]; xp1 = s.x[1]; y0 = s.y[0]; y1 = s.y[1];
    }
    int clipped = 0;
#pragma unroll
    for (int k = 0; k < PE_RUN; k++) {
        if (k < k0 || k - PE_WARM >= cnt || cnt == 0) continue;        /* (not a break: the loop unrolls, d stays in registers) */
        const double x0 = pcm_x(d[k], 0), x1 = pcm_x(d[k], 1);
        if (!run) { y0 = x0; y1 = x1; run = true; }     /* the filter starts: the word stays */
        else {
            y0 = a.c[0] * x0 + a.c[1] * xp0 - a.c[2] * y0; y1 = a.c[0] * x1 + a.c[1] * xp1 - a.c[2] * y1;
            if (k >= PE_WARM) { const uint32_t w0 = pcm_round(y0, clipped), w1 = pcm_round(y1, clipped); d[k] = w0 | (w1 << 16); }
        }
        xp0 = x0; xp1 = x1;
    }
    if (cnt > 0 && base + (uint64_t)first + (uint64_t)cnt == a.n) {
        PeState o; o.key = a.key; o._pad = 0; o.x[0] = xp0; o.x[1] = xp1; o.y[0] = y0; o.y[1] = y1;
        *a.state_out = o;
    }
    /* a lane clipped 0 .. 2 PE_R words: the wave's sum, a bit of the counts at a time */
    unsigned long long total = 0;
#pragma unroll
    for (int b = 0; b < 6; b++) total += (unsigned long long)__popcll((unsigned long long)__ballot((clipped >> b) & 1)) << b;
    if (lane == 0 && total) atomicAdd(a.clipped, total);
#pragma unroll
    for (int i = 0; i < PE_R; i++) lds.w[(lane + PE_WARM / PE_R) * PE_LDS_PITCH + i] = d[PE_WARM + i];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PE_OUT_ROWS; j++) {
        const uint32_t i = 4u * ((uint32_t)j * 64u + (uint32_t)lane);
        if (i >= n_tile) continue;
        const uint32_t s = pe_slot(i + (uint32_t)PE_WARM);
        uint32_t *dst = a.out + base + i;
        if (a.vec_out && i + 4u <= n_tile) *reinterpret_cast<PeRow *>(dst) = PeRow{ lds.w[s], lds.w[s + 1], lds.w[s + 2], lds.w[s + 3] };
        else for (uint32_t k = 0; k < 4u && i + k < n_tile; k++) dst[k] = lds.w[s + k];
    }
}

} // namespace sdvc

__global__ void __launch_bounds__(64) sdv_k_preemph(sdvc::PeArgs a)
{
    __shared__ sdvc::PeLds lds;
    sdvc::preemph_body(a, blockIdx.x, lds, (int)threadIdx.x);
}
