/*
 * audio_deemph_device.h - device side of sdv_audio_deemphasis (include/sdvpcm.h): the 50/15 us de-emphasis network on the
 * PCMSamplePair stream, for gfx950.  Included by audio_device.h; compiled by hipcc into the product and by g++ on the SIMT
 * emulator for the CPU tests (tests/emu).  The reference has no such stage: the definition is the one in the header.
 *
 * The filter is a first-order recurrence y[i] = b0 x[i] + b1 x[i-1] - a1 y[i-1] per channel, restarted (y = x) wherever a
 * selected pair follows one that is not selected, a service pair, or a pair of the other sample rate.  What makes it parallel:
 *   - whether pair i restarts, and every coefficient of its step, follow from pairs i and i - 1 alone, so a step is an affine
 *     map y -> P y + C known from the input (P = 0 at a restart, -a1 otherwise; P is the same for both channels), and a run of
 *     steps is the composition of their maps: a scan.  A lane composes its DE_R pairs, the wave scans the 64 composites with
 *     shuffles, every lane then walks its pairs once more from the state the scan hands it;
 *   - |a1| is about 0.63, so what a state owes to the pairs more than DE_WARM = 128 back is below the rounding of a double
 *     (0.63^128 = 2e-26): the state a tile starts from comes from the DE_WARM pairs in front of it (first pass, inputs only,
 *     into a scratch record per tile), tile 0 takes the state the stream's last call left.  No wave waits for another.
 * Two passes make a call in place exact: the second pass reads nothing outside its own tile but that record.
 * A tile is one wave's: 64 lanes x DE_R pairs.  The 12-byte pairs cross global memory as whole rows of dwords (any 4-byte
 * alignment of the buffers will do) and are regrouped per lane through LDS, a lane's run 3 DE_R + 1 dwords from the next
 * (odd: no bank conflicts).  All arithmetic is in double.
 */
#pragma once
#include <math.h>

namespace sdva {

enum { DE_R = 16, DE_TILE = 64 * DE_R, DE_WARM = 128, DE_RUN = 3 * DE_R, DE_LDS_PITCH = DE_RUN + 1 };
static_assert(DE_TILE == SDV_DEEMPH_TILE && DE_WARM == SDV_DEEMPH_WARMUP && DE_TILE % DE_WARM == 0, "the tile geometry include/sdvpcm.h documents");
enum { DE_KEY_IDLE = 0, DE_KEY_44056 = 1, DE_KEY_44100 = 2 };

/* The filter between two pairs: what the last pair was (DE_KEY_*: not selected, or the rate it ran at), its input words and its
 * unrounded outputs.  All zero = idle. */
struct DeState { double x[2], y[2]; uint32_t key, _pad; };
struct DeArgs {
    const sdv_sample_pair *in; sdv_sample_pair *out; size_t n;
    DeState *tiles;             /* one per tile: the state in front of its first pair */
    DeState *state;             /* of the stream: read by tile 0 (unless head_idle), written behind the last pair */
    double c[2][3];             /* b0, b1, a1 at 44056 and at 44100 (sdv_deemphasis_coeffs) */
    uint8_t force, head_idle;
};
struct DeLds { uint32_t w[64 * DE_LDS_PITCH]; };

__device__ __forceinline__ double de_pull(double v, int src)
{
    uint64_t u; __builtin_memcpy(&u, &v, 8);
    u = lane_pull64(u, src);
    __builtin_memcpy(&v, &u, 8);
    return v;
}
/* dwords 1 and 2 of a pair: flags, rate | emphasis, service_type, _pad */
__device__ __forceinline__ uint32_t de_key(uint32_t d1, uint32_t d2, bool force)
{
    const bool selected = ((d2 >> 8) & 0xFFu) == 0u && (force || (d2 & 0xFFu) != 0u);
    return !selected ? (uint32_t)DE_KEY_IDLE : (d1 >> 16) == 44056u ? (uint32_t)DE_KEY_44056 : (uint32_t)DE_KEY_44100;
}
struct DeCoef { double b0, b1, a1; };
__device__ __forceinline__ DeCoef de_coef(const DeArgs &a, uint32_t key)      /* (a select, not an index: the arguments stay where they are) */
{
    const bool lo = key == (uint32_t)DE_KEY_44056;
    DeCoef c; c.b0 = lo ? a.c[0][0] : a.c[1][0]; c.b1 = lo ? a.c[0][1] : a.c[1][1]; c.a1 = lo ? a.c[0][2] : a.c[1][2];
    return c;
}
__device__ __forceinline__ double de_x(uint32_t d0, int ch) { return (double)(int16_t)(uint16_t)(ch ? d0 >> 16 : d0 & 0xFFFFu); }

/* The composite map of the lane's `cnt` pairs d[3 i .. 3 i + 2], in front of which lay a pair of key `key`, words `w`. */
template <int R> __device__ __forceinline__ void de_compose(const uint32_t *d, int cnt, uint32_t key, uint32_t w, const DeArgs &a, double &P, double &C0, double &C1)
{
    P = 1.0; C0 = 0.0; C1 = 0.0;
#pragma unroll
    for (int i = 0; i < R; i++) {
        if (i >= cnt) continue;         /* (not a break: the loop unrolls, d stays in registers) */
        const uint32_t k = de_key(d[3 * i + 1], d[3 * i + 2], a.force != 0);
        const double x0 = de_x(d[3 * i], 0), x1 = de_x(d[3 * i], 1);
        if (k == (uint32_t)DE_KEY_IDLE) { P = 0.0; C0 = 0.0; C1 = 0.0; }        /* (any map will do: the next selected pair restarts) */
        else if (k != key) { P = 0.0; C0 = x0; C1 = x1; }
        else {
            const DeCoef c = de_coef(a, k);
            C0 = c.b0 * x0 + c.b1 * de_x(w, 0) - c.a1 * C0; C1 = c.b0 * x1 + c.b1 * de_x(w, 1) - c.a1 * C1; P = -c.a1 * P;
        }
        key = k; w = d[3 * i];
    }
}
/* Inclusive scan of the lanes' maps (the earlier lane's map is applied first). */
__device__ __forceinline__ void de_scan(double &P, double &C0, double &C1, int lane)
{
    for (int d = 1; d < 64; d <<= 1) {
        const int src = lane >= d ? lane - d : lane;
        const double Pp = de_pull(P, src), Cp0 = de_pull(C0, src), Cp1 = de_pull(C1, src);
        if (lane >= d) { C0 = P * Cp0 + C0; C1 = P * Cp1 + C1; P = P * Pp; }
    }
}
/* The key and the words of the last of the lane before's pairs (lane 0: `key0`, `w0`).  Lanes without pairs lie behind every lane that has some. */
template <int R> __device__ __forceinline__ void de_before(const uint32_t *d, int cnt, uint32_t key0, uint32_t w0, const DeArgs &a, int lane, uint32_t &key, uint32_t &w)
{
    uint32_t lk = 0, lw = 0;
#pragma unroll
    for (int i = 0; i < R; i++) if (i < cnt) { lk = de_key(d[3 * i + 1], d[3 * i + 2], a.force != 0); lw = d[3 * i]; }      /* (no index that is not a constant: d stays in registers) */
    const uint32_t pk = a_shfl(lk, lane > 0 ? lane - 1 : 0), pw = a_shfl(lw, lane > 0 ? lane - 1 : 0);
    key = lane > 0 ? pk : key0; w = lane > 0 ? pw : w0;
}

/* ---- first pass: the state in front of every tile ----------------------------------------------------------------------- */
__device__ inline void deemph_warm_body(const DeArgs &a, uint32_t tile, int lane)
{
    DeState s;
    if (tile == 0) {
        if (a.head_idle) { s.x[0] = s.x[1] = s.y[0] = s.y[1] = 0.0; s.key = DE_KEY_IDLE; s._pad = 0; }
        else s = *a.state;
        if (lane == 0) a.tiles[0] = s;
        return;
    }
    /* DE_WARM pairs in front of the tile, two per lane; the first of them restarts (exact when the pair before it was not selected,
     * forgotten otherwise) */
    const uint32_t *src = (const uint32_t *)(a.in + ((size_t)tile * DE_TILE - DE_WARM)) + 6 * lane;
    uint32_t d[6];
#pragma unroll
    for (int k = 0; k < 6; k++) d[k] = src[k];
    uint32_t key, w;
    de_before<2>(d, 2, DE_KEY_IDLE, 0u, a, lane, key, w);
    double P, C0, C1;
    de_compose<2>(d, 2, key, w, a, P, C0, C1);
    de_scan(P, C0, C1, lane);
    if (lane == 63) {
        s.key = de_key(d[4], d[5], a.force != 0); s._pad = 0;
        const bool run = s.key != (uint32_t)DE_KEY_IDLE;        /* (then some pair of the window restarted: the map is a constant) */
        s.x[0] = run ? de_x(d[3], 0) : 0.0; s.x[1] = run ? de_x(d[3], 1) : 0.0; s.y[0] = run ? C0 : 0.0; s.y[1] = run ? C1 : 0.0;
        a.tiles[tile] = s;
    }
}

/* ---- second pass: the tiles ---------------------------------------------------------------------------------------------- */
__device__ __forceinline__ uint32_t de_round(double y)
{
    double r = rint(y);                 /* half to even */
    r = r < -32768.0 ? -32768.0 : r > 32767.0 ? 32767.0 : r;
    return (uint32_t)(uint16_t)(int16_t)(int)r;
}
__device__ inline void deemph_body(const DeArgs &a, uint32_t tile, DeLds &lds, int lane)
{
    const size_t base = (size_t)tile * DE_TILE;
    const uint32_t n_tile = a.n - base < (size_t)DE_TILE ? (uint32_t)(a.n - base) : (uint32_t)DE_TILE, n_dw = 3u * n_tile;
    const uint32_t *src = (const uint32_t *)(a.in + base); uint32_t *dst = (uint32_t *)(a.out + base);
    const DeState s = a.tiles[tile];
    /* in: rows of 64 dwords, sixteen rows in flight */
    for (int j0 = 0; j0 < DE_RUN; j0 += 16) {
        uint32_t v[16];
#pragma unroll
        for (int j = 0; j < 16; j++) { const uint32_t g = (uint32_t)(j0 + j) * 64u + (uint32_t)lane; v[j] = g < n_dw ? src[g] : 0u; }
#pragma unroll
        for (int j = 0; j < 16; j++) { const uint32_t g = (uint32_t)(j0 + j) * 64u + (uint32_t)lane; lds.w[g + g / (uint32_t)DE_RUN] = v[j]; }
    }
    __syncthreads();
    uint32_t d[DE_RUN];
#pragma unroll
    for (int k = 0; k < DE_RUN; k++) d[k] = lds.w[lane * DE_LDS_PITCH + k];
    const int first = lane * DE_R, cnt = (int)n_tile - first < 0 ? 0 : (int)n_tile - first > DE_R ? DE_R : (int)n_tile - first;
    const uint32_t w_in = ((uint32_t)(uint16_t)(int16_t)s.x[0]) | ((uint32_t)(uint16_t)(int16_t)s.x[1] << 16);
    uint32_t key, w;
    de_before<DE_R>(d, cnt, s.key, w_in, a, lane, key, w);
    double P, C0, C1;
    de_compose<DE_R>(d, cnt, key, w, a, P, C0, C1);
    de_scan(P, C0, C1, lane);
    /* the outputs of the pair in front of the lane's first: the maps of the lanes before applied to the tile's state */
    const int prev = lane > 0 ? lane - 1 : 0;
    const double Pe = de_pull(P, prev), Ce0 = de_pull(C0, prev), Ce1 = de_pull(C1, prev);
    double y0 = lane > 0 ? Pe * s.y[0] + Ce0 : s.y[0], y1 = lane > 0 ? Pe * s.y[1] + Ce1 : s.y[1];
#pragma unroll
    for (int i = 0; i < DE_R; i++) {
        if (i >= cnt) continue;         /* (not a break: the loop unrolls, d stays in registers) */
        const uint32_t k = de_key(d[3 * i + 1], d[3 * i + 2], a.force != 0), w_own = d[3 * i];
        const double x0 = de_x(w_own, 0), x1 = de_x(w_own, 1);
        if (k != (uint32_t)DE_KEY_IDLE) {
            if (k != key) { y0 = x0; y1 = x1; }     /* a segment starts: the words stay */
            else {
                const DeCoef c = de_coef(a, k);
                y0 = c.b0 * x0 + c.b1 * de_x(w, 0) - c.a1 * y0; y1 = c.b0 * x1 + c.b1 * de_x(w, 1) - c.a1 * y1;
                d[3 * i] = de_round(y0) | (de_round(y1) << 16);
            }
            d[3 * i + 2] &= ~0xFFu;                 /* emphasis: the stream is flat now */
        }
        key = k; w = w_own;
    }
    if (base + (size_t)first + (size_t)cnt == a.n && cnt > 0) {
        DeState o; o.key = key; o._pad = 0;
        const bool run = key != (uint32_t)DE_KEY_IDLE;
        o.x[0] = run ? de_x(w, 0) : 0.0; o.x[1] = run ? de_x(w, 1) : 0.0; o.y[0] = run ? y0 : 0.0; o.y[1] = run ? y1 : 0.0;
        *a.state = o;
    }
#pragma unroll
    for (int k = 0; k < DE_RUN; k++) lds.w[lane * DE_LDS_PITCH + k] = d[k];
    __syncthreads();
    for (int j0 = 0; j0 < DE_RUN; j0 += 16) {
#pragma unroll
        for (int j = 0; j < 16; j++) { const uint32_t g = (uint32_t)(j0 + j) * 64u + (uint32_t)lane; if (g < n_dw) dst[g] = lds.w[g + g / (uint32_t)DE_RUN]; }
    }
}

} // namespace sdva

__global__ void __launch_bounds__(64) sdv_k_deemph_warm(sdva::DeArgs a) { sdva::deemph_warm_body(a, blockIdx.x, (int)threadIdx.x); }
__global__ void __launch_bounds__(64) sdv_k_deemph(sdva::DeArgs a)
{
    __shared__ sdva::DeLds lds;
    sdva::deemph_body(a, blockIdx.x, lds, (int)threadIdx.x);
}
