/*
 * audio_skew_device.h - device side of the skew stage of sdv_audio_resample (include/sdvpcm.h, SDV_RESAMPLE_DELAY_RIGHT / _LEFT): one channel
 * of the PCMSamplePair stream delayed by half a sampling period, for gfx950.  Included by audio_device.h behind audio_resample_device.h (whose
 * small helpers it uses); compiled by hipcc into the product and by g++ on the SIMT emulator for the CPU tests (tests/emu).  The reference has
 * no such stage: the definition is the one in the header.
 *
 * A call works on the engine's history (the last 127 pairs the stage has seen, positions -127 .. -1; those of the open segment count) and its
 * input (positions 0 .. n - 1) as one array.  Every input pair yields exactly one output pair, in order, so the output index of position i is
 * the number of pairs that waited in front of the call plus i: there is nothing to count and nothing to scan.  What an output needs to know is
 * where its segment begins and ends among the 64 pairs in front of it and the 63 behind it, and a bitmap of segment boundaries says that:
 * bit q is set where no segment runs from pair q - 1 into pair q (a service pair on either side, another sample_rate, the origin of the open
 * segment, the end of a call made with flush).
 * One launch, one wave per tile of 1024 pairs: the words of the delayed channel over the tile with 128 pairs in front (tile 0 also emits what waited, and
 * that reaches back to -127) and 64 behind go to LDS once, as doubles, the boundary bitmap next to them.  One lane computes one output: 128 multiply-adds
 * in double, k ascending; tap k is the same for every lane, and a wave none of whose lanes has a boundary in reach reads its inputs without clamps.  When the stage follows the resampler it reads the count of its input from
 * the resampler's result in device memory, and the waves of tiles behind that count leave at once.  The wave of tile 0 also writes the call's
 * result and the new history.  No atomics, no scratch; nothing is written that another wave of the same launch reads.
 */
#pragma once
#include <math.h>

namespace sdva {

enum { SK_TILE = 1024,                  /* pairs per tile (not part of the ABI: no output depends on it) */
       SK_HALF = 64, SK_TAPS = 128, SK_HIST = SK_TAPS - 1, SK_WAIT = SK_HALF - 1,
       SK_MANY = SK_HIST + 1,           /* "the open segment has seen more than the history holds": all the stage needs to know beyond 127 */
       SK_FRONT = 2 * SK_HALF, SK_STAGE = SK_FRONT + SK_TILE + SK_HALF, SK_WORDS = SK_STAGE / 64 + 1 };
static_assert(SK_TILE % 64 == 0 && SK_STAGE % 64 == 0 && SK_HALF == SDV_RESAMPLE_HALF, "the geometry include/sdvpcm.h documents");
#define SK_KEY_SERVICE 0x10000u         /* what a pair is to its neighbours: a service pair, or its sample_rate */
#define SK_KEY_OUTSIDE 0x20000u         /* no pair: in front of the history, behind the input */

struct SkResult { uint64_t n_out; uint32_t seen, _pad; RsResult a; };      /* of the call; of the open segment behind it; the resampler's result, passed on */
struct SkArgs {
    const sdv_sample_pair *in; sdv_sample_pair *out; int64_t n; uint64_t out_cap;
    const RsResult *a_result;                                   /* not null: the input is the resampler's output, its n_out pairs (n: the room of `in`) */
    const sdv_sample_pair *hist; sdv_sample_pair *hist_out;     /* SK_HIST pairs, the last one at SK_HIST - 1 */
    const double *taps;                                         /* [SK_TAPS] */
    SkResult *result;
    uint32_t seen0;                                             /* the open segment in front of the call: pairs seen, SK_MANY for more than SK_HIST */
    int flush, channel;                                         /* channel: the delayed one, 0 left, 1 right */
};
struct SkLds { double x[SK_STAGE]; uint64_t bnd[SK_WORDS]; };            /* the words of the delayed channel, as doubles; the boundary bits */

__device__ __forceinline__ const uint32_t *sk_src(const SkArgs &a, int64_t i)      /* position i of history + input */
{
    return i < 0 ? (const uint32_t *)(a.hist + (SK_HIST + i)) : (const uint32_t *)(a.in + i);
}
__device__ __forceinline__ uint32_t sk_key(uint32_t d1, uint32_t d2) { return ((d2 >> 8) & 0xFFu) != 0u ? SK_KEY_SERVICE : d1 >> 16; }
__device__ __forceinline__ uint32_t sk_key_at(const SkArgs &a, int64_t i, int64_t first, int64_t n)
{
    if (i < first || i >= n) return SK_KEY_OUTSIDE;
    const uint32_t *s = sk_src(a, i);
    return sk_key(s[1], s[2]);
}
/* Does no segment run from position i - 1 (key `prev`) into position i (key `key`)?  first: the first position the history holds. */
__device__ __forceinline__ bool sk_boundary(const SkArgs &a, uint32_t prev, uint32_t key, int64_t i, int64_t first, int64_t n)
{
    if (i >= n) return i == n && a.flush != 0;
    if (i < first) return false;
    if (i == first && a.seen0 > (uint32_t)SK_HIST) return false;        /* the open segment began in front of the history */
    return key == SK_KEY_SERVICE || key != prev;
}
__device__ __forceinline__ uint64_t sk_bits(const SkLds &lds, int b)    /* the 64 boundary bits from bit b on */
{
    const int sh = b & 63;
    return (lds.bnd[b >> 6] >> sh) | (sh ? lds.bnd[(b >> 6) + 1] << (64 - sh) : 0ull);
}

/* The output of position i (its index: wait0 + i), for the lanes that have one (`active`); every lane of the wave comes here.  w0: the position of
 * lds.x[0].  Where no lane of the wave has a boundary in its reach - nearly always - the wave takes the loop without clamps: a tap is one LDS read at a
 * constant offset and one multiply-add.  The sums are the same ones in both loops, k ascending. */
__device__ inline void sk_emit(const SkArgs &a, const SkLds &lds, bool active, int64_t i, int64_t w0, int64_t n, int64_t wait0)
{
    uint32_t d0 = 0, d1 = 0, d2 = 0;
    int at = SK_HALF, lo = 0, hi = 2 * SK_HALF - 1;
    bool sum = false;
    if (active) {
        const uint32_t *src = sk_src(a, i);
        d0 = src[0]; d1 = src[1]; d2 = src[2];
        at = (int)(i - w0);
        if (sk_key(d1, d2) != SK_KEY_SERVICE) {
            /* the segment: from the last boundary among the 64 positions up to this one, to the first one among the 63 behind it */
            const uint64_t back = sk_bits(lds, at - (SK_HALF - 1)), ahead = sk_bits(lds, at + 1) & 0x7FFFFFFFFFFFFFFFull;
            lo = back ? at - (SK_HALF - 1) + rs_high(back) : at - SK_HALF;
            hi = ahead ? at + rs_low(ahead) : at + SK_WAIT;
            sum = true;
            if (!ahead && i + SK_WAIT >= n) { sum = false; active = false; }       /* the open segment has not seen z[m + 63] yet: the output waits */
        }
    }
    const int base = at - SK_HALF;
    const bool clamps = sum && (lo != base || hi != at + SK_WAIT);
    const double *h = a.taps;
    double y = 0.0;
    if (rs_ballot(clamps) == 0ull) {
        if (sum) {
            const double *x = lds.x + base;
#pragma unroll 16
            for (int k = 0; k < SK_TAPS; k++) y += h[k] * x[k];
        }
    } else if (sum) {
#pragma unroll 8
        for (int k = 0; k < SK_TAPS; k++) {
            int idx = base + k; idx = idx < lo ? lo : idx; idx = idx > hi ? hi : idx;
            y += h[k] * lds.x[idx];
        }
    }
    if (!active) return;
    if (sum) d0 = a.channel ? (d0 & 0x0000FFFFu) | (rs_round(y) << 16) : (d0 & 0xFFFF0000u) | rs_round(y);
    const int64_t dst = wait0 + i;
    if (dst < 0 || (uint64_t)dst >= a.out_cap) return;          /* (never: sdv_audio_resample_room) */
    uint32_t *o = (uint32_t *)(a.out + dst);
    o[0] = d0; o[1] = d1; o[2] = d2;
}

__device__ inline void skew_body(const SkArgs &a, uint32_t tile, SkLds &lds, int lane)
{
    const int64_t n = a.a_result && a.a_result->n_out < (uint64_t)a.n ? (int64_t)a.a_result->n_out : a.n;
    const int64_t base = (int64_t)tile * SK_TILE;
    if (tile > 0 && base >= n) return;                          /* (the same for every lane) a tile behind what the resampler put out */
    const int64_t end = n - base < (int64_t)SK_TILE ? n : base + SK_TILE, w0 = base - SK_FRONT;
    const int64_t first = -(int64_t)(a.seen0 < (uint32_t)SK_HIST ? a.seen0 : (uint32_t)SK_HIST);
    const int64_t wait0 = (int64_t)(a.seen0 < (uint32_t)SK_WAIT ? a.seen0 : (uint32_t)SK_WAIT);
    /* the words of the delayed channel at positions w0 .. w0 + SK_STAGE - 1, converted once, and the boundary bits */
    const int shift = a.channel ? 16 : 0;
    uint32_t carry = sk_key_at(a, w0 - 1, first, n);
    for (int r = 0; r < SK_STAGE / 64; r++) {
        const int64_t i = w0 + 64 * r + lane;
        uint32_t d0 = 0, key = SK_KEY_OUTSIDE;
        if (i >= first && i < n) { const uint32_t *s = sk_src(a, i); d0 = s[0]; key = sk_key(s[1], s[2]); }
        const uint32_t up = a_shfl(key, lane > 0 ? lane - 1 : 0);
        const uint32_t prev = lane > 0 ? up : carry;
        carry = a_shfl(key, 63);
        lds.x[64 * r + lane] = (double)(int16_t)(uint16_t)((d0 >> shift) & 0xFFFFu);
        const uint64_t m = rs_ballot(sk_boundary(a, prev, key, i, first, n));
        if (lane == 0) lds.bnd[r] = m;
    }
    if (lane == 0) lds.bnd[SK_WORDS - 1] = 0;
    __syncthreads();
    if (tile == 0 && wait0 > 0) {
        /* the pairs of the open segment that still owe their outputs */
        const int64_t i = -(int64_t)SK_HALF + lane;
        sk_emit(a, lds, i >= -wait0, i, w0, n, wait0);
    }
    for (int g = 0; g < SK_TILE / 64; g++) {
        const int64_t g0 = base + 64 * g, i = g0 + lane;
        if (g0 >= end) break;                                   /* (the same for every lane) */
        sk_emit(a, lds, i < end, i, w0, n, wait0);
    }
    if (tile != 0) return;
    /* behind the last pair: the segment that is open there (none behind a service pair, or with flush), and the new history */
    bool found = false; int64_t last = 0;
    for (int r = 0; r < (SK_HIST + 63) / 64; r++) {
        const int k = 64 * r + lane;
        const int64_t i = n - SK_HIST + k;
        bool b = false;
        if (k < SK_HIST && i >= first) {
            b = sk_boundary(a, sk_key_at(a, i - 1, first, n), sk_key_at(a, i, first, n), i, first, n);
            const uint32_t *s = sk_src(a, i);
            uint32_t *o = (uint32_t *)(a.hist_out + k);
            o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
        }
        const uint64_t m = rs_ballot(b);
        if (m) { found = true; last = n - SK_HIST + 64 * r + rs_high(m); }
    }
    if (lane == 0) {
        const uint32_t tail = sk_key_at(a, n - 1, first, n);
        const bool open = !a.flush && tail != SK_KEY_SERVICE && tail != SK_KEY_OUTSIDE;
        SkResult res;
        res.seen = !open ? 0u : found ? (uint32_t)(n - last) : (uint32_t)SK_MANY;
        res.n_out = (uint64_t)(wait0 + n - (int64_t)(res.seen < (uint32_t)SK_WAIT ? res.seen : (uint32_t)SK_WAIT));
        res._pad = 0;
        if (a.a_result) res.a = *a.a_result; else { res.a.n_out = 0; res.a.seen = 0; res.a.emitted = 0; }
        *a.result = res;
    }
}

} // namespace sdva

__global__ void __launch_bounds__(64) sdv_k_skew(sdva::SkArgs a)
{
    __shared__ sdva::SkLds lds;
    sdva::skew_body(a, blockIdx.x, lds, (int)threadIdx.x);
}
