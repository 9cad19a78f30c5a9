/*
 * audio_resample_device.h - device side of sdv_audio_resample (include/sdvpcm.h): 44 056 Hz segments of the PCMSamplePair stream to
 * 44 100 Hz by the 1001 / 1000 polyphase filter, for gfx950.  Included by audio_device.h; compiled by hipcc into the product and by g++ on
 * the SIMT emulator for the CPU tests (tests/emu).  The reference has no such stage: the definition is the one in the header.
 *
 * A call works on the engine's history (the open segment's last 127 pairs, positions -127 .. -1) and its input (positions 0 .. n - 1) as one
 * array.  A pair is "through" (copied: a service pair or a pair of another rate) or belongs to a segment.  Every output has one owner among
 * the input pairs, so that counting outputs is a sum over pairs that needs nothing from behind the pair:
 *   - a through pair owns its copy;
 *   - pair j (counted from its segment's origin) owns the outputs m whose position m 1000 / 1001 lies in (j - 1, j]: m = j + floor(j / 1000),
 *     and also m - 1 where j is a multiple of 1000 other than 0.  (Owning by the pair at or behind the position rather than by x[i0] in
 *     front of it: a segment of n pairs then owns exactly its n_out outputs wherever it ends, and no count depends on where that is.)
 *     F(j) = j + floor((j - 1) / 1000) outputs are owned by the first j pairs of a segment.
 * Three launches:
 *   classify  one wave per tile of 1024 pairs: where the tile's first and last through pairs are and how many outputs the pairs from the
 *             first one on own (what lies in front of it belongs to a segment whose origin the tile cannot know);
 *   scan      one wave over the tile summaries, 64 per round, composed with shuffles: every tile's start - the origin of the segment it
 *             inherits and the output index of its first pair; then the call's result (count, the open segment's counters) and the new history;
 *   emit      one wave per tile: the tile's audio dwords with 128 pairs in front and 64 behind go to LDS (one dword per pair serves both channels),
 *             the through flags as a bitmap next to them.  Lane l of round r owns pair 64 r + l, so the 64 lanes of a round walk consecutive outputs,
 *             i.e. phases in descending order (m 1000 = -m mod 1001): the tap table is stored transposed, [k][phase], and a round's loads of tap k are
 *             one run of 64 doubles.  The 128-term sums run in double, k ascending.  The open segment's owing pairs (positions -64 .. -1) are tile 0's.
 * No atomics, no scratch; nothing is written that another wave of the same launch reads.
 */
#pragma once
#include <math.h>

namespace sdva {

enum { RS_TILE = 1024,                  /* pairs per tile; the tiles of a call start at its first pair (not part of the ABI: no output depends on it) */
       RS_HALF = SDV_RESAMPLE_HALF, RS_TAPS = 2 * SDV_RESAMPLE_HALF, RS_HIST = RS_TAPS - 1,
       RS_PHASES = SDV_RESAMPLE_L, RS_PITCH = 1024,             /* doubles per row of the transposed table */
       RS_FRONT = 2 * RS_HALF, RS_STAGE = RS_FRONT + RS_TILE + RS_HALF, RS_WORDS = RS_STAGE / 64 + 1 };
static_assert(RS_TILE % 64 == 0 && RS_STAGE % 64 == 0 && SDV_RESAMPLE_L == SDV_RESAMPLE_M + 1, "the geometry include/sdvpcm.h documents");
#define RS_NONE 0xFFFFFFFFu

/* What a run of pairs [start, end) says to the scan: its first and last through pairs (RS_NONE: none) and the outputs owned from the first one on. */
struct RsSum { uint32_t first, last, rest, _pad; };
/* A tile's start: the origin of the segment it inherits (at or in front of the tile, negative in the history) and the output index of its first pair. */
struct RsStart { int64_t origin, out; };
struct RsResult { uint64_t n_out, seen, emitted; };             /* of the call; of the open segment behind it */
struct RsArgs {
    const sdv_sample_pair *in; sdv_sample_pair *out; int64_t n; uint64_t out_cap;
    const sdv_sample_pair *hist; sdv_sample_pair *hist_out;     /* RS_HIST pairs, the last one at RS_HIST - 1 */
    const double *taps;                                         /* [RS_TAPS][RS_PITCH] */
    RsSum *sums; RsStart *starts; RsResult *result;
    uint64_t seen0, emitted0;                                   /* the open segment in front of the call: pairs seen, outputs emitted */
    uint32_t n_tiles; int flush;
};
struct RsLds { uint32_t x[RS_STAGE]; uint64_t through[RS_WORDS]; };

__device__ __forceinline__ int64_t rs_owned(int64_t j) { return j <= 0 ? 0 : j + (j - 1) / 1000; }             /* F */
__device__ __forceinline__ bool rs_through(uint32_t d1, uint32_t d2) { return ((d2 >> 8) & 0xFFu) != 0u || (d1 >> 16) != 44056u; }
__device__ __forceinline__ uint64_t rs_ballot(bool p) { return (uint64_t)__ballot(p); }
__device__ __forceinline__ int rs_low(uint64_t m) { return __ffsll((unsigned long long)m) - 1; }
__device__ __forceinline__ int rs_high(uint64_t m) { return 63 - __clzll((unsigned long long)m); }

/* ---- classify ------------------------------------------------------------------------------------------------------------ */
__device__ inline void resample_classify_body(const RsArgs &a, uint32_t tile, int lane)
{
    const int64_t base = (int64_t)tile * RS_TILE, end = a.n - base < (int64_t)RS_TILE ? a.n : base + RS_TILE;
    const uint32_t *src = (const uint32_t *)a.in;
    RsSum s; s.first = RS_NONE; s.last = RS_NONE; s.rest = 0; s._pad = 0;
    for (int g = 0; g < RS_TILE / 64; g++) {
        const int64_t g0 = base + 64 * g, i = g0 + lane;
        if (g0 >= end) break;                                   /* (the same for every lane) */
        bool thr = false;
        if (i < end) thr = rs_through(src[3 * i + 1], src[3 * i + 2]);
        const uint64_t m = rs_ballot(thr);
        const int64_t g1 = g0 + 64 < end ? g0 + 64 : end;
        if (m == 0) {
            if (s.first != RS_NONE) s.rest += (uint32_t)(rs_owned(g1 - ((int64_t)s.last + 1)) - rs_owned(g0 - ((int64_t)s.last + 1)));
            continue;
        }
        const int64_t f = g0 + rs_low(m);
        if (s.first == RS_NONE) s.first = (uint32_t)f;
        else s.rest += (uint32_t)(rs_owned(f - ((int64_t)s.last + 1)) - rs_owned(g0 - ((int64_t)s.last + 1)));
        s.rest += (uint32_t)(g1 - f);                           /* from f on the group's pairs own one output each: the segments among them are shorter than 64 */
        s.last = (uint32_t)(g0 + rs_high(m));
    }
    if (lane == 0) a.sums[tile] = s;
}

/* ---- scan ---------------------------------------------------------------------------------------------------------------- */
struct RsRun { uint32_t start, end, first, last, rest; };      /* a summary with the pairs it covers */
__device__ __forceinline__ RsRun rs_join(const RsRun &p, const RsRun &q)      /* p, then q */
{
    RsRun r; r.start = p.start; r.end = q.end;
    if (p.first == RS_NONE) { r.first = q.first; r.last = q.last; r.rest = q.rest; return r; }
    const int64_t o = (int64_t)p.last + 1;
    r.first = p.first;
    if (q.first == RS_NONE) { r.last = p.last; r.rest = p.rest + (uint32_t)(rs_owned((int64_t)q.end - o) - rs_owned((int64_t)q.start - o)); }
    else { r.last = q.last; r.rest = p.rest + (uint32_t)(rs_owned((int64_t)q.first - o) - rs_owned((int64_t)q.start - o)) + q.rest; }
    return r;
}
__device__ __forceinline__ RsStart rs_apply(RsStart s, const RsRun &r)
{
    if (r.first == RS_NONE) { s.out += rs_owned((int64_t)r.end - s.origin) - rs_owned((int64_t)r.start - s.origin); return s; }
    s.out += rs_owned((int64_t)r.first - s.origin) - rs_owned((int64_t)r.start - s.origin) + (int64_t)r.rest;
    s.origin = (int64_t)r.last + 1;
    return s;
}
__device__ __forceinline__ RsRun rs_pull(const RsRun &r, int src)
{
    RsRun o; o.start = a_shfl(r.start, src); o.end = a_shfl(r.end, src); o.first = a_shfl(r.first, src); o.last = a_shfl(r.last, src); o.rest = a_shfl(r.rest, src);
    return o;
}
__device__ __forceinline__ sdv_sample_pair rs_pair(const RsArgs &a, int64_t i)      /* position i of history + input (i >= -RS_HIST) */
{
    return i < 0 ? a.hist[RS_HIST + i] : a.in[i];
}
__device__ inline void resample_scan_body(const RsArgs &a, int lane)
{
    RsStart carry; carry.origin = -(int64_t)a.seen0; carry.out = rs_owned((int64_t)a.seen0) - (int64_t)a.emitted0;
    const uint32_t n32 = (uint32_t)a.n;
    for (uint32_t t0 = 0; t0 < a.n_tiles; t0 += 64) {
        const uint32_t t = t0 + (uint32_t)lane;
        RsRun r; r.start = r.end = n32; r.first = r.last = RS_NONE; r.rest = 0;         /* behind the last tile: nothing */
        if (t < a.n_tiles) {
            const RsSum s = a.sums[t];
            r.start = t * (uint32_t)RS_TILE; r.end = n32 - r.start < (uint32_t)RS_TILE ? n32 : r.start + (uint32_t)RS_TILE;
            r.first = s.first; r.last = s.last; r.rest = s.rest;
        }
        for (int d = 1; d < 64; d <<= 1) {                      /* inclusive: the runs from lane 0 up to this lane */
            const RsRun p = rs_pull(r, lane >= d ? lane - d : lane);
            if (lane >= d) r = rs_join(p, r);
        }
        const RsRun before = rs_pull(r, lane > 0 ? lane - 1 : 0), all = rs_pull(r, 63);
        if (t < a.n_tiles) a.starts[t] = lane > 0 ? rs_apply(carry, before) : carry;
        carry = rs_apply(carry, all);
    }
    /* behind the last pair: the segment that is open there (none when the last pair went through, or with flush) */
    const int64_t seen = a.n - carry.origin;
    const bool open = seen > 0 && !a.flush;
    const int64_t ready = seen > RS_HALF ? ((seen - RS_HALF) * SDV_RESAMPLE_L + SDV_RESAMPLE_M - 1) / SDV_RESAMPLE_M : 0;         /* outputs whose i0 + 64 < seen */
    if (lane == 0) {
        RsResult res;
        res.n_out = (uint64_t)(open ? carry.out - rs_owned(seen) + ready : carry.out);
        res.seen = open ? (uint64_t)seen : 0u; res.emitted = open ? (uint64_t)ready : 0u;
        *a.result = res;
    }
    if (open)
        for (int k = lane; k < RS_HIST; k += 64) {
            const int64_t i = a.n - RS_HIST + k;
            if (i >= -(int64_t)RS_HIST && i >= carry.origin) a.hist_out[k] = rs_pair(a, i);
        }
}

/* ---- emit ---------------------------------------------------------------------------------------------------------------- */
__device__ __forceinline__ uint32_t rs_round(double y)
{
    double r = rint(y);                 /* half to even */
    r = r < -32768.0 ? -32768.0 : r > 32767.0 ? 32767.0 : r;
    return (uint32_t)(uint16_t)(int16_t)(int)r;
}
/* Output m of the segment with origin `origin` (a position) whose output 0 has index `seg_out`.  w0: the position of lds.x[0]. */
__device__ inline void rs_emit_output(const RsArgs &a, const RsLds &lds, int64_t origin, int64_t seg_out, uint64_t m, int64_t w0)
{
    const uint64_t t = m * (uint64_t)SDV_RESAMPLE_M, i0 = t / (uint64_t)SDV_RESAMPLE_L;
    const uint32_t p = (uint32_t)(t - i0 * (uint64_t)SDV_RESAMPLE_L);
    const int64_t at = origin + (int64_t)i0;                    /* the position of x[i0] */
    /* where the segment ends: the first through pair among the 64 positions behind x[i0], else the end of the call */
    const int b = (int)(at + 1 - w0), sh = b & 63;
    const uint64_t win = (lds.through[b >> 6] >> sh) | (sh ? lds.through[(b >> 6) + 1] << (64 - sh) : 0ull);
    int64_t end = win ? at + 1 + rs_low(win) : at + RS_HALF + 1;
    if (!win && at + RS_HALF >= a.n) {
        if (!a.flush) return;                                   /* the open segment has not seen x[i0 + 64] yet: the output waits */
        end = a.n;
    }
    const int base = (int)(at - (RS_HALF - 1) - w0);
    const int lo = origin > at - (RS_HALF - 1) ? (int)(origin - w0) : base, hi = (int)(end - 1 - w0);
    const double *h = a.taps + p;
    double y0 = 0.0, y1 = 0.0;
#pragma unroll 8
    for (int k = 0; k < RS_TAPS; k++) {
        int idx = base + k; idx = idx < lo ? lo : idx; idx = idx > hi ? hi : idx;
        const uint32_t w = lds.x[idx];
        const double c = h[(size_t)k * RS_PITCH];
        y0 += c * (double)(int16_t)(uint16_t)(w & 0xFFFFu); y1 += c * (double)(int16_t)(uint16_t)(w >> 16);
    }
    const int64_t dst = seg_out + (int64_t)m;
    if (dst < 0 || (uint64_t)dst >= a.out_cap) return;          /* (never: sdv_audio_resample_room) */
    const uint32_t *src = at < 0 ? (const uint32_t *)(a.hist + (RS_HIST + at)) : (const uint32_t *)(a.in + at);
    uint32_t *o = (uint32_t *)(a.out + dst);
    o[0] = rs_round(y0) | (rs_round(y1) << 16);
    o[1] = (src[1] & 0xFFFFu) | (44100u << 16);
    o[2] = src[2];
}
/* The outputs pair j of a segment owns; m_from: outputs of the segment below it were emitted by earlier calls. */
__device__ __forceinline__ void rs_emit_owned(const RsArgs &a, const RsLds &lds, int64_t origin, int64_t seg_out, int64_t j, uint64_t m_from, int64_t w0)
{
    const uint64_t m = (uint64_t)(j + j / 1000);
    if (j > 0 && j % 1000 == 0 && m - 1 >= m_from) rs_emit_output(a, lds, origin, seg_out, m - 1, w0);
    if (m >= m_from) rs_emit_output(a, lds, origin, seg_out, m, w0);
}
__device__ inline void resample_emit_body(const RsArgs &a, uint32_t tile, RsLds &lds, int lane)
{
    const int64_t base = (int64_t)tile * RS_TILE, end = a.n - base < (int64_t)RS_TILE ? a.n : base + RS_TILE, w0 = base - RS_FRONT;
    const int64_t origin0 = -(int64_t)a.seen0, first_pos = a.seen0 < (uint64_t)RS_HIST ? origin0 : -(int64_t)RS_HIST;
    /* the audio dwords of positions w0 .. w0 + RS_STAGE - 1 and their through flags */
    for (int r = 0; r < RS_STAGE / 64; r++) {
        const int64_t i = w0 + 64 * r + lane;
        uint32_t d0 = 0; bool thr = false;
        if (i >= first_pos && i < a.n) {
            const uint32_t *src = i < 0 ? (const uint32_t *)(a.hist + (RS_HIST + i)) : (const uint32_t *)(a.in + i);
            d0 = src[0];
            thr = i >= 0 && rs_through(src[1], src[2]);
        }
        lds.x[64 * r + lane] = d0;
        const uint64_t m = rs_ballot(thr);
        if (lane == 0) lds.through[r] = m;
    }
    if (lane == 0) lds.through[RS_WORDS - 1] = 0;
    __syncthreads();
    RsStart run; run.origin = origin0; run.out = rs_owned((int64_t)a.seen0) - (int64_t)a.emitted0;
    if (a.n_tiles > 0) run = a.starts[tile];
    if (tile == 0 && a.seen0 > 0) {
        /* the pairs of the open segment that still owe outputs */
        const int64_t i = -(int64_t)RS_HALF + lane;
        if (i >= origin0) rs_emit_owned(a, lds, origin0, -(int64_t)a.emitted0, i - origin0, a.emitted0, w0);
    }
    for (int g = 0; g < RS_TILE / 64; g++) {
        const int64_t g0 = base + 64 * g, i = g0 + lane;
        if (g0 >= end) break;                                   /* (the same for every lane) */
        const int64_t g1 = g0 + 64 < end ? g0 + 64 : end;
        const uint64_t m = lds.through[RS_FRONT / 64 + g];
        const int64_t lead = run.out - rs_owned(g0 - run.origin);        /* the index of output 0 of the inherited segment */
        const int64_t f = m ? g0 + rs_low(m) : g1;                          /* the inherited segment's pairs in this group end here */
        const int64_t at_f = lead + rs_owned(f - run.origin);               /* the output index of pair f */
        if (i < end) {
            const uint64_t below = m & ((1ull << lane) - 1ull);
            if ((m >> lane) & 1ull) {
                const uint32_t *src = (const uint32_t *)(a.in + i); const int64_t dst = at_f + (i - f);
                if (dst >= 0 && (uint64_t)dst < a.out_cap) { uint32_t *o = (uint32_t *)(a.out + dst); o[0] = src[0]; o[1] = src[1]; o[2] = src[2]; }
            } else if (below == 0) rs_emit_owned(a, lds, run.origin, lead, i - run.origin, run.origin == origin0 ? a.emitted0 : 0u, w0);
            else {
                const int64_t o = g0 + rs_high(below) + 1;                  /* a segment that starts inside the group */
                rs_emit_owned(a, lds, o, at_f + (o - f), i - o, 0u, w0);
            }
        }
        if (m) { run.out = at_f + (g1 - f); run.origin = g0 + rs_high(m) + 1; }
        else run.out = lead + rs_owned(g1 - run.origin);
    }
}

} // namespace sdva

__global__ void __launch_bounds__(64) sdv_k_resample_classify(sdva::RsArgs a) { sdva::resample_classify_body(a, blockIdx.x, (int)threadIdx.x); }
__global__ void __launch_bounds__(64) sdv_k_resample_scan(sdva::RsArgs a) { sdva::resample_scan_body(a, (int)threadIdx.x); }
__global__ void __launch_bounds__(64) sdv_k_resample_emit(sdva::RsArgs a)
{
    __shared__ sdva::RsLds lds;
    sdva::resample_emit_body(a, blockIdx.x, lds, (int)threadIdx.x);
}
