/*
 * ingest_device.h - device side of sdv_ingest_frames (include/sdvpcm.h): packed capture formats -> the 8-bit luma plane the frame entries
 * read, with crop, channel pick and the integer 2x width doubling, for gfx950.  Included by engine.inc; compiled by hipcc into the product
 * and by g++ for the CPU tests (tests/emu).  The sample values are the header's integer formulas, not libswscale's.
 *
 * A pure streaming kernel: no LDS, no atomics, no wave collectives.
 *   - Work item = one 16-byte-aligned chunk of a destination row.  Slot c of a row whose first byte sits at address a covers the row bytes
 *     p0 .. p0 + 15, p0 = 16 c - (a & 15); (out_w + 30) / 16 slots cover a row at any alignment.  A slot that lies inside the row is written
 *     with one 16-byte store, the head and the tail of a row bytewise (ingest_bytes, which is also the plain statement of every format).
 *   - The source bytes of a chunk are one contiguous span of the source row (16 pixels, 8 with doubling).  It is read with one constant-size
 *     copy from a byte pointer, which the compiler lowers to the widest loads (gfx950 takes them at any address); v210 reads the whole
 *     16-byte groups the pixels can lie in, one group earlier where the last of them would leave the row.  Nothing outside the bytes of a
 *     row is read.  With doubling a chunk at an odd row offset (an odd destination address) splits pixel pairs: it goes the bytewise way.
 *   - The byte picks are shifts and masks on the loaded dwords with compile-time indices: the arrays below never leave the registers.
 *   - One flat index over (frame, row, slot), walked with a grid stride that the host hands over already split into (frames, rows, slots):
 *     a step is three additions with carry, no division, and no launch is sliced by rows.
 */
#pragma once
#include "../../include/sdvpcm.h"

namespace sdv {

/* format families: what the sample function of a kernel build is */
enum { ING_GRAY8 = 0, ING_UYVY = 1, ING_YUYV = 2, ING_V210 = 3, ING_GRAY10 = 4, ING_RGB3 = 5, ING_RGB4 = 6, ING_FAMILIES = 7 };

struct IngestArgs {
    const uint8_t *src; size_t src_row_stride, src_frame_stride;
    uint8_t *dst; size_t dst_row_stride, dst_frame_stride;
    int n_frames, out_w, out_h;         /* out_w: bytes of a destination row (twice the kept pixels when doubling) */
    int crop_left, crop_top;
    uint32_t src_row_bytes;             /* the bytes of a source row that belong to its src_width pixels: nothing behind them is read */
    int slots;                          /* chunk slots per destination row */
    int step_f, step_r, step_c;         /* the grid stride (threads of the launch) as frames, rows and slots */
    uint32_t wt[3];                     /* RGB families: weights of the pixel's bytes 0..2, sum 256 (one of them 256: that byte itself) */
};

template <int FAM, bool DBL> struct IngestShape {
    static constexpr int NPX = DBL ? 8 : 16;                                    /* source pixels of a chunk */
    static constexpr int BPP = FAM == ING_GRAY8 ? 1 : FAM == ING_RGB3 ? 3 : FAM == ING_RGB4 ? 4 : 2;
    static constexpr int NB = FAM == ING_V210 ? (DBL ? 48 : 64) : NPX * BPP;    /* bytes read: v210, the 3 / 4 groups 8 / 16 pixels can touch */
    static constexpr int NSMP = FAM == ING_V210 ? NB / 16 * 6 : NPX;            /* samples unpacked from them */
};

/* a weight, told to be small: the products are 24-bit multiply-adds */
__device__ __forceinline__ uint32_t ing_wt(const IngestArgs &a, int i) { return a.wt[i] & 0x1FFu; }

/* ---- one sample, bytewise: the contract of include/sdvpcm.h as it is written there ------------------------------------------- */
template <int FAM> __device__ inline uint32_t ingest_sample(const IngestArgs &a, const uint8_t *row, int x)
{
    if (FAM == ING_GRAY8) return row[x];
    if (FAM == ING_UYVY) return row[2 * (size_t)x + 1];
    if (FAM == ING_YUYV) return row[2 * (size_t)x];
    if (FAM == ING_GRAY10) return (((uint32_t)row[2 * (size_t)x] | (uint32_t)row[2 * (size_t)x + 1] << 8) & 0x3FFu) >> 2;
    if (FAM == ING_V210) {
        const int g = x / 6, c = 2 * (x % 6) + 1;
        const uint8_t *p = row + 16 * (size_t)g + 4 * (c / 3);
        const uint32_t w = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
        return ((w >> (10 * (c % 3))) & 0x3FFu) >> 2;
    }
    const uint8_t *p = row + (size_t)(FAM == ING_RGB3 ? 3 : 4) * (size_t)x;
    return (ing_wt(a, 0) * p[0] + ing_wt(a, 1) * p[1] + ing_wt(a, 2) * p[2] + 128u) >> 8;
}

/* bytes lo .. hi - 1 of a destination row (at most 16), a sample at a time: heads and tails of rows.  All loads first, then all stores: one
 * wait for memory, not one per byte. */
template <int FAM, bool DBL> __device__ inline void ingest_bytes(const IngestArgs &a, const uint8_t *srow, uint8_t *drow, int lo, int hi)
{
    uint32_t v[16];
#pragma unroll
    for (int i = 0; i < 16; i++) v[i] = lo + i < hi ? ingest_sample<FAM>(a, srow, a.crop_left + (DBL ? (lo + i) >> 1 : lo + i)) : 0;
#pragma unroll
    for (int i = 0; i < 16; i++) if (lo + i < hi) drow[lo + i] = (uint8_t)v[i];
}

/* ---- a chunk from registers ----------------------------------------------------------------------------------------------------- */
__device__ __forceinline__ uint32_t ing_byte(const uint32_t *w, int n) { return (w[n >> 2] >> (8 * (n & 3))) & 0xFFu; }
/* bits sh .. sh + 31 of hi:lo, sh in 0..31 */
__device__ __forceinline__ uint32_t ing_funnel(uint32_t lo, uint32_t hi, uint32_t sh) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh); }
/* the 16-bit pair (a, b) as the bytes a a b b */
__device__ __forceinline__ uint32_t ing_dup(uint32_t h) { return ((h & 0xFFu) | ((h & 0xFF00u) << 8)) * 0x0101u; }

/* sample i of the span in w (v210: luma i of the groups in w), i a constant once unrolled */
template <int FAM> __device__ __forceinline__ uint32_t ing_unpack(const IngestArgs &a, const uint32_t *w, int i)
{
    if (FAM == ING_GRAY8) return ing_byte(w, i);
    if (FAM == ING_UYVY) return ing_byte(w, 2 * i + 1);
    if (FAM == ING_YUYV) return ing_byte(w, 2 * i);
    if (FAM == ING_GRAY10) return (w[i >> 1] >> (16 * (i & 1) + 2)) & 0xFFu;                /* (v & 0x3FF) >> 2 */
    if (FAM == ING_V210) { const int c = 2 * (i % 6) + 1; return (w[4 * (i / 6) + c / 3] >> (10 * (c % 3) + 2)) & 0xFFu; }
    const int b = (FAM == ING_RGB3 ? 3 : 4) * i;
    return (ing_wt(a, 0) * ing_byte(w, b) + ing_wt(a, 1) * ing_byte(w, b + 1) + ing_wt(a, 2) * ing_byte(w, b + 2) + 128u) >> 8;
}

/* The chunk at `out` (16-byte aligned, inside its row) from the NB source bytes of its span, in w; `skip`: v210 only, the lumas in w in front of
 * the chunk's first pixel (0..10). */
template <int FAM, bool DBL> __device__ __forceinline__ void ingest_chunk(const IngestArgs &a, const uint32_t *w, uint32_t skip, uint8_t *out)
{
    typedef IngestShape<FAM, DBL> S;
    constexpr int NS = (S::NSMP + 3) / 4;
    uint32_t s[NS + 2];                             /* four samples a dword, two dwords of room for the shift below */
#pragma unroll
    for (int k = 0; k < NS; k++) {
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) if (4 * k + j < S::NSMP) v |= ing_unpack<FAM>(a, w, 4 * k + j) << (8 * j);
        s[k] = v;
    }
    s[NS] = s[NS + 1] = 0;
    constexpr int NP = DBL ? 2 : 4;                 /* the chunk's own samples: 8 (doubling) or 16 */
    uint32_t px[NP];
    if constexpr (FAM == ING_V210) {                /* drop `skip` bytes: whole dwords by a select, the rest by a funnel shift */
        const uint32_t q = skip >> 2, sh = 8 * (skip & 3);
#pragma unroll
        for (int k = 0; k < NP; k++)
            px[k] = ing_funnel(q == 0 ? s[k] : q == 1 ? s[k + 1] : s[k + 2], q == 0 ? s[k + 1] : q == 1 ? s[k + 2] : s[k + 3], sh);
    } else {
#pragma unroll
        for (int k = 0; k < NP; k++) px[k] = s[k];
    }
    uint4 v;
    if constexpr (DBL) { v.x = ing_dup(px[0]); v.y = ing_dup(px[0] >> 16); v.z = ing_dup(px[1]); v.w = ing_dup(px[1] >> 16); }
    else { v.x = px[0]; v.y = px[1]; v.z = px[2]; v.w = px[3]; }
    *reinterpret_cast<uint4 *>(out) = v;
}

/* One step of the flat index (frame f, row r, slot c, and the offsets of that row in the two buffers) by the launch's threads: a step of the
 * rows is step_f frames and step_r rows, one row more with a carry from the slots, and back by a frame's rows with a carry into the frames. */
struct IngestAt { int c, r, f; size_t s_at, d_at; };
__device__ __forceinline__ void ingest_step(const IngestArgs &a, IngestAt &i, size_t s_step, size_t s_wrap, size_t d_step, size_t d_wrap)
{
    i.c += a.step_c;
    const bool cc = i.c >= a.slots;
    if (cc) i.c -= a.slots;
    i.r += a.step_r + (cc ? 1 : 0);
    const bool cr = i.r >= a.out_h;
    if (cr) i.r -= a.out_h;
    i.f += a.step_f + (cr ? 1 : 0);
    i.s_at += s_step + (cc ? a.src_row_stride : 0) + (cr ? s_wrap : 0);
    i.d_at += d_step + (cc ? a.dst_row_stride : 0) + (cr ? d_wrap : 0);
}

/* thread t of a launch of step_f * out_h * slots + step_r * slots + step_c threads.  The row offsets move with the index: no multiplication in
 * the loop. */
template <int FAM, bool DBL> __device__ inline void ingest_body(const IngestArgs &a, uint32_t t)
{
    typedef IngestShape<FAM, DBL> S;
    IngestAt i;
    i.c = (int)(t % (uint32_t)a.slots);
    const uint32_t line = t / (uint32_t)a.slots;
    i.r = (int)(line % (uint32_t)a.out_h); i.f = (int)(line / (uint32_t)a.out_h);
    i.s_at = (size_t)i.f * a.src_frame_stride + (size_t)(a.crop_top + i.r) * a.src_row_stride;
    i.d_at = (size_t)i.f * a.dst_frame_stride + (size_t)i.r * a.dst_row_stride;
    const size_t s_step = (size_t)a.step_f * a.src_frame_stride + (size_t)a.step_r * a.src_row_stride, s_wrap = a.src_frame_stride - (size_t)a.out_h * a.src_row_stride;
    const size_t d_step = (size_t)a.step_f * a.dst_frame_stride + (size_t)a.step_r * a.dst_row_stride, d_wrap = a.dst_frame_stride - (size_t)a.out_h * a.dst_row_stride;
    for (; i.f < a.n_frames; ingest_step(a, i, s_step, s_wrap, d_step, d_wrap)) {
        const uint8_t *srow = a.src + i.s_at;
        uint8_t *drow = a.dst + i.d_at;
        const int p0 = 16 * i.c - (int)((uintptr_t)drow & 15);
        if (p0 >= a.out_w) continue;                /* the spare slot of a row */
        /* a whole chunk, of whole pixel pairs when doubling, in a row that is long enough for a span */
        if (p0 >= 0 && p0 + 16 <= a.out_w && !(DBL && (p0 & 1)) && a.src_row_bytes >= (uint32_t)S::NB) {
            const uint32_t x0 = (uint32_t)a.crop_left + (uint32_t)(DBL ? p0 >> 1 : p0), last_span = a.src_row_bytes - (uint32_t)S::NB;
            uint32_t at = FAM == ING_V210 ? 16 * (x0 / 6) : (uint32_t)S::BPP * x0, skip = FAM == ING_V210 ? x0 % 6 : 0;
            if (at > last_span) { skip += 6 * ((at - last_span) / 16); at = last_span; }       /* (v210 only: the last group is not there, one earlier) */
            uint32_t w[S::NB / 4];
            __builtin_memcpy(w, srow + at, S::NB);
            ingest_chunk<FAM, DBL>(a, w, skip, drow + p0);
        } else ingest_bytes<FAM, DBL>(a, srow, drow, p0 < 0 ? 0 : p0, p0 + 16 < a.out_w ? p0 + 16 : a.out_w);
    }
}

} // namespace sdv

#ifndef SDV_EMU
template <int FAM, bool DBL> __global__ void __launch_bounds__(256) sdv_k_ingest(sdv::IngestArgs a)
{
    sdv::ingest_body<FAM, DBL>(a, blockIdx.x * 256u + threadIdx.x);
}
#endif
