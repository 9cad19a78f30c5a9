/*
 * encode_packed_device.h - the raster of the encoders (sdv_encode_frames, sdv_encode_markerless_frames, include/sdvpcm.h) for every out_fmt but
 * SDV_PIX_GRAY8: the rows leave the kernel as UYVY / YUY2, v210, a 10-bit plane or RGB / BGR with 3 or 4 bytes a pixel, for gfx950.  Included by
 * engine.inc behind encode_device.h, whose words step, cell table, line records, lookup (enc_four_win / enc_four_plain, `narrow`), levels and flat
 * (frame, row, slot) index it uses as they are; compiled by hipcc into the product and by g++ for the CPU tests (tests/emu).  SDV_PIX_GRAY8 stays
 * with sdv_k_encode_raster.  The packing is what sdv_ingest_frames unpacks (ingest_device.h), with neutral chroma and an opaque fourth byte.
 *
 * Write only, no LDS, no atomics, no wave collectives.
 *   - Work item = a unit of 16 consecutive pixels counted from the row's START (v210: 12 pixels, two groups, since 16 is no multiple of 6): slot c of a
 *     row is the pixels 16 c .. 16 c + 15 and the row bytes NB c .. NB c + NB - 1, NB = 32 (4:2:2, 10-bit plane, v210), 48 (3 bytes a pixel) or 64
 *     (4 bytes a pixel).  ceil(width / 16) slots cover a row (whole quads of them in the 48- and 64-byte builds, below).  The flat index and its
 *     grid stride are encode_device.h's.
 *   - The 16 levels of a unit are made exactly as sdv_k_encode_raster makes a chunk's: one 16-byte load of table entries (the table's room behind
 *     the row covers the last unit), the 8 record bytes the first entry lies in, a shift per pixel; `narrow` windows pixel by pixel.  Pixels of
 *     the unit at or behind `width` - the second half of the last pair of an odd width, the rest of the last v210 group - become `black`.
 *   - Expansion: shifts, masks and ORs on the four dwords of levels with compile-time indices, the reverse of ingest_chunk; nothing leaves the
 *     registers.
 *   - Stores: WIDE STORES AT THE ROW'S OWN ALIGNMENT.  A unit whose NB bytes lie inside the row's *row_bytes is stored with one constant-size copy
 *     to a byte pointer, which the compiler lowers to 16-byte stores (gfx950 takes them at any address); a row that starts on a 16-byte boundary
 *     with a stride that keeps it there - the fast case - gets aligned ones, any other row the same instructions at its own addresses.  Units
 *     count from the row's start, so a row has no head, and only its last unit can be a tail: that one alone stores the bytes below *row_bytes one
 *     by one.  The lanes of a wave part for nothing else.
 *   - The builds with 48 and 64 bytes a unit do not let a lane store its own unit: four neighbouring lanes share their four units, and each stores
 *     every fourth piece of 16 bytes of the 192 or 256 they make, so that a store instruction writes runs of 64 consecutive bytes
 *     (encode_packed_quad_body says how, and why).  The same table, records, lookup, levels, index and stores at the row's own alignment.
 */
#pragma once
#include "encode_device.h"

namespace sdv {

/* format families: what the expansion of a kernel build is (RGB and BGR write the same bytes) */
enum { ENCP_UYVY = 0, ENCP_YUYV = 1, ENCP_V210 = 2, ENCP_GRAY10 = 3, ENCP_RGB3 = 4, ENCP_RGB4 = 5, ENCP_FAMILIES = 6 };

template <int FAM> struct EncodePackedShape {
    static constexpr int NPX = FAM == ENCP_V210 ? 12 : 16;                      /* pixels of a unit */
    static constexpr int NB = FAM == ENCP_RGB3 ? 48 : FAM == ENCP_RGB4 ? 64 : 32;       /* bytes of a unit */
    static constexpr int NV = (NPX + 3) / 4;                                    /* dwords of levels */
    static constexpr bool QUAD = NB > 32;                                       /* four lanes share four units (encode_packed_quad_body) */
    /* slots of a row of w pixels: its units, for the quads whole quads */
    static constexpr int slots(int w) { return QUAD ? 4 * ((w + 4 * NPX - 1) / (4 * NPX)) : (w + NPX - 1) / NPX; }
};
enum { ENCP_QUAD_PX = 64 };             /* the pixels the lanes of a quad share: the window of a lane's lookup has to hold the cells of that many */

struct EncodePackedArgs {
    EncodeRasterArgs r;                 /* as for sdv_k_encode_raster; slots: units per row */
    uint32_t row_bytes;                 /* the bytes of a row (*row_bytes of the geometry calls): nothing behind them is written */
    int narrow_quad;                    /* the `narrow` of the quad builds: the entries of ENCP_QUAD_PX neighbouring pixels can lie more than 31 apart */
};

/* luma n of the levels in v, n a constant once unrolled */
__device__ __forceinline__ uint32_t encp_byte(const uint32_t *v, int n) { return (v[n >> 2] >> (8 * (n & 3))) & 0xFFu; }
/* y as y y y 0 */
__device__ __forceinline__ uint32_t encp_three(uint32_t y) { return y | (y << 8) | (y << 16); }

/* the 32 bytes of a unit from its levels, four pixels a dword (4:2:2, 10-bit plane, v210) */
template <int FAM> __device__ __forceinline__ void encp_expand(const uint32_t *v, uint32_t *o)
{
    if constexpr (FAM == ENCP_UYVY || FAM == ENCP_YUYV || FAM == ENCP_GRAY10) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t d = v[k];
            const uint32_t lo = (d & 0xFFu) | ((d & 0xFF00u) << 8), hi = ((d >> 16) & 0xFFu) | ((d >> 8) & 0xFF0000u);     /* two lumas, at the bytes 0 and 2 */
            if (FAM == ENCP_UYVY) { o[2 * k] = (lo << 8) | 0x00800080u; o[2 * k + 1] = (hi << 8) | 0x00800080u; }       /* 128 y 128 y */
            else if (FAM == ENCP_YUYV) { o[2 * k] = lo | 0x80008000u; o[2 * k + 1] = hi | 0x80008000u; }                /* y 128 y 128 */
            else { o[2 * k] = lo << 2; o[2 * k + 1] = hi << 2; }                                                        /* 16-bit y << 2 */
        }
    } else {                                        /* v210: luma j of a group is component 2 j + 1, at bits 10 (c % 3) of word c / 3; chroma 512 */
#pragma unroll
        for (int g = 0; g < 2; g++) {
            o[4 * g] = 0x20000200u | (encp_byte(v, 6 * g) << 12);
            o[4 * g + 1] = (encp_byte(v, 6 * g + 1) << 2) | 0x00080000u | (encp_byte(v, 6 * g + 2) << 22);
            o[4 * g + 2] = 0x20000200u | (encp_byte(v, 6 * g + 3) << 12);
            o[4 * g + 3] = (encp_byte(v, 6 * g + 4) << 2) | 0x00080000u | (encp_byte(v, 6 * g + 5) << 22);
        }
    }
}

/* thread t of a launch of step_f * height * slots + step_r * slots + step_c threads: the builds with 32 bytes a unit */
template <int FAM> __device__ inline void encode_packed_unit_body(const EncodePackedArgs &pa, uint32_t t)
{
    typedef EncodePackedShape<FAM> S;
    const EncodeRasterArgs &a = pa.r;
    EncodeAt i;
    i.c = (int)(t % (uint32_t)a.slots);
    const uint32_t row = t / (uint32_t)a.slots;
    i.r = (int)(row % (uint32_t)a.height); i.f = (int)(row / (uint32_t)a.height);
    i.d_at = (size_t)i.f * a.dst_frame_stride + (size_t)i.r * a.dst_row_stride;
    const size_t d_step = (size_t)a.step_f * a.dst_frame_stride + (size_t)a.step_r * a.dst_row_stride, d_wrap = a.dst_frame_stride - (size_t)a.height * a.dst_row_stride;
    for (; i.f < a.n_frames; encode_step(a, i, d_step, d_wrap)) {
        const int x0 = S::NPX * i.c;                /* (below width: the slots are ceil(width / NPX)) */
        const int line = a.top_line + (i.r >> 1);
        const bool live = i.r < a.line_rows && line >= 0 && line < a.lpft;
        const uint32_t *rec = a.lines + (size_t)ENC_REC_DWORDS * ((uint64_t)(2u * (uint32_t)i.f + (uint32_t)((i.r & 1) ^ a.bff)) * (uint32_t)a.lpft + (uint32_t)(live ? line : 0));
        uint32_t v[4];
        if (!live) v[0] = v[1] = v[2] = v[3] = a.black4;
        else {
            uint32_t tb[4];                         /* the cells of the pixels x0 .. x0 + 15, four to a dword (the table has 16 entries of room behind the row) */
            __builtin_memcpy(tb, a.cell_of + x0, 16);
            if (!a.narrow) {                        /* as encode_raster_body has it */
                const uint32_t base = tb[0] & 0xFFu;
                uint64_t q;
                __builtin_memcpy(&q, reinterpret_cast<const uint8_t *>(rec) + (base >> 3), 8);
                const uint32_t win = (uint32_t)(q >> (base & 7)), r = base & 31u;
                const uint32_t rot = (win << r) | (win >> ((32u - r) & 31u));
#pragma unroll
                for (int k = 0; k < S::NV; k++) v[k] = enc_four_win(a, tb[k], rot);
            } else {
#pragma unroll
                for (int k = 0; k < S::NV; k++) v[k] = enc_four_plain(a, tb[k], rec);
            }
            if (S::NV < 4) v[3] = a.black4;
        }
        const int n = a.width - x0;                 /* the unit's pixels that the row has */
        if (n < S::NPX) {                           /* the last unit: what a pair or a group holds behind the width is black */
#pragma unroll
            for (int k = 0; k < S::NV; k++) {
                const int have = n - 4 * k;         /* of this dword */
                const uint32_t m = have >= 4 ? 0xFFFFFFFFu : have <= 0 ? 0u : (1u << (8 * have)) - 1u;
                v[k] = (v[k] & m) | (a.black4 & ~m);
            }
        }
        uint32_t o[S::NB / 4];
        encp_expand<FAM>(v, o);
        const uint32_t at = (uint32_t)S::NB * (uint32_t)i.c;
        uint8_t *out = a.dst + i.d_at + at;
        if (at + (uint32_t)S::NB <= pa.row_bytes) __builtin_memcpy(out, o, S::NB);
        else {                                      /* the tail of a row: its bytes below row_bytes */
#pragma unroll
            for (int k = 0; k < S::NB; k++) if (at + (uint32_t)k < pa.row_bytes) out[k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
        }
    }
}

/* The 16 bytes of piece `phase` of a 48-byte unit (3 bytes a pixel) from the levels of the six pixels it touches, y0 .. y3 in l4, y4 y5 in l2:
 * phase 0 is the pixels 0 .. 5 of the unit (the last with one byte), 1 the pixels 5 .. 10 (two bytes, four pixels, two bytes), 2 the pixels 10 .. 15
 * (the first with one byte).  All three bytes of a pixel are its luma, so which of them a piece holds does not matter. */
template <int PHASE> __device__ __forceinline__ void encp_rgb3_piece(uint32_t l4, uint32_t l2, uint32_t *o)
{
    const uint32_t v[2] = { l4, l2 };
    const uint32_t y0 = encp_byte(v, 0), y1 = encp_byte(v, 1), y2 = encp_byte(v, 2), y3 = encp_byte(v, 3), y4 = encp_byte(v, 4), y5 = encp_byte(v, 5);
    if (PHASE == 0) {               /* y0 y0 y0 y1, y1 y1 y2 y2, y2 y3 y3 y3, y4 y4 y4 y5 */
        o[0] = encp_three(y0) | (y1 << 24); o[1] = y1 | (y1 << 8) | (y2 << 16) | (y2 << 24); o[2] = y2 | (encp_three(y3) << 8); o[3] = encp_three(y4) | (y5 << 24);
    } else if (PHASE == 1) {        /* y0 y0 y1 y1, y1 y2 y2 y2, y3 y3 y3 y4, y4 y4 y5 y5 */
        o[0] = y0 | (y0 << 8) | (y1 << 16) | (y1 << 24); o[1] = y1 | (encp_three(y2) << 8); o[2] = encp_three(y3) | (y4 << 24); o[3] = y4 | (y4 << 8) | (y5 << 16) | (y5 << 24);
    } else {                        /* y0 y1 y1 y1, y2 y2 y2 y3, y3 y3 y4 y4, y4 y5 y5 y5 */
        o[0] = y0 | (encp_three(y1) << 8); o[1] = encp_three(y2) | (y3 << 24); o[2] = y3 | (y3 << 8) | (y4 << 16) | (y4 << 24); o[3] = y4 | (encp_three(y5) << 8);
    }
}

/* 16 bytes at byte `at` of a row: one store where they lie inside the row's row_bytes, else the bytes of them that do */
__device__ __forceinline__ void encp_store_piece(uint8_t *drow, uint32_t at, uint32_t row_bytes, const uint32_t *o)
{
    if (at + 16u <= row_bytes) __builtin_memcpy(drow + at, o, 16);
    else {
#pragma unroll
        for (int k = 0; k < 16; k++) if (at + (uint32_t)k < row_bytes) drow[at + k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
    }
}

/* The builds with 48 and 64 bytes a unit (3 and 4 bytes a pixel).  A lane that stored its own unit's 48 or 64 consecutive bytes would leave every store
 * instruction of its wave with 64 pieces of 16 bytes that lie 48 or 64 bytes apart, which the memory side takes at little more than half the rate of
 * consecutive ones (profiles/encode_notes.md).  So four neighbouring lanes - slots 4 Q .. 4 Q + 3 of a row, a quad - share their four units, the
 * pixels 64 Q .. 64 Q + 63 and the K = 12 or 16 pieces of 16 bytes these make: lane q of the quad owns the pieces q, q + 4, q + 8 (, q + 12), so the
 * k-th store of the four lanes writes 64 consecutive bytes.  A piece is 4 pixels (4 bytes a pixel) or touches 6 (3 bytes a pixel, three phases; a
 * lane has one piece of each phase, so the phases are compile-time and the piece that has one is found by arithmetic on q); its table entries are
 * one 4- or 8-byte load, clamped to the table's room behind the row, and all pieces of a lane are looked up in ONE window of the record, from the
 * lane's lowest entry on: the host's rule for that is narrow_quad.  A row has whole quads of slots; pieces at or behind row_bytes are not stored. */
template <int FAM> __device__ inline void encode_packed_quad_body(const EncodePackedArgs &pa, uint32_t t)
{
    constexpr int K = EncodePackedShape<FAM>::NB / 16;          /* pieces of a lane */
    constexpr bool RGB3 = FAM == ENCP_RGB3;
    const EncodeRasterArgs &a = pa.r;
    EncodeAt i;
    i.c = (int)(t % (uint32_t)a.slots);
    const uint32_t row = t / (uint32_t)a.slots;
    i.r = (int)(row % (uint32_t)a.height); i.f = (int)(row / (uint32_t)a.height);
    i.d_at = (size_t)i.f * a.dst_frame_stride + (size_t)i.r * a.dst_row_stride;
    const size_t d_step = (size_t)a.step_f * a.dst_frame_stride + (size_t)a.step_r * a.dst_row_stride, d_wrap = a.dst_frame_stride - (size_t)a.height * a.dst_row_stride;
    for (; i.f < a.n_frames; encode_step(a, i, d_step, d_wrap)) {
        const uint32_t quad = (uint32_t)i.c >> 2, q = (uint32_t)i.c & 3u;
        const int line = a.top_line + (i.r >> 1);
        const bool live = i.r < a.line_rows && line >= 0 && line < a.lpft;
        const uint32_t *rec = a.lines + (size_t)ENC_REC_DWORDS * ((uint64_t)(2u * (uint32_t)i.f + (uint32_t)((i.r & 1) ^ a.bff)) * (uint32_t)a.lpft + (uint32_t)(live ? line : 0));
        uint32_t at[K], lo[K], hi[K];               /* piece j: its byte in the row, the table entries of its pixels (hi: the fifth and sixth) */
#pragma unroll
        for (int j = 0; j < K; j++) {
            uint32_t piece, x;                      /* the piece in the quad, its first pixel in the row */
            if (RGB3) { piece = q + 4u * ((j + 2u * q) % 3u); x = ENCP_QUAD_PX * quad + 16u * (piece / 3u) + 5u * j; }     /* the piece of phase j: (q + 4 k) % 3 = j */
            else { piece = q + 4u * j; x = ENCP_QUAD_PX * quad + 4u * piece; }
            at[j] = 16u * (uint32_t)K * 4u * quad + 16u * piece;
            const uint8_t *tbl = a.cell_of + (x < (uint32_t)a.width ? x : (uint32_t)a.width);      /* (a piece behind the row: inside the table's room, and not stored) */
            __builtin_memcpy(&lo[j], tbl, 4);
            if (RGB3) __builtin_memcpy(&hi[j], tbl + 4, 4); else hi[j] = 0;
        }
        uint32_t l4[K], l2[K];                      /* the levels of those pixels */
        if (!live) {
#pragma unroll
            for (int j = 0; j < K; j++) l4[j] = l2[j] = a.black4;
        } else if (!pa.narrow_quad) {
            uint32_t base = lo[0] & 0xFFu;          /* the lane's lowest entry: the table rises */
            if (RGB3) {
#pragma unroll
                for (int j = 1; j < K; j++) base = (lo[j] & 0xFFu) < base ? (lo[j] & 0xFFu) : base;
            }
            uint64_t w8;
            __builtin_memcpy(&w8, reinterpret_cast<const uint8_t *>(rec) + (base >> 3), 8);
            const uint32_t win = (uint32_t)(w8 >> (base & 7)), r = base & 31u;
            const uint32_t rot = (win << r) | (win >> ((32u - r) & 31u));
#pragma unroll
            for (int j = 0; j < K; j++) { l4[j] = enc_four_win(a, lo[j], rot); l2[j] = RGB3 ? enc_four_win(a, hi[j], rot) : 0u; }
        } else {
#pragma unroll
            for (int j = 0; j < K; j++) { l4[j] = enc_four_plain(a, lo[j], rec); l2[j] = RGB3 ? enc_four_plain(a, hi[j], rec) : 0u; }
        }
        uint8_t *drow = a.dst + i.d_at;
#pragma unroll
        for (int j = 0; j < K; j++) {
            uint32_t o[4];
            if (RGB3) { if (j == 0) encp_rgb3_piece<0>(l4[j], l2[j], o); else if (j == 1) encp_rgb3_piece<1>(l4[j], l2[j], o); else encp_rgb3_piece<2>(l4[j], l2[j], o); }
            else {
#pragma unroll
                for (int k = 0; k < 4; k++) o[k] = encp_three((l4[j] >> (8 * k)) & 0xFFu) | 0xFF000000u;     /* y y y 255 */
            }
            encp_store_piece(drow, at[j], pa.row_bytes, o);
        }
    }
}

/* thread t of a launch of a family's build */
template <int FAM> __device__ inline void encode_packed_body(const EncodePackedArgs &pa, uint32_t t)
{
    if constexpr (EncodePackedShape<FAM>::QUAD) encode_packed_quad_body<FAM>(pa, t);
    else encode_packed_unit_body<FAM>(pa, t);
}

} // namespace sdv

#ifndef SDV_EMU
template <int FAM> __global__ void __launch_bounds__(256) sdv_k_encode_raster_packed(sdv::EncodePackedArgs a)
{
    sdv::encode_packed_body<FAM>(a, blockIdx.x * 256u + threadIdx.x);
}
#endif
