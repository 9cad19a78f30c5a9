/*
 * encode_device.h - device side of sdv_encode_frames (include/sdvpcm.h): interleaved 16-bit PCM -> STC-007 / PCM-F1 video frames, for gfx950.
 * Included by engine.inc; compiled by hipcc into the product and by g++ for the CPU tests (tests/emu).  The format is the text of the header;
 * the decode path reads it back (tests/test_encode.py).
 *
 * Two steps, neither with LDS, atomics or wave collectives:
 *   - words (encode_words_body): a thread per line of the call's fields.  A data line gathers its eight slots - word k of the block 16 k lines
 *     back, from the call's PCM or, in front of it, from the 112 blocks the engine keeps -, with P and Q of the blocks slots 6 and 7 come from,
 *     adds the CRC and packs the 137 cells, cell c at bit c + 1, into a record of 32 bytes.  A control line is made from the field count.  The
 *     threads of the call's last 112 data lines also leave their own block's words as the next call's history, thread 0 the next field count -
 *     in a second state buffer, which the host swaps in: nothing a thread of the launch reads is written by it.  The threads behind the lines
 *     fill the cell table: for every x of a row the cell it shows, by the header's integer division, plus 1, or ENC_LEFT / ENC_RIGHT outside the
 *     data window - the numbers of two bits of every record that are clear.
 *   - raster (encode_raster_body): the hot path, write only.  Work item = one 16-byte-aligned chunk of a destination row, as sdv_k_ingest has
 *     it: slot c of a row whose first byte sits at address a covers the row bytes p0 .. p0 + 15, p0 = 16 c - (a & 15); one flat index over
 *     (frame, row, slot) is walked with a grid stride the host hands over split into frames, rows and slots, so a step is three additions with
 *     carry.  Every chunk - whole, head or tail of a row, inside the data window or across its edge - is made the same way, so the lanes of a
 *     wave do not part: 16 table bytes (the table has 16 entries of room on either side of the row), the 8 record bytes the chunk's first entry
 *     lies in, rotated so that an entry sits at the bit of its number modulo 32, and one shift of that 32-bit window per pixel; the entries of
 *     16 neighbouring pixels are at most 31 apart (the host says so, EncodeRasterArgs::narrow, or the pixels are read one by one).  Four pixels
 *     become a dword of levels without a multiplication.  A whole chunk is one 16-byte store; of a head or a tail the bytes inside the row are
 *     stored one by one.
 */
#pragma once
#include "../../include/sdvpcm.h"

namespace sdv {

enum { ENC_DELAY = 112, ENC_CELLS = 137, ENC_REC_DWORDS = 8, ENC_TABLE_PAD = 16 };
/* A pixel's entry in the cell table and a cell's bit in a line's record are numbered alike: 0 for a pixel left of the data window, c + 1 for
 * cell c, ENC_RIGHT for a pixel right of the window; bits 0 and ENC_RIGHT of a record are clear, so every pixel of a row is looked up the same way. */
enum { ENC_LEFT = 0, ENC_RIGHT = ENC_CELLS + 1 };

/* what the engine keeps on the device between two calls of a tape */
struct EncodeState {
    uint32_t tc;                        /* time code of the next field as a count of fields from 0:00:00, below 16 hours */
    uint32_t _pad;
    uint16_t hist[ENC_DELAY][8];        /* the words of the last 112 blocks, oldest first: 14 bit L0 R0 L1 R1 L2 R2 P Q; 16 bit the six 16-bit words, their XOR, 0 */
};

struct EncodeWordsArgs {
    const uint8_t *pcm; uint64_t n_pairs;           /* int16 L R pairs at any alignment; pairs behind n_pairs are silence */
    const EncodeState *st_in; EncodeState *st_out;
    uint32_t *lines;                                /* ENC_REC_DWORDS per line: field, then line of the field (control line first) */
    uint8_t *cell_of; int width; int64_t data_start, span;      /* the table: width + 2 ENC_TABLE_PAD entries, the first one pixel -ENC_TABLE_PAD */
    uint64_t n_lines, n_data;                       /* lines of the call with and without the control lines */
    int lpf, lpft;                                  /* data lines of a field; lines of a field (one more with the control block) */
    uint32_t tc0, tc_wrap, fps;                     /* fresh: the time code of the first field; 16 hours in fields; fields per second */
    uint16_t addr1_index, ctrl_word;                /* index << 8; the control bits */
    uint8_t ctrl, res16, fresh;
};

/* T: multiply by x modulo x^14 + x^8 + 1 */
__device__ __forceinline__ uint32_t enc_t_mul(uint32_t v) { return ((v << 1) & 0x3FFFu) ^ ((v >> 13) & 1u ? 0x0101u : 0u); }

/* sample w (L0 R0 L1 R1 L2 R2) of block b of the call, as 16 bits */
__device__ inline uint32_t enc_sample(const EncodeWordsArgs &a, int64_t b, int w)
{
    const uint64_t pair = 3 * (uint64_t)b + (uint64_t)(w >> 1);
    if (pair >= a.n_pairs) return 0;
    const uint8_t *p = a.pcm + 4 * pair + 2 * (size_t)(w & 1);
    return (uint32_t)p[0] | (uint32_t)p[1] << 8;
}

/* the eight words of block b >= 0 of the call, as the history keeps them */
__device__ inline void enc_block(const EncodeWordsArgs &a, int64_t b, uint32_t w[8])
{
    uint32_t p = 0, q = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const uint32_t s = enc_sample(a, b, k);
        w[k] = a.res16 ? s : s >> 2;                /* 14 bit: (sample >> 2) & 0x3FFF */
        p ^= w[k];
        q = enc_t_mul(q ^ w[k]);                    /* Horner: T^6 L0 + T^5 R0 + ... + T R2 */
    }
    w[6] = p; w[7] = a.res16 ? 0 : q;
}

/* word k of block b, b >= -ENC_DELAY: from the call's PCM, or from the blocks in front of it (zero in front of the tape) */
__device__ inline uint32_t enc_word(const EncodeWordsArgs &a, int64_t b, int k)
{
    if (b < 0) return a.fresh ? 0u : a.st_in->hist[ENC_DELAY + b][k];
    if (k < 6) { const uint32_t s = enc_sample(a, b, k); return a.res16 ? s : s >> 2; }
    uint32_t w[8];
    enc_block(a, b, w);
    return w[k];
}

/* CRC-16/CCITT-FALSE over eight 14-bit words, MSB first */
__device__ inline uint32_t enc_crc(const uint32_t w[8])
{
    uint32_t crc = 0xFFFF;
    for (int k = 0; k < 8; k++)
        for (int bit = 13; bit >= 0; bit--) {
            const uint32_t top = ((crc >> 15) ^ (w[k] >> bit)) & 1u;
            crc = ((crc << 1) & 0xFFFFu) ^ (top ? 0x1021u : 0u);
        }
    return crc;
}

/* n bits of v (its bit 0 first) to the cells pos .. pos + n - 1 of a record */
__device__ __forceinline__ void enc_put(uint32_t *rec, int pos, uint32_t v)
{
    rec[pos >> 5] |= v << (pos & 31);
    if (pos & 31) rec[(pos >> 5) + 1] |= v >> (32 - (pos & 31));
}

/* 1010, eight words and the CRC MSB first, 01111: cell c at bit c + 1 of the record */
__device__ inline void enc_pack(const uint32_t w[8], uint32_t crc, uint32_t rec[ENC_REC_DWORDS])
{
#pragma unroll
    for (int i = 0; i < ENC_REC_DWORDS; i++) rec[i] = 0;
    enc_put(rec, 1, 0x5u);                                          /* cells 1 0 1 0 */
#pragma unroll
    for (int k = 0; k < 8; k++) enc_put(rec, 5 + 14 * k, __brev(w[k] & 0x3FFFu) >> 18);
    enc_put(rec, 5 + 14 * 8, __brev(crc & 0xFFFFu) >> 16);
    enc_put(rec, 5 + 14 * 8 + 16, 0x1Eu);                           /* cells 0 1 1 1 1 */
}

__device__ inline void encode_words_body(const EncodeWordsArgs &a, uint64_t t)
{
    if (t >= a.n_lines) {                           /* the cell table */
        const uint64_t i = t - a.n_lines;           /* entry i is pixel x = i - ENC_TABLE_PAD: a chunk may begin in front of its row and end behind it */
        if (i >= (uint64_t)a.width + 2 * ENC_TABLE_PAD) return;
        const int64_t d = (int64_t)i - ENC_TABLE_PAD - a.data_start;
        a.cell_of[i] = (uint8_t)(d < 0 ? ENC_LEFT : d >= a.span ? ENC_RIGHT : 1 + (d * ENC_CELLS) / a.span);
        return;
    }
    const uint64_t fld = t / (uint64_t)a.lpft;
    const int j = (int)(t % (uint64_t)a.lpft);
    const uint32_t tc_first = a.fresh ? a.tc0 : a.st_in->tc;
    uint32_t w[8];
    if (a.ctrl && j == 0) {                         /* the control line of field fld */
        const uint32_t tc = (uint32_t)(((uint64_t)tc_first + fld) % a.tc_wrap);
        const uint32_t field = tc % a.fps, secs = tc / a.fps, second = secs % 60u, minute = (secs / 60u) % 60u, hour = secs / 3600u;
        w[0] = 0x3333; w[1] = 0x0CCC; w[2] = 0x3333; w[3] = 0x0CCC; w[4] = 0;
        w[5] = a.addr1_index | hour << 4 | minute >> 2;
        w[6] = (minute & 3u) << 12 | second << 6 | field;
        w[7] = a.ctrl_word;
    } else {
        const int64_t m = (int64_t)fld * a.lpf + (j - (int)a.ctrl);         /* data line of the call */
        if (a.res16) {                              /* slot 7: the two low bits of the seven 16-bit words of this line */
            uint32_t s = 0;
#pragma unroll
            for (int k = 0; k < 7; k++) { const uint32_t full = enc_word(a, m - 16 * k, k); w[k] = full >> 2; s |= (full & 3u) << (12 - 2 * k); }
            w[7] = s;
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) w[k] = enc_word(a, m - 16 * k, k);
        }
        if ((uint64_t)m + ENC_DELAY >= a.n_data) {  /* one of the last 112 blocks: the next call's history */
            uint32_t own[8];
            enc_block(a, m, own);
            uint16_t *h = a.st_out->hist[(uint64_t)m + ENC_DELAY - a.n_data];
#pragma unroll
            for (int k = 0; k < 8; k++) h[k] = (uint16_t)own[k];
        }
    }
    if (t == 0) { a.st_out->tc = (uint32_t)(((uint64_t)tc_first + a.n_lines / (uint64_t)a.lpft) % a.tc_wrap); a.st_out->_pad = 0; }
    uint32_t rec[ENC_REC_DWORDS];
    enc_pack(w, enc_crc(w), rec);
    uint4 *out = reinterpret_cast<uint4 *>(a.lines + ENC_REC_DWORDS * t);
    uint4 lo, hi;
    lo.x = rec[0]; lo.y = rec[1]; lo.z = rec[2]; lo.w = rec[3]; hi.x = rec[4]; hi.y = rec[5]; hi.z = rec[6]; hi.w = rec[7];
    out[0] = lo; out[1] = hi;
}

/* ---- raster ----------------------------------------------------------------------------------------------------------------------------- */
struct EncodeRasterArgs {
    const uint32_t *lines;
    const uint8_t *cell_of;             /* entry x: the cell of pixel x, for x = -ENC_TABLE_PAD .. width + ENC_TABLE_PAD - 1 */
    uint8_t *dst; size_t dst_row_stride, dst_frame_stride;
    int n_frames, width, height;
    int line_rows;                      /* rows below this one show lines: height without the last row of an odd height */
    int lpft, top_line, bff;
    uint32_t black4, white4;            /* the levels in every byte */
    int narrow;                         /* the entries of 16 neighbouring pixels can lie more than 31 apart: no window */
    int slots;                          /* chunk slots per row */
    int step_f, step_r, step_c;         /* the grid stride (threads of the launch) as frames, rows and slots */
};

/* four pixels, a bit in every byte of `bits`, as levels: no carries between the bytes */
__device__ __forceinline__ uint32_t enc_levels(const EncodeRasterArgs &a, uint32_t bits)
{
    const uint32_t m = (bits + 0x7F7F7F7Fu) ^ 0x7F7F7F7Fu;          /* 0x01 -> 0xFF in every byte: 0x7F + 1 stays inside its byte */
    return a.black4 ^ (m & (a.black4 ^ a.white4));
}

/* Four pixels whose table entries are the bytes of `cells`, from `rot`: the 32 bits of the record from the chunk's first entry on, each at the bit of
 * its number modulo 32 (a shift looks at the five low bits of its count). */
__device__ __forceinline__ uint32_t enc_four_win(const EncodeRasterArgs &a, uint32_t cells, uint32_t rot)
{
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) bits |= ((rot >> ((cells >> (8 * j)) & 31u)) & 1u) << (8 * j);
    return enc_levels(a, bits);
}
/* ... the plain way: entries any distance apart, each from the record in memory */
__device__ __forceinline__ uint32_t enc_four_plain(const EncodeRasterArgs &a, uint32_t cells, const uint32_t *rec)
{
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t c = (cells >> (8 * j)) & 0xFFu;
        bits |= ((rec[c >> 5] >> (c & 31)) & 1u) << (8 * j);
    }
    return enc_levels(a, bits);
}

struct EncodeAt { int c, r, f; size_t d_at; };
__device__ __forceinline__ void encode_step(const EncodeRasterArgs &a, EncodeAt &i, size_t d_step, size_t d_wrap)
{
    i.c += a.step_c;
    const bool cc = i.c >= a.slots;
    if (cc) i.c -= a.slots;
    i.r += a.step_r + (cc ? 1 : 0);
    const bool cr = i.r >= a.height;
    if (cr) i.r -= a.height;
    i.f += a.step_f + (cr ? 1 : 0);
    i.d_at += d_step + (cc ? a.dst_row_stride : 0) + (cr ? d_wrap : 0);
}

/* thread t of a launch of step_f * height * slots + step_r * slots + step_c threads */
__device__ inline void encode_raster_body(const EncodeRasterArgs &a, uint32_t t)
{
    EncodeAt i;
    i.c = (int)(t % (uint32_t)a.slots);
    const uint32_t row = t / (uint32_t)a.slots;
    i.r = (int)(row % (uint32_t)a.height); i.f = (int)(row / (uint32_t)a.height);
    i.d_at = (size_t)i.f * a.dst_frame_stride + (size_t)i.r * a.dst_row_stride;
    const size_t d_step = (size_t)a.step_f * a.dst_frame_stride + (size_t)a.step_r * a.dst_row_stride, d_wrap = a.dst_frame_stride - (size_t)a.height * a.dst_row_stride;
    for (; i.f < a.n_frames; encode_step(a, i, d_step, d_wrap)) {
        uint8_t *drow = a.dst + i.d_at;
        const int p0 = 16 * i.c - (int)((uintptr_t)drow & 15);
        if (p0 >= a.width) continue;                /* the spare slot of a row */
        /* row 2 r shows line top_line + r of the field first in time (of the other one with bottom field first), row 2 r + 1 the other field's */
        const int line = a.top_line + (i.r >> 1);
        const bool live = i.r < a.line_rows && line >= 0 && line < a.lpft;
        const uint32_t *rec = a.lines + (size_t)ENC_REC_DWORDS * ((uint64_t)(2u * (uint32_t)i.f + (uint32_t)((i.r & 1) ^ a.bff)) * (uint32_t)a.lpft + (uint32_t)(live ? line : 0));
        uint4 v;
        if (!live) v.x = v.y = v.z = v.w = a.black4;
        else {
            struct { uint32_t x, y, z, w; } tb;     /* the cells of the pixels p0 .. p0 + 15, four to a dword (the table has 16 entries of room on either side) */
            __builtin_memcpy(&tb, a.cell_of + p0, 16);
            if (!a.narrow) {
                /* The entries of a chunk rise and lie within 32 of its first one. */
                const uint32_t base = tb.x & 0xFFu;
                uint64_t q;
                __builtin_memcpy(&q, reinterpret_cast<const uint8_t *>(rec) + (base >> 3), 8);       /* (base <= 138: bytes 17 .. 24 of 32 at most) */
                const uint32_t win = (uint32_t)(q >> (base & 7)), r = base & 31u;               /* entries base .. base + 31 at bits 0 .. 31 */
                const uint32_t rot = (win << r) | (win >> ((32u - r) & 31u));                   /* ... each at the bit of its own number modulo 32 */
                v.x = enc_four_win(a, tb.x, rot); v.y = enc_four_win(a, tb.y, rot); v.z = enc_four_win(a, tb.z, rot); v.w = enc_four_win(a, tb.w, rot);
            } else {
                v.x = enc_four_plain(a, tb.x, rec); v.y = enc_four_plain(a, tb.y, rec); v.z = enc_four_plain(a, tb.z, rec); v.w = enc_four_plain(a, tb.w, rec);
            }
        }
        if (p0 >= 0 && p0 + 16 <= a.width) *reinterpret_cast<uint4 *>(drow + p0) = v;
        else {                                      /* head or tail of a row: the bytes of it that lie in the row */
            const uint32_t px[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
            for (int k = 0; k < 16; k++) if (p0 + k >= 0 && p0 + k < a.width) drow[p0 + k] = (uint8_t)(px[k >> 2] >> (8 * (k & 3)));
        }
    }
}

} // namespace sdv

#ifndef SDV_EMU
__global__ void __launch_bounds__(256) sdv_k_encode_words(sdv::EncodeWordsArgs a)
{
    sdv::encode_words_body(a, (uint64_t)blockIdx.x * 256u + threadIdx.x);
}
__global__ void __launch_bounds__(256) sdv_k_encode_raster(sdv::EncodeRasterArgs a)
{
    sdv::encode_raster_body(a, blockIdx.x * 256u + threadIdx.x);
}
#endif
