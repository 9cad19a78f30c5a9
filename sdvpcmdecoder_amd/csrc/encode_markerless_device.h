/*
 * encode_markerless_device.h - device side of sdv_encode_markerless_frames (include/sdvpcm.h): interleaved 16-bit PCM -> Sony PCM-1 and
 * PCM-1600/1610/1630 ("PCM-16x0", SI and EI) video frames, for gfx950.  Included by engine.inc behind encode_device.h; compiled by hipcc into the
 * product and by g++ for the CPU tests (tests/emu).  The format is the text of the header; the decode path reads it back
 * (tests/test_encode_markerless.py).
 *
 * One step of its own, the words, a kernel per format; the raster is sdv_k_encode_raster of encode_device.h as it is: a packed line stays the
 * record of 32 bytes, cell c at bit c + 1, with bits 0 and CELLS + 1 clear (95 and 194 of 256 bits), the table's entries (at most 194) fit a byte and
 * the 8 record bytes the raster reads begin at byte 194 >> 3 = 24 at most.
 *   - words (mlenc_pcm1_words_body, mlenc_pcm16_words_body): a thread per line of the call's fields.  Neither format carries anything from one
 *     frame to the next, so a line gathers its pairs from the call's PCM alone, by the inverse of the interleave - sub-line -> pair, a few integer
 *     operations, no table in memory - reads them bytewise at any alignment, makes the words (PCM-1: the 13-bit companded word; PCM-16x0: L, R or
 *     L ^ R), the CRCs and, for PCM-16x0, the Control Bit, and packs the cells.  The lines of a field read pairs that lie 46 or 35 sub-lines apart, so
 *     neighbouring threads do not read neighbouring bytes; the step moves 1/500 of the call's bytes and is left that way.  The threads behind the
 *     lines fill the cell table for the format's cell count, as encode_words_body does for 137.
 * No LDS, no atomics, no wave collectives.
 */
#pragma once
#include "encode_device.h"

namespace sdv {

enum { MLENC_PCM1_CELLS = 94, MLENC_PCM16_CELLS = 193, MLENC_LINES = 245, MLENC_FIELD_PAIRS = 735, MLENC_MAX_HEADER = 8 };

struct MlencWordsArgs {
    const uint8_t *pcm; uint64_t n_pairs;           /* int16 L R pairs at any alignment; pairs behind n_pairs are silence */
    uint32_t *lines;                                /* ENC_REC_DWORDS per line: field, then line of the field (PCM-1: the Header lines first) */
    uint8_t *cell_of; int width; int64_t data_start, span;      /* the table: width + 2 ENC_TABLE_PAD entries, the first one pixel -ENC_TABLE_PAD */
    uint64_t n_lines;                               /* lines of the call */
    int lpft, header;                               /* lines of a field; PCM-1: Header lines on top of them */
    int cells;                                      /* 94 / 193 */
    uint8_t ei, ctrl_flags;                         /* PCM-16x0: the interleave, SDV_ENC_ML_* */
};

/* entry i of the cell table: 0 left of the window, cell + 1 inside, cells + 1 right of it */
__device__ __forceinline__ void mlenc_table(const MlencWordsArgs &a, uint64_t i)
{
    if (i >= (uint64_t)a.width + 2 * ENC_TABLE_PAD) return;
    const int64_t d = (int64_t)i - ENC_TABLE_PAD - a.data_start;
    a.cell_of[i] = (uint8_t)(d < 0 ? 0 : d >= a.span ? a.cells + 1 : 1 + (d * a.cells) / a.span);
}

/* pair `pair` of the call as L | R << 16, silence behind n_pairs */
__device__ __forceinline__ uint32_t mlenc_pair(const MlencWordsArgs &a, uint64_t pair)
{
    if (pair >= a.n_pairs) return 0;
    const uint8_t *p = a.pcm + 4 * pair;
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

__device__ __forceinline__ void mlenc_store(const MlencWordsArgs &a, uint64_t t, const uint32_t rec[ENC_REC_DWORDS])
{
    uint4 *out = reinterpret_cast<uint4 *>(a.lines + ENC_REC_DWORDS * t);
    uint4 lo, hi;
    lo.x = rec[0]; lo.y = rec[1]; lo.z = rec[2]; lo.w = rec[3]; hi.x = rec[4]; hi.y = rec[5]; hi.z = rec[6]; hi.w = rec[7];
    out[0] = lo; out[1] = hi;
}

/* CRC-16/CCITT-FALSE, MSB first: `bits` bits of v on top of crc */
__device__ __forceinline__ uint32_t mlenc_crc(uint32_t crc, uint32_t v, int bits)
{
    for (int bit = bits - 1; bit >= 0; bit--) {
        const uint32_t top = ((crc >> 15) ^ (v >> bit)) & 1u;
        crc = ((crc << 1) & 0xFFFFu) ^ (top ? 0x1021u : 0u);
    }
    return crc;
}

/* ---- PCM-1 ------------------------------------------------------------------------------------------------------------------------------ */
/* a sample as its 13-bit word: the range bit and 12 bits of the sample's upper 14, or of its upper 12 */
__device__ __forceinline__ uint32_t mlenc_pcm1_word(uint32_t s16)
{
    const int32_t s = (int32_t)(int16_t)s16;
    return s >= -8192 && s < 8192 ? 0x1000u | ((uint32_t)(s >> 2) & 0x0FFFu) : (uint32_t)(s >> 4) & 0x0FFFu;
}

/* the pair of a field that sits on its sub-line u = 0 .. 734: interleave block u / 92, halves of 46 sub-lines, the odd pairs of an even block and
 * the even pairs of an odd block in the first half */
__device__ __forceinline__ uint32_t mlenc_pcm1_pair_of(uint32_t u)
{
    const uint32_t itl = u / 92u, r = u % 92u, second = r >= 46u ? 1u : 0u, wp = r - 46u * second;
    return 92u * itl + 2u * wp + (((itl & 1u) ^ second) ^ 1u);
}

__device__ inline void mlenc_pcm1_words_body(const MlencWordsArgs &a, uint64_t t)
{
    if (t >= a.n_lines) { mlenc_table(a, t - a.n_lines); return; }
    const uint64_t fld = t / (uint64_t)a.lpft;
    const int j = (int)(t % (uint64_t)a.lpft) - a.header;
    uint32_t w[6], crc;
    if (j < 0) {                                    /* a Header line */
        w[0] = 0x0666; w[1] = 0x0CCC; w[2] = 0x1999; w[3] = 0x1333; w[4] = 0x0666; w[5] = 0x0CCC; crc = 0xCCCC;
    } else {
        crc = 0xFFFF;
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const uint32_t lr = mlenc_pair(a, fld * MLENC_FIELD_PAIRS + mlenc_pcm1_pair_of(3u * (uint32_t)j + (uint32_t)q));
            w[2 * q] = mlenc_pcm1_word(lr & 0xFFFFu); w[2 * q + 1] = mlenc_pcm1_word(lr >> 16);
            crc = mlenc_crc(crc, ~w[2 * q] & 0x1FFFu, 13);
            crc = mlenc_crc(crc, ~w[2 * q + 1] & 0x1FFFu, 13);
        }
        crc = ~crc & 0xFFFFu;
    }
    uint32_t rec[ENC_REC_DWORDS];
#pragma unroll
    for (int i = 0; i < ENC_REC_DWORDS; i++) rec[i] = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) enc_put(rec, 1 + 13 * k, __brev(w[k] & 0x1FFFu) >> 19);
    enc_put(rec, 1 + 13 * 6, __brev(crc & 0xFFFFu) >> 16);
    mlenc_store(a, t, rec);
}

/* ---- PCM-16x0 --------------------------------------------------------------------------------------------------------------------------- */
__device__ inline void mlenc_pcm16_words_body(const MlencWordsArgs &a, uint64_t t)
{
    if (t >= a.n_lines) { mlenc_table(a, t - a.n_lines); return; }
    const uint64_t fld = t / (uint64_t)MLENC_LINES;
    const uint32_t j = (uint32_t)(t % (uint64_t)MLENC_LINES);
    const uint64_t pair0 = (fld >> 1) * (2u * MLENC_FIELD_PAIRS);
    uint32_t rec[ENC_REC_DWORDS];
#pragma unroll
    for (int i = 0; i < ENC_REC_DWORDS; i++) rec[i] = 0;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const uint32_t s = (uint32_t)(fld & 1u) * MLENC_FIELD_PAIRS + 3u * j + (uint32_t)q;         /* sub-line of the frame */
        uint32_t block, role, odd;
        if (a.ei) { block = s % 490u; role = s / 490u; odd = block & 1u; }
        else { block = 35u * (s / 105u) + s % 35u; role = (s % 105u) / 35u; odd = (s % 35u) & 1u; }
        const int pos = 1 + 64 * q + (q == 2 ? 1 : 0);
        uint32_t crc = 0xFFFF;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint32_t lr = mlenc_pair(a, pair0 + 3u * block + (uint32_t)k), l = lr & 0xFFFFu, r = lr >> 16;
            const bool l_first = ((k & 1) != 0) != (odd != 0);
            const uint32_t w = role == 1u ? l ^ r : (role == 0u) == l_first ? l : r;
            crc = mlenc_crc(crc, w, 16);
            enc_put(rec, pos + 16 * k, __brev(w) >> 16);
        }
        enc_put(rec, pos + 48, __brev(crc) >> 16);
    }
    /* the Control Bit: 1, but 0 on lines 35 i + 0 .. 3 of a field for emphasis, 44100 Hz, EI and the code bit */
    const uint32_t m = j % 35u;
    const bool clear = (m == 0u && (a.ctrl_flags & SDV_ENC_ML_EMPHASIS)) || (m == 1u && (a.ctrl_flags & SDV_ENC_ML_RATE_44100)) || (m == 2u && a.ei) ||
                       (m == 3u && (a.ctrl_flags & SDV_ENC_ML_CODE));
    if (!clear) enc_put(rec, 1 + 128, 1u);
    mlenc_store(a, t, rec);
}

} // namespace sdv

#ifndef SDV_EMU
__global__ void __launch_bounds__(256) sdv_k_mlenc_pcm1_words(sdv::MlencWordsArgs a)
{
    sdv::mlenc_pcm1_words_body(a, (uint64_t)blockIdx.x * 256u + threadIdx.x);
}
__global__ void __launch_bounds__(256) sdv_k_mlenc_pcm16_words(sdv::MlencWordsArgs a)
{
    sdv::mlenc_pcm16_words_body(a, (uint64_t)blockIdx.x * 256u + threadIdx.x);
}
#endif
