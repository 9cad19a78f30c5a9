/*
 * pcm1_frames_device.h - PCM-1 frame driver: the PCM-1 branch of VideoToDigital::doBinarize (videotodigital.cpp:698-1815) and
 * VideoToDigital::prescanCoordinates (:148-345) around the PCM-1 line binarizer of pcm1_bin_device.h (SURVEY.md section 8 row
 * a11 for PCM-1).
 *
 * Two kernels per round:
 *   sdv_k_pcm1_prescan   one wave per (frame, prescan line): the four lines the worker decodes from scratch before every frame
 *                        (all modes but DRAFT) to find the frame's data coordinates and reference level.  The worker resets its
 *                        Binarizer first, so the result is a pure function of the pixels - all frames of a batch at once.
 *   sdv_k_pcm1_frames    one wave per frame, the pattern of the STC-007 frame kernel: the lines of a frame one after the other
 *                        in VideoInFFMPEG::spliceFrame order, every line decoded from what the lines before it left preset on the
 *                        Binarizer (setGoodParameters / setDataCoordinates / setBWLevels), with the per-line bookkeeping of the
 *                        worker (Header lines, duplicate-line detection, coordinate damper, statistics).  Frames run in parallel
 *                        from predicted incoming states; every frame checks the link to its successor itself (stc007_device.h,
 *                        v2d_store_state) and the host repeats the frames behind broken links (markerless_frames_engine.inc;
 *                        the model of the states: markerless_chain_device.h).
 */
#pragma once
#include "markerless_frames_device.h"

namespace sdvp1f {
using namespace sdv;
using namespace sdvp1b;
using namespace sdvmf;

enum { P1_LINES_PF = 245 };                                                     /* PCM1DataStitcher::LINES_PF, pcm1datastitcher.h:103 */

struct FrameArgs1 {
    FrameArgs f;                    /* geometry, flags, states, stats, scratch as for STC-007 (f.recs unused) */
    sdv_pcm1_bin_rec *recs1;        /* frame k: recs1 + k*(height+3) (+1 behind the NEW_FILE frame) */
    PrescanRes *prescan;            /* [n_total][COORD_CHECK_LINES] */
    uint2 *frame_med;               /* [n_total] what frame f pushed into the multi-frame history: {coordinate key, 1} or {0, 0} (nothing) */
};

/* ---- prescan: block = (frame, k) ------------------------------------------------------------------------------------------ */
template <bool kInsane>
__device__ inline void prescan_body(const FrameArgs1 &a1, P1Lds &lds, int f, int k)
{
    const FrameArgs &a = a1.f;
    K1_BEGIN(); K1_T(tq0_);
    PrescanRes r; r.start = r.stop = 0; r.ref = 0; r.valid = 0; r.pad[0] = r.pad[1] = 0;
    if (prescan_runs(a, f)) {
        const int gap = frame_buf_lines(a, f) / (COORD_CHECK_PARTS - 1);
        const int row = frame_buf_row(a, f, (k + 1) * gap);
        if (row >= 0) {
            stage_row(lds.w.px, a.luma + (size_t)f * a.frame_stride + (size_t)row * a.row_stride, a.width);
            K1_T(tq1_); K1_ADD(16, tq0_, tq1_);
#pragma unroll 1
            for (int variant = 0; variant < (sweep_flag_matters(a.preset) ? 2 : 1); variant++) {
                BinCtx c; Bin b;
                b.in_black = b.in_white = b.in_ref = 0; coords_clear(b.in_coord);       /* setGoodParameters() (:221) */
                ctx_for_line(a, c, b);
                b.do_ref_lvl_sweep = variant != 0;
                L1 out;
                process_line_p1<kInsane>(c, b, true, lds, out, a.doubled != 0);
                PrescanRes q = r;
                if (crc_valid(out)) { q.start = out.coords.start; q.stop = out.coords.stop; q.ref = out.ref_level; q.valid = 1; }
                q.pad[1] = out.bw_set || out.service == SDV_SRV_HEADER_LINE ? 1 : 0;      /* (a Header line is only recognised behind the levels) */
                if (lane_id() == 0) a1.prescan[((size_t)variant * a.n_total + f) * COORD_CHECK_LINES + k] = q;
                SDV_WAVE_SYNC();
            }
            K1_T(tq2_); K1_ADD(23, tq0_, tq2_); K1_FLUSH();
            return;
        }
    }
    if (lane_id() == 0) {
        a1.prescan[(size_t)f * COORD_CHECK_LINES + k] = r;
        if (sweep_flag_matters(a.preset)) a1.prescan[((size_t)a.n_total + f) * COORD_CHECK_LINES + k] = r;
    }
}

/* ---- state of a PCM-1 frame wave ------------------------------------------------------------------------------------------ */
struct V2D1 {
    V2D v;                          /* the part shared with STC-007 (last_words: the six data words of last_pcm1_line) */
    uint8_t prescan_ref;
};

__device__ inline void v2d1_load_state(V2D1 &w, WaveLds &lds, const sdv_v2d_state *s, const FrameArgs &a)
{
    v2d_load_state(w.v, lds, s, a);
    w.prescan_ref = (uint8_t)uni(prescan_ref_of(*s));
}

/* The chain after frame f; the link to frame f+1 is checked by the frame itself: when the worker prescans frame
 * f+1 it resets its Binarizer first (prescanCoordinates :221), so what frame f left preset there does not reach frame f+1 and does
 * not count. */
__device__ inline void v2d1_store_state(const V2D1 &w, const WaveLds &lds, sdv_v2d_state *s, const FrameArgs &a)
{
    if (lane_id() != 0) return;
    const V2D &v = w.v;
    sdv_v2d_state o;
    o.bin.in_def_black = v.bin.in_black; o.bin.in_def_white = v.bin.in_white; o.bin.in_def_reference = v.bin.in_ref; o.bin.do_ref_lvl_sweep = 0;
    o.bin.in_def_start = v.bin.in_coord.start; o.bin.in_def_stop = v.bin.in_coord.stop;
    o.bin.in_def_from_doubled = v.bin.in_coord.doubled ? 1 : 0; o.bin._pad2 = 0;
    o.do_ref_lvl_sweep = v.bin.do_ref_lvl_sweep ? 1 : 0; o.reset_stats = v.reset_stats ? 1 : 0;
    o.n_last_valid = (uint8_t)v.n_last; o.n_long_valid = (uint8_t)v.n_long;
    const uint16_t lm = a.doubled ? (uint16_t)((1u << v.n_last) - 1u) : 0, gm = a.doubled ? (uint16_t)((1u << v.n_long) - 1u) : 0;
    o.last_valid_doubled_mask_lo = (uint8_t)(lm & 0xFF); o.last_valid_doubled_mask_hi = (uint8_t)(lm >> 8);
    o.long_valid_doubled_mask = gm;
    for (int i = 0; i < COORD_HISTORY_DEPTH; i++) {
        if (i < v.n_last) { o.last_valid[i].data_start = key_start(lds.lv_keys[i]); o.last_valid[i].data_stop = key_stop(lds.lv_keys[i]); }
        else { o.last_valid[i].data_start = 0; o.last_valid[i].data_stop = 0; }
    }
    for (int i = 0; i < COORD_LONG_HISTORY; i++) {
        if (i < v.n_long) { o.long_valid[i].data_start = key_start(lds.long_keys[i]); o.long_valid[i].data_stop = key_stop(lds.long_keys[i]); }
        else { o.long_valid[i].data_start = 0; o.long_valid[i].data_stop = 0; }
    }
    o._pad[0] = 0; o._pad[1] = (uint8_t)(w.prescan_ref ^ 128);
    *s = o;
    const int f = (int)(s - a.states_out);
    a.flag[f] = (f + 1 < a.n_total && !link_holds(a, f, o, a.states_in[f + 1])) ? VF_BREAK : VF_OK;
}

/* service lines: Binarizer::processLine :539-568 + VideoToDigital :1006-1114 */
__device__ inline void v2d1_service_line(V2D1 &w, const FrameArgs &a, L1 &wl, uint8_t srv)
{
    p1_clear(wl);
    set_service(wl, srv);
    service_state(w.v, a, srv);
    if (srv == SDV_SRV_END_FIELD) for (int i = 0; i < 8; i++) w.v.last_words[i] = 0;           /* last_pcm1_line.clear(): the data words are zero */
}

__device__ inline int16_t p1_get_sample(uint16_t w)     /* pcm1line.cpp:188-222 */
{
    if ((w & (1 << 12)) == 0) w = (uint16_t)(w << 4);
    else {
        const bool pos = (w & (1 << 11)) == 0;
        w = (uint16_t)(w & ~(1 << 12));
        w = (uint16_t)(w << 2);
        if (!pos) w |= (1 << 15) | (1 << 14);
    }
    return (int16_t)w;
}

/* regular line, after Binarizer::processLine: VideoToDigital :1115-1634 (PCM-1 branches) */
__device__ inline void v2d1_post_line(V2D1 &w, const FrameArgs &a, WaveLds &lds, L1 &wl, uint32_t *fv_keys, uint32_t *fi_keys, bool even_line)
{
    V2D &v = w.v;
    const sdv_bin_preset &ps = a.preset;
    if (wl.service != SDV_SRV_NO) {
        if (wl.service == SDV_SRV_HEADER_LINE && v.field_state == FIELD_NEW) v.field_state = FIELD_SAFE;     /* :1064-1088 */
        return;
    }
    const bool count_has_data = wl.bw_set;
    const bool count_has_pcm = crc_valid(wl) || count_has_data;
    if (count_has_pcm && v.field_state == FIELD_NEW) v.field_state = FIELD_UNSAFE;
    if (crc_valid(wl)) {
        v.good_coords_in_field++;
        v.q_line_length = (uint16_t)a.width;
        if (a.check_line_copy) {
            if (v.field_state == FIELD_UNSAFE) {
                set_good_parameters(v.bin, ps, wl);
                if (ps.en_first_line_dup) wl.forced_bad = true;
            } else {
                int diff = 0, silent = 0;
                for (int i = 0; i < 6; i++) {
                    const uint16_t wd = get_word(wl, i);
                    diff += __popc((uint32_t)(uint8_t)(wd ^ v.last_words[i]));          /* the XOR is truncated to uint8_t (pcm1line.cpp:236-263) */
                    const int16_t smp = p1_get_sample(wd);
                    if (!(smp >= 8) && !(smp < -8)) silent++;
                }
                if (!(silent >= 2) && diff <= (P1_BITS / BIT_DIFF_THRES_DIV)) { wl.forced_bad = true; count_dup(v, even_line); }
            }
        }
        if (crc_valid_ignore_forced(wl)) {
            const uint32_t key = coords_key(wl.coords.start, wl.coords.stop);
            push_last_valid<COORD_HISTORY_DEPTH>(lds.lv_keys, v, key);
            fv_keys[v.nfv++] = key;
            if (damper_forces_bad(v, a, lds.lv_keys, wl)) wl.forced_bad = true;
        }
        if (crc_valid(wl)) set_good_parameters(v.bin, ps, wl);
        else count_bad(v, even_line);
        v.field_state = FIELD_INIT;
    } else {
        if (v.q_line_length == 0) v.q_line_length = (uint16_t)a.width;
        if (coords_valid(wl.coords)) fi_keys[v.nfi++] = coords_key(wl.coords.start, wl.coords.stop);
        if (count_has_data) {
            count_bad(v, even_line);
            const Coords preset_coords = preset_behind_unreadable(v, a, lds.lv_keys);
            v.field_state = FIELD_INIT;
            bin_set_data_coordinates(v.bin, preset_coords);
            bin_set_bw_levels(v.bin, ps, 0, 0);
        } else {
            bin_set_bw_levels(v.bin, ps, 0, 0);
        }
    }
    count_line(v, even_line, count_has_pcm, [&v, &wl]() __attribute__((always_inline)) { for (int i = 0; i < 6; i++) v.last_words[i] = get_word(wl, i); });
}

/* ---- the tape plays: lines that read from what their predecessor left preset ----------------------------------------------------------- */
#ifndef SDV_P1_BATCH
#define SDV_P1_BATCH 1              /* runs of lines that read from one tuning take batch1, single ones lean_line1 */
#endif
#ifndef SDV_P1_CAPTURE_D
#define SDV_P1_CAPTURE_D 8          /* batch1: lines in flight */
#endif
/* The tuning of sdvmf::LeanBase and the pixels a lane samples: cells lane and lane + 64 */
struct Lean1 : LeanBase { uint16_t x0, x1; };
__device__ inline bool lean1_prepare(Lean1 &n, const BinCtx &c, const Bin &b)
{
    return lean_prepare<L1, P1_BITS>(n, c, b, [&n](const L1 &t) {
        const int lane = lane_id();
        n.x0 = (uint16_t)pixel_of(t, lane, 0);
        n.x1 = (uint16_t)pixel_of(t, lane + 64 < P1_BITS ? lane + 64 : P1_BITS - 1, 0);
    });
}
/* one read of a line under the tuning in n: the cells as two masks (cell b = bit b), the CRC over them; false when the CRC does not match
 * or the line is a Header (*header says which: a Header is read, all 94 cells of it - the first rung of the ladder takes it, pick_cut_bits
 * leaves a line alone that is valid, and a Header is valid whatever its CRC, pcm1line.cpp:314-323) */
__device__ inline bool lean_read1(const Lean1 &n, uint8_t p0, uint8_t p1, uint64_t &s_lo, uint64_t &s_hi, u128 &cells, uint16_t &crc, bool *header = nullptr)
{
    const int lane = lane_id();
    const bool second = lane + 64 < P1_BITS;
    const uint64_t a_lo = __ballot(p0 > n.low), b_lo = __ballot(p0 >= n.high);
    const uint64_t a_hi = __ballot(second && p1 > n.low), b_hi = __ballot(second && p1 >= n.high);
    solve_automaton(a_lo, a_hi, b_lo, b_hi, s_lo, s_hi);
    s_hi &= (1ull << (P1_BITS - 64)) - 1ull;
    cells = ((u128)__brevll(s_lo) << 30) | (u128)(__brevll(s_hi) >> 34);
    const uint64_t klo = (lane < 16) ? c_crc1.klo[lane & 15] : 0ull, khi = (lane < 16) ? c_crc1.khi[lane & 15] : 0ull;
    const int par = (__popcll(s_lo & klo) + __popcll(s_hi & khi)) & 1;
    crc = (uint16_t)((uint16_t)(__ballot(par) & 0xFFFF) ^ c_crc1.base);
    L1 t; t.v = cells;
    const bool hdr = has_header(t);
    if (header) *header = hdr;
    if (hdr) return false;
    return crc == (uint16_t)(cells & 0xFFFF);
}
__device__ inline void lean_fill_line1(const Lean1 &n, const FrameArgs &a, const Bin &b, u128 cells, uint16_t crc, L1 &out)
{
    p1_clear(out);
    out.pixel_start = 0; out.pixel_stop = (uint16_t)(a.width - 1);
    out.coords = b.in_coord;
    out.black = b.in_black; out.white = b.in_white; out.bw_set = true;
    out.ref_level = b.in_ref; out.ref_low = n.low; out.ref_high = n.high;
    out.hyst = 0; out.shift = 0;
    out.psm = n.psm; out.hpsm = n.hpsm; out.pso = n.pso;
    out.v = cells; out.calc_crc = crc;
    out.picked_l = n.bits_l; out.picked_r = n.bits_r;
    out.by_ext_tune = true;
}
/* Binarizer::processLine for a line that reads from its presets on the first rung of the ladder: stage STG_INPUT_ALL and nothing else */
__device__ inline bool lean_line1(Lean1 &n, const BinCtx &c, const FrameArgs &a, const Bin &b, const uint8_t *px_row, L1 &out)
{
    if (!lean1_prepare(n, c, b)) return false;
    uint64_t s_lo, s_hi; u128 cells; uint16_t crc; bool header = false;
    if (!lean_read1(n, px_row[n.x0], px_row[n.x1], s_lo, s_hi, cells, crc, &header)) {
        if (!header) return false;
        /* a Header line: read like any line (STG_INPUT_ALL, valid on the first rung), then made a service line (STG_DATA_OK, binarizer.cpp:1534-1621:
         * PCMLine::setServiceLine clears the base class's members - levels, coordinates, flags, the calculated CRC - and leaves the words and the
         * picked bits) */
        lean_fill_line1(n, a, b, cells, crc, out);
        set_service(out, SDV_SRV_HEADER_LINE);
        return true;
    }
    lean_fill_line1(n, a, b, cells, crc, out);
    return true;
}
/* A run of up to 64 lines that all read from the same presets (the pattern of batch16, pcm16_frames_device.h): phase A reads them - two
 * byte gathers per lane straight from the frame, four ballots, the automaton, the CRC - and parks each line's cells in the lane that
 * owns it; phase B does VideoToDigital's per-line bookkeeping (:1115-1634) a lane per line.  Returns the number of lines taken. */
__device__ inline int batch1(V2D1 &w, const FrameArgs &a, WaveLds &lds, const Lean1 &n, const uint8_t *frame, int field, int idx, int nl,
                             uint32_t frame_no, sdv_pcm1_bin_rec *rec, uint32_t *fv_keys, L1 &wl)
{
    V2D &v = w.v;
    const int lane = lane_id();
    if (v.field_state != FIELD_INIT) return 0;
    if ((uint8_t)((uint8_t)(n.psm / 128u) * 3) == 0) return 0;         /* in_delta = getPPB() * 3 as uint8_t: at 0 the damper flags a delta of zero */
    const uint32_t key = coords_key(v.bin.in_coord.start, v.bin.in_coord.stop);
    if (__ballot(lane < v.n_last && lds.lv_keys[lane < COORD_HISTORY_DEPTH ? lane : 0] != key) != 0ull) return 0;
    int n_lines = nl - idx; if (n_lines > 64) n_lines = 64;
    uint32_t m0 = 0, m1 = 0, m2 = 0;
    int n_ok = 0;
    {   /* Phase A, the pattern of the STC-007 capture (stc007_device.h): per line two byte gathers per lane straight from the frame (D lines in
         * flight: a line costs its share of the memory's bandwidth, not one trip to it), four ballots, and the masks parked in the lane that owns the
         * line; then every lane solves its own line - automaton and CRC.  A line that does not read ends the run: what was fetched behind it is
         * fetched again by whatever takes that line. */
        constexpr int D = SDV_P1_CAPTURE_D;
        static_assert(64 % D == 0, "whole groups of D lines make a run of up to 64");
        const uint32_t rs2 = 2u * (uint32_t)a.row_stride;        /* offsets inside a frame fit 32 bits (frame_body1 checks) */
        const uint8_t *row0 = frame + (size_t)(2 * idx + field) * a.row_stride;
        const uint32_t x0 = n.x0, x1 = n.x1, lo = n.low, hi = n.high;
        const bool second = lane + 64 < P1_BITS;
        uint8_t q[D][2];
#pragma unroll
        for (int d = 0; d < D; d++) { const uint32_t o = (uint32_t)(d < n_lines ? d : n_lines - 1) * rs2; q[d][0] = lean_load_u8(row0 + (o + x0)); q[d][1] = lean_load_u8(row0 + (o + x1)); }
        uint32_t ra0 = 0, ra1 = 0, ra2 = 0, rb0 = 0, rb1 = 0, rb2 = 0;
        for (int j0 = 0; j0 < n_lines; j0 += D) {
#pragma unroll
            for (int d = 0; d < D; d++) {
                const int j = j0 + d;
                const uint8_t p0 = q[d][0], p1 = q[d][1];
                const uint64_t a_lo = __ballot(p0 > lo), b_lo = __ballot(p0 >= hi), a_hi = __ballot(second && p1 > lo), b_hi = __ballot(second && p1 >= hi);
                { const int jn = j + D < n_lines ? j + D : n_lines - 1; const uint32_t o = (uint32_t)jn * rs2; q[d][0] = lean_load_u8(row0 + (o + x0)); q[d][1] = lean_load_u8(row0 + (o + x1)); }
                ra0 = write_lane(ra0, (uint32_t)a_lo, j); ra1 = write_lane(ra1, (uint32_t)(a_lo >> 32), j); ra2 = write_lane(ra2, (uint32_t)a_hi, j);
                rb0 = write_lane(rb0, (uint32_t)b_lo, j); rb1 = write_lane(rb1, (uint32_t)(b_lo >> 32), j); rb2 = write_lane(rb2, (uint32_t)b_hi, j);
            }
        }
        uint64_t s_lo, s_hi;
        solve_automaton_lane((uint64_t)ra0 | ((uint64_t)ra1 << 32), (uint64_t)ra2, (uint64_t)rb0 | ((uint64_t)rb1 << 32), (uint64_t)rb2, s_lo, s_hi);
        s_hi &= (1ull << (P1_BITS - 64)) - 1ull;
        const u128 cells = ((u128)__brevll(s_lo) << 30) | (u128)(__brevll(s_hi) >> 34);
        const uint16_t crc = crc_of_masks(s_lo, s_hi);
        L1 t; t.v = cells;
        const bool ok = crc == (uint16_t)(cells & 0xFFFF) && !has_header(t);
        const uint64_t okm = __ballot(ok || lane >= n_lines);
        n_ok = okm == ~0ull ? n_lines : (__ffsll((unsigned long long)~okm) - 1);
        m0 = (uint32_t)s_lo; m1 = (uint32_t)(s_lo >> 32); m2 = (uint32_t)s_hi;
    }
    if (n_ok == 0) return 0;
    /* phase B: lane j = line j of the run */
    const uint64_t my_lo = ((uint64_t)m1 << 32) | m0, my_hi = m2;
    const u128 mine = ((u128)__brevll(my_lo) << 30) | (u128)(__brevll(my_hi) >> 34);
    L1 t; t.v = mine;
    uint16_t wd[6];
#pragma unroll
    for (int k = 0; k < 6; k++) wd[k] = get_word(t, k);
    if (a.check_line_copy) {
        const int src = lane >= 1 ? lane - 1 : 0;
        const uint32_t p0 = (uint32_t)__shfl((int)m0, src), p1 = (uint32_t)__shfl((int)m1, src), p2 = (uint32_t)__shfl((int)m2, src);
        L1 ab; ab.v = ((u128)__brevll(((uint64_t)p1 << 32) | p0) << 30) | (u128)(__brevll((uint64_t)p2) >> 34);
        int diff = 0, silent = 0;
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const uint16_t above = lane == 0 ? v.last_words[k] : get_word(ab, k);
            diff += __popc((uint32_t)(uint8_t)(wd[k] ^ above));
            const int16_t smp = p1_get_sample(wd[k]);
            if (!(smp >= 8) && !(smp < -8)) silent++;
        }
        const uint64_t dup = __ballot(lane < n_ok && !(silent >= 2) && diff <= (P1_BITS / BIT_DIFF_THRES_DIV));
        if (dup) { n_ok = __ffsll((unsigned long long)dup) - 1; if (n_ok == 0) return 0; }
    }
    const bool even_line = field == 1;
    const uint8_t ref = v.bin.in_ref;
    if (lane < n_ok) {
        sdv_pcm1_bin_rec r;
        r.frame_number = frame_no; r.line_number = (uint16_t)(field + 1 + 2 * (idx + lane));
#pragma unroll
        for (int k = 0; k < 6; k++) r.words[k] = wd[k];
        r.words[6] = (uint16_t)(mine & 0xFFFF);
        r.calc_crc = (uint16_t)(mine & 0xFFFF);
        r.data_start = v.bin.in_coord.start; r.data_stop = v.bin.in_coord.stop;
        r.black_level = v.bin.in_black; r.white_level = v.bin.in_white; r.ref_low = n.low; r.ref_level = ref; r.ref_high = n.high;
        r.hysteresis_depth = 0; r.shift_stage = 0; r.service_type = SDV_SRV_NO;
        r.picked_bits_left = n.bits_l; r.picked_bits_right = n.bits_r;
        r.flags = (uint8_t)(SDV_LF_BY_EXT_TUNE | SDV_LF_BW_SET | SDV_LF_CRC_VALID | (a.doubled ? SDV_LF_FROM_DOUBLED : 0));
        r._pad[0] = r._pad[1] = r._pad[2] = 0;
        rec[lane] = r;
        fv_keys[v.nfv + lane] = key;
    }
    v.good_coords_in_field = (uint16_t)(v.good_coords_in_field + n_ok);
    v.q_line_length = (uint16_t)a.width;
    if (!even_line) { v.q_odd = (uint16_t)(v.q_odd + n_ok); v.q_pcm_odd = (uint16_t)(v.q_pcm_odd + n_ok); }
    else { v.q_even = (uint16_t)(v.q_even + n_ok); v.q_pcm_even = (uint16_t)(v.q_pcm_even + n_ok); }
    v.pcm_lines_in_field = (uint16_t)(v.pcm_lines_in_field + n_ok);
    v.line_in_field_cnt = (uint16_t)(v.line_in_field_cnt + n_ok);
    v.nfv += n_ok;
    {
        int fill_to = v.n_last + n_ok; if (fill_to > COORD_HISTORY_DEPTH) fill_to = COORD_HISTORY_DEPTH;
        SDV_WAVE_SYNC();
        if (lane >= v.n_last && lane < fill_to) lds.lv_keys[lane] = key;
        SDV_WAVE_SYNC();
        v.n_last = fill_to;
    }
    {   /* what the last line leaves behind */
        const uint64_t l_lo = ((uint64_t)lane_read32(m1, (uint32_t)(n_ok - 1)) << 32) | lane_read32(m0, (uint32_t)(n_ok - 1)), l_hi = lane_read32(m2, (uint32_t)(n_ok - 1));
        const u128 last = ((u128)__brevll(l_lo) << 30) | (u128)(__brevll(l_hi) >> 34);
        lean_fill_line1(n, a, v.bin, last, (uint16_t)(last & 0xFFFF), wl);
        for (int k = 0; k < 6; k++) v.last_words[k] = get_word(wl, k);
    }
    return n_ok;
}

/* one frame.  kLean: the build without Binarizer::processLine's search stages - a frame with a line the tuning it inherits does not read is given up
 * (its flag says VF_ABORTED) and decoded again by the full build (pcm1_frames_engine.inc); the pattern of the STC-007 frame kernels. */
template <bool kInsane, bool kLean = false>
__device__ inline void frame_body1(const FrameArgs1 &a1, P1Lds &lds, int f)
{
    const FrameArgs &a = a1.f;
    if (kLean && (f == a.end_file_frame || frame_is_empty(a, f))) {          /* frames without pixels: the full build's */
        if (lane_id() == 0) a.flag[f] = VF_ABORTED;
        return;
    }
    V2D1 w; L1 wl;
    v2d1_load_state(w, lds.w, &a.states_in[f], a);
    V2D &v = w.v;
    const uint32_t frame_no = a.first_frame_no + (uint32_t)f;
    const uint8_t *frame = a.luma + (size_t)f * a.frame_stride;
    uint32_t *fv_keys = a.scratch + (size_t)f * 2u * (size_t)a.height;
    uint32_t *fi_keys = fv_keys + a.height;
    sdv_pcm1_bin_rec *rec = a1.recs1 + rec_base(a, f, 1);
    const bool doubled = a.doubled != 0;

    begin_frame(v, w.prescan_ref, a, a1.prescan, lds.w.long_keys, f, [](int, int) {});
    const bool empty_frame = frame_is_empty(a, f);
    Lean1 lean; lean_reset(lean);
    const int n_field[2] = { (a.height + 1) / 2, a.height / 2 };
    /* batch1 forms its offsets inside the frame in 32 bits: taken only where they fit, the rule of the STC-007 capture (stc007_device.h); rows
     * farther apart are staged line by line, at 64-bit addresses */
    const bool near_rows = (uint64_t)a.row_stride * (uint64_t)a.height < (1ull << 31);
    uint16_t line_num = 0;
    if (f == a.new_file_frame) { v2d1_service_line(w, a, wl, SDV_SRV_NEW_FILE); emit_rec(wl, frame_no, 0, false, rec++); }
    for (int field = 0; field < 2; field++) {
        const int nl = n_field[field];
        for (int idx = 0; idx < nl; idx++) {
            line_num = (uint16_t)(field + 1 + 2 * idx);
            if (f == a.end_file_frame) {            /* VideoInFFMPEG::insertDummyFrame(true, false): FILLER lines (vin_ffmpeg.cpp:367-523) */
                v2d1_service_line(w, a, wl, SDV_SRV_FILLER);
                emit_rec(wl, frame_no, line_num, false, rec++);
                continue;
            }
            if (empty_frame) {                      /* a dropped frame: an empty VideoLine comes back as a cleared line (binarizer.cpp:1689-1700), its length counts as 0 */
                p1_clear(wl);
                const uint16_t ql = v.q_line_length;
                v2d1_post_line(w, a, lds.w, wl, fv_keys, fi_keys, (line_num % 2) == 0);
                v.q_line_length = ql;
                emit_rec(wl, frame_no, line_num, false, rec++);
                continue;
            }
            BinCtx c;
            ctx_for_line(a, c, v.bin);
#if SDV_P1_BATCH
            if (near_rows && lean1_prepare(lean, c, v.bin)) {
                const int took = batch1(w, a, lds.w, lean, frame, field, idx, nl, frame_no, rec, fv_keys, wl);
                if (took > 0) { rec += took; idx += took - 1; continue; }
            }
#endif
            stage_row(lds.w.px, frame + (size_t)(2 * idx + field) * a.row_stride, a.width);
            /* :853-884: the real-time modes stop searching once a field has produced enough good lines */
            bool coord_search = true;
            if (a.mode == SDV_MODE_DRAFT || a.mode == SDV_MODE_FAST) coord_search = !(v.good_coords_in_field > 2 || v.pcm_lines_in_field > 2);
            if (!(SDV_P1_BATCH && lean_line1(lean, c, a, v.bin, lds.w.px, wl))) {
                if (kLean) { if (!input_all_p1(c, v.bin, lds.w, wl, doubled)) { if (lane_id() == 0) a.flag[f] = VF_ABORTED; return; } }
                else process_line_p1<kInsane>(c, v.bin, coord_search, lds, wl, doubled);
            }
            v2d1_post_line(w, a, lds.w, wl, fv_keys, fi_keys, (line_num % 2) == 0);
            emit_rec(wl, frame_no, line_num, doubled, rec++);
        }
        line_num = (uint16_t)(field + 1 + 2 * nl);
        v2d1_service_line(w, a, wl, SDV_SRV_END_FIELD);
        emit_rec(wl, frame_no, line_num, false, rec++);
    }
    if (f == a.end_file_frame) {
        line_num = (uint16_t)(line_num + 2);
        v2d1_service_line(w, a, wl, SDV_SRV_END_FILE);
        emit_rec(wl, frame_no, line_num, false, rec++);
    }
    line_num = (uint16_t)(line_num + 2);
    v2d1_service_line(w, a, wl, SDV_SRV_END_FRAME);
    v.q_odd = v.q_even = P1_LINES_PF;                               /* :1638-1642 */
    store_frame_median(a1.frame_med, f, fv_keys, v.nfv);
    v2d_end_frame(v, a, lds.w, frame_no, fv_keys, fi_keys, &a.stats[f]);
    emit_rec(wl, frame_no, line_num, false, rec++);
    v2d1_store_state(w, lds.w, &a.states_out[f], a);
}

} // namespace sdvp1f

#ifndef SDV_P1PRE_WAVES_PER_EU
#define SDV_P1PRE_WAVES_PER_EU SDV_P1B_WAVES_PER_EU
#endif
#ifndef SDV_P1F_LEAN_WAVES_PER_EU
#define SDV_P1F_LEAN_WAVES_PER_EU 4
#endif
SDV_MLF_KERNELS(pcm1, sdvp1f::FrameArgs1, sdvp1b::P1Lds, sdvp1f::prescan_body, sdvp1f::frame_body1, SDV_P1PRE_WAVES_PER_EU, SDV_P1B_WAVES_PER_EU, SDV_P1F_LEAN_WAVES_PER_EU)
