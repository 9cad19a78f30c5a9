/*
 * markerless_chain_device.h - the state model of the chain speculation of the two marker-less frame drivers (PCM-1: pcm1_frames_device.h,
 * PCM-16x0: pcm16_frames_device.h; host side: markerless_frames_engine.inc): prediction of the incoming states from the prescan results,
 * repair of the frames behind broken links, the check of the links after a round.  Written once, on the chain state type S:
 * sdv_v2d_state for PCM-1, State16 (the same with a last-valid window of 27) for PCM-16x0.
 */
#pragma once
#include "pcm1_frames_device.h"
#include "pcm16_frames_device.h"

namespace sdvml {
using namespace sdv;
using sdvmf::PrescanRes;
using sdvmf::prescan_ref_of;
using sdvmf::prescan_runs;
using sdvmf::COORD_CHECK_LINES;
using sdvmf::link_holds;
using sdvmf::v2d_of;
using sdvp16f::v2d_of;
using sdvp16f::State16;
using sdvp16f::LV16;

/* ---- what differs between the formats (v2d_of: with the state types) ------------------------------------------------------- */
/* the window of last valid coordinates: its length, entry i, all of it filled with one pair */
constexpr int last_valid_depth(const sdv_v2d_state *) { return COORD_HISTORY_DEPTH; }
constexpr int last_valid_depth(const State16 *) { return LV16; }
__device__ __forceinline__ sdv_coord last_valid_at(const sdv_v2d_state &s, int i) { return s.last_valid[i]; }
__device__ __forceinline__ sdv_coord last_valid_at(const State16 &s, int i) { return i < COORD_HISTORY_DEPTH ? s.s.last_valid[i] : s.more[i - COORD_HISTORY_DEPTH]; }
__device__ __forceinline__ void fill_last_valid(sdv_v2d_state &p, sdv_coord c)
{
    p.n_last_valid = COORD_HISTORY_DEPTH;
    for (int i = 0; i < COORD_HISTORY_DEPTH; i++) p.last_valid[i] = c;
}
__device__ __forceinline__ void fill_last_valid(State16 &p, sdv_coord c)
{
    p.s.n_last_valid = LV16;
    for (int i = 0; i < COORD_HISTORY_DEPTH; i++) p.s.last_valid[i] = c;
    for (int i = 0; i < LV16 - COORD_HISTORY_DEPTH; i++) p.more[i] = c;
}
/* Is the first prediction of a call the sticky model (predict_state)?  PCM-16x0 has no Header lines: the first line of a field is always
 * marked bad and the worker falls back on its coordinate history behind it, so a stream keeps the coordinates it carries.  A PCM-1 field
 * opens with its Header line, and the frames decode with what their own prescan finds. */
constexpr bool first_prediction_sticky(const sdv_v2d_state *) { return false; }
constexpr bool first_prediction_sticky(const State16 *) { return true; }

/* ---- prediction of the incoming states ------------------------------------------------------------------------------------ */
/* states[k] for the frames behind frame 0, whose state is true: what the worker carries from frame to frame is the coordinate
 * history - the last valid lines (nine; PCM-16x0: 27 parts), the medians of the last sixteen frames - and prescan_ref.  On a tape that
 * plays every line of a frame reads with the coordinates its prescan found, so all of that follows from the prescan results, which are
 * known before any frame is decoded.  DRAFT mode has no prescan: there the state is handed on as it is, like for STC-007. */
template <class S> struct PredictArgs { S *states; const PrescanRes *prescan; FrameArgs f; };

/* the median of a state's window of last valid coordinates (videotodigital.cpp:348-371), or false when it is empty */
template <class S> __device__ inline bool last_valid_median(const S &s0, sdv_coord *out)
{
    constexpr int depth = last_valid_depth((const S *)0);
    const sdv_v2d_state &v0 = v2d_of(s0);
    const int n = v0.n_last_valid > depth ? depth : v0.n_last_valid;
    if (n == 0 || v0.reset_stats) return false;
    uint32_t keys[depth];
    for (int i = 0; i < n; i++) { const sdv_coord cc = last_valid_at(s0, i); keys[i] = coords_key(cc.data_start, cc.data_stop); }
    for (int i = 1; i < n; i++) { const uint32_t x = keys[i]; int j = i; while (j > 0 && keys[j - 1] > x) { keys[j] = keys[j - 1]; j--; } keys[j] = x; }
    out->data_start = key_start(keys[n / 2]); out->data_stop = key_stop(keys[n / 2]);
    return true;
}
/* sticky = the frames in between are taken to decode with the coordinates the stream already carries (the median of the window of
 * last valid coordinates) instead of the ones their own prescan finds: what happens on a tape without Header lines, where the first
 * line of a field is marked bad (:1193-1211) and the worker falls back on its history for the lines behind it (:1431-1451) */
template <class S> __device__ inline S predict_state(const PredictArgs<S> &a, int k, int base, bool sticky)
{
    const S s0 = a.states[base];
    const sdv_v2d_state &v0 = v2d_of(s0);
    S p = s0;
    sdv_v2d_state &pv = v2d_of(p);
    sdv_coord carried; carried.data_start = 0; carried.data_stop = 0;
    const bool use_carried = sticky && last_valid_median(s0, &carried);
    const uint8_t dbl = a.f.doubled;
    int n_long = v0.reset_stats ? 0 : v0.n_long_valid;       /* a worker that starts over clears its histories first (:778-790) */
    sdv_coord lg[COORD_LONG_HISTORY];
    for (int i = 0; i < COORD_LONG_HISTORY; i++) lg[i] = v0.long_valid[i];
    bool touched = false;
    sdv_coord last; last.data_start = 0; last.data_stop = 0;
    uint8_t pref = prescan_ref_of(v0);
    /* only the last sixteen frames in between can still be seen in the history */
    int j0 = base; if (k - j0 > COORD_LONG_HISTORY + 1) j0 = k - (COORD_LONG_HISTORY + 1);
    for (int j = j0; j < k; j++) {
        if (!prescan_runs(a.f, j)) continue;
        uint32_t keys[COORD_CHECK_LINES]; uint8_t refs[COORD_CHECK_LINES]; int n = 0;
        for (int q = 0; q < COORD_CHECK_LINES; q++) {
            const PrescanRes r = a.prescan[(size_t)j * COORD_CHECK_LINES + q];
            if (r.valid) { keys[n] = coords_key(r.start, r.stop); refs[n] = r.ref; n++; }
            if (r.pad[1]) pv.do_ref_lvl_sweep = a.f.mode == SDV_MODE_INSANE ? 1 : 0;
        }
        if (n == 0) continue;
        for (int i = 1; i < n; i++)
            for (int q = i; q > 0; q--) {
                if (keys[q - 1] > keys[q]) { const uint32_t t = keys[q]; keys[q] = keys[q - 1]; keys[q - 1] = t; }
                if (refs[q - 1] > refs[q]) { const uint8_t t = refs[q]; refs[q] = refs[q - 1]; refs[q - 1] = t; }
            }
        last.data_start = key_start(keys[n / 2]); last.data_stop = key_stop(keys[n / 2]);
        if (use_carried) last = carried;
        pref = refs[n / 2];
        touched = true;
        if (n_long == COORD_LONG_HISTORY) { for (int i = 0; i + 1 < COORD_LONG_HISTORY; i++) lg[i] = lg[i + 1]; n_long--; }
        lg[n_long++] = last;
    }
    if (touched) {
        pv.reset_stats = 0;
        fill_last_valid(p, last);
        pv.n_long_valid = (uint8_t)n_long;
        for (int i = 0; i < COORD_LONG_HISTORY; i++) { if (i < n_long) pv.long_valid[i] = lg[i]; else { pv.long_valid[i].data_start = 0; pv.long_valid[i].data_stop = 0; } }
        const uint16_t lm = dbl ? (uint16_t)((1u << COORD_HISTORY_DEPTH) - 1u) : 0, gm = dbl ? (uint16_t)((1u << n_long) - 1u) : 0;
        pv.last_valid_doubled_mask_lo = (uint8_t)(lm & 0xFF); pv.last_valid_doubled_mask_hi = (uint8_t)(lm >> 8);
        pv.long_valid_doubled_mask = gm;
        pv._pad[1] = (uint8_t)(pref ^ 128);
        pv.bin.in_def_start = last.data_start; pv.bin.in_def_stop = last.data_stop; pv.bin.in_def_from_doubled = dbl;
    } else if (!v0.reset_stats && a.f.mode == SDV_MODE_DRAFT) {
        /* DRAFT: the tuning is handed on; a frame that plays fills the histories with the pair it inherited (the STC-007 model) */
        sdv_coord c; c.data_start = v0.bin.in_def_start; c.data_stop = v0.bin.in_def_stop;
        if (v0.bin.in_def_reference >= a.f.preset.min_ref_lvl && (c.data_start != NO_COORD_LEFT && c.data_stop != NO_COORD_RIGHT && c.data_start < c.data_stop)) {
            const int m = k - base;
            pv.bin.in_def_from_doubled = dbl;
            fill_last_valid(p, c);
            const int total = (int)v0.n_long_valid + m;
            const int keep = total > COORD_LONG_HISTORY ? COORD_LONG_HISTORY : total, drop = total - keep;
            for (int i = 0; i < COORD_LONG_HISTORY; i++) {
                const int src = i + drop;
                if (i >= keep) { pv.long_valid[i].data_start = 0; pv.long_valid[i].data_stop = 0; }
                else if (src < (int)v0.n_long_valid) pv.long_valid[i] = v0.long_valid[src];
                else pv.long_valid[i] = c;
            }
            pv.n_long_valid = (uint8_t)keep;
            const uint16_t lm = dbl ? (uint16_t)((1u << COORD_HISTORY_DEPTH) - 1u) : 0, gm = dbl ? (uint16_t)((1u << keep) - 1u) : 0;
            pv.last_valid_doubled_mask_lo = (uint8_t)(lm & 0xFF); pv.last_valid_doubled_mask_hi = (uint8_t)(lm >> 8);
            pv.long_valid_doubled_mask = gm;
        }
    }
    return p;
}
template <class S> __device__ inline void predict_body(const PredictArgs<S> &a, int k)
{
    a.states[k] = predict_state(a, k, 0, first_prediction_sticky((const S *)0));
}

/* Repair of a run of broken links (markerless_frames_engine.inc).  Heads (head[i] == list[i]) take their predecessor's real outcome; they
 * come first in the list and are written by an earlier launch than the others read them.  A frame list[i] further into the run, whose
 * run starts at frame head[i]:
 *   DRAFT mode (the whole tuning is handed on): predicted again from its run's head - or, when that tells nothing new, its own
 *   predecessor's outcome;
 *   the other modes, first attempt (sticky[i]): predicted again from the head with the coordinates the stream carries (predict_state);
 *   later attempts: its own predecessor's outcome (what a frame hands on depends little on what it was handed), except for the
 *   multi-frame history, which only passes through the frames - that is rebuilt from the head's true state and what the frames
 *   since then have pushed themselves, so that one wrong median does not need sixteen rounds to leave the chain. */
template <class S> struct RepairArgs { PredictArgs<S> p; const S *states_out; const int *list, *head; const uint8_t *sticky; const uint2 *frame_med; };
template <class S> __device__ inline void repair_body(const RepairArgs<S> &a, int i)
{
    const int k = a.list[i], h = a.head[i];
    if (h == k) { a.p.states[k] = a.states_out[k - 1]; return; }
    if (a.p.f.mode == SDV_MODE_DRAFT || a.sticky[i]) {
        S p = predict_state(a.p, k, h, a.p.f.mode != SDV_MODE_DRAFT);
        const S cur = a.p.states[k];
        uint32_t x[sizeof(S) / 4], y[sizeof(S) / 4];
        __builtin_memcpy(x, &p, sizeof(p));
        __builtin_memcpy(y, &cur, sizeof(cur));
        bool same = true;
        for (unsigned q = 0; q < sizeof(S) / 4; q++) same = same && (x[q] == y[q]);
        a.p.states[k] = same ? a.states_out[k - 1] : p;
        return;
    }
    S p = a.states_out[k - 1];
    sdv_v2d_state &pv = v2d_of(p);
    const S h_in = a.p.states[h];
    const sdv_v2d_state &hv = v2d_of(h_in);
    int n_long = hv.reset_stats ? 0 : hv.n_long_valid;
    sdv_coord lg[COORD_LONG_HISTORY];
    for (int q = 0; q < COORD_LONG_HISTORY; q++) lg[q] = hv.long_valid[q];
    for (int j = h; j < k; j++) {
        const uint2 m = a.frame_med[j];
        if (!m.y) continue;
        if (n_long == COORD_LONG_HISTORY) { for (int q = 0; q + 1 < COORD_LONG_HISTORY; q++) lg[q] = lg[q + 1]; n_long--; }
        lg[n_long].data_start = key_start(m.x); lg[n_long].data_stop = key_stop(m.x); n_long++;
    }
    pv.n_long_valid = (uint8_t)n_long;
    for (int q = 0; q < COORD_LONG_HISTORY; q++) { if (q < n_long) pv.long_valid[q] = lg[q]; else { pv.long_valid[q].data_start = 0; pv.long_valid[q].data_stop = 0; } }
    pv.long_valid_doubled_mask = a.p.f.doubled ? (uint16_t)((1u << n_long) - 1u) : 0;
    a.p.states[k] = p;
}
/* the links of the chain after a round: flag[k] for k in [0, n - 1) */
template <class S> struct VerifyArgs { FrameArgs f; const S *states_in, *states_out; };
template <class S> __device__ inline void verify_body(const VerifyArgs<S> &a, int k)
{
    a.f.flag[k] = link_holds(a.f, k, a.states_out[k], a.states_in[k + 1]) ? VF_OK : VF_BREAK;
}

} // namespace sdvml

/* The model's kernels, a thread per index of [lo, hi).  The emulator's build runs the same range index by index. */
#ifndef SDV_EMU
#define SDV_CHAIN_KERNEL(NAME, ARGS, BODY) \
__global__ void NAME(ARGS a, int lo, int hi) \
{ \
    const int i = lo + (int)(blockIdx.x * blockDim.x + threadIdx.x); \
    if (i < hi) BODY(a, i); \
}
#else
#define SDV_CHAIN_KERNEL(NAME, ARGS, BODY) \
static inline void NAME(ARGS a, int lo, int hi) { for (int i = lo; i < hi; i++) BODY(a, i); }
#endif
SDV_CHAIN_KERNEL(sdv_k_pcm1_predict, sdvml::PredictArgs<sdv_v2d_state>, sdvml::predict_body)
SDV_CHAIN_KERNEL(sdv_k_pcm1_repair, sdvml::RepairArgs<sdv_v2d_state>, sdvml::repair_body)
SDV_CHAIN_KERNEL(sdv_k_pcm1_verify, sdvml::VerifyArgs<sdv_v2d_state>, sdvml::verify_body)
SDV_CHAIN_KERNEL(sdv_k_pcm16_predict, sdvml::PredictArgs<sdvp16f::State16>, sdvml::predict_body)
SDV_CHAIN_KERNEL(sdv_k_pcm16_repair, sdvml::RepairArgs<sdvp16f::State16>, sdvml::repair_body)
SDV_CHAIN_KERNEL(sdv_k_pcm16_verify, sdvml::VerifyArgs<sdvp16f::State16>, sdvml::verify_body)
