/*
 * markerless_frames_device.h - what the two marker-less frame drivers (PCM-1: pcm1_frames_device.h, PCM-16x0: pcm16_frames_device.h) do in the
 * same way, written once: the geometry of the worker's frame buffer and of the prescan (VideoToDigital::prescanCoordinates, videotodigital.cpp:148-345),
 * the start of a frame, what a service line does to the worker's state, the pieces of the per-line bookkeeping that do not depend on the line type
 * (VideoToDigital::doBinarize :698-1815), the part of the lean tuning that is the same for both, the frame-end median, and the macro that makes a
 * format's five kernels.  The inner loops (batch1, batch16, lean_read1, lean_line1, lean_part16), the state stores and PCM-16x0's hand-over between
 * the parts of a line stay with their format.
 */
#pragma once
#include "pcm1_bin_device.h"

namespace sdvmf {
using namespace sdv;
using sdvp1b::BinCtx;

enum { COORD_CHECK_LINES = 4, COORD_CHECK_PARTS = COORD_CHECK_LINES + 2 };      /* videotodigital.h:101-102 */

struct PrescanRes { int16_t start, stop; uint8_t ref, valid, pad[2]; };         /* one prescan line: the coordinates and level it read valid with */
/* pad[0] (PCM-16x0): VideoLine::scan_done after the prescan read.
 * pad[1]: the line found levels, i.e. it went through binarizer.cpp:1104 and left Binarizer::do_ref_lvl_sweep at "the mode is MODE_INSANE".
 * That member is the one thing a prescan line takes over from whatever the Binarizer did before (it enters the level validation, :3409),
 * and it only matters when min_valid_crcs > min_contrast: then every prescan line is decoded for both values of it (second half of the
 * array) and the frame picks, line after line, the variant its own flag calls for. */
__device__ __forceinline__ bool sweep_flag_matters(const sdv_bin_preset &ps) { return ps.min_valid_crcs > ps.min_contrast; }

/* sdv_v2d_state::_pad[1] carries prescan_ref (videotodigital.cpp:703, 730: a local of the worker, 128 at its start) as its distance
 * from 128, so that an all-zero pad is the fresh worker for every format */
__device__ __forceinline__ uint8_t prescan_ref_of(const sdv_v2d_state &s) { return (uint8_t)(s._pad[1] ^ 128); }

/* lines in the frame buffer of frame f (waitForOneFrame, :84-145): the rows, END_FIELD twice, END_FRAME, the NEW_FILE line in
 * front of a file's first frame, END_FILE in the filler frame behind its last */
__device__ __forceinline__ int frame_buf_lines(const FrameArgs &a, int f) { return a.height + 3 + (f == a.new_file_frame ? 1 : 0) + (f == a.end_file_frame ? 1 : 0); }
/* does the worker prescan frame f? (prescanCoordinates :171-200, called in every mode but DRAFT, :796-801) */
__device__ __forceinline__ bool prescan_runs(const FrameArgs &a, int f)
{
    return !a.preset.en_force_coords && a.mode != SDV_MODE_DRAFT && frame_buf_lines(a, f) > COORD_CHECK_PARTS;
}
/* row of the picture at index i of frame f's buffer, or -1 for a service line */
__device__ inline int frame_buf_row(const FrameArgs &a, int f, int i)
{
    if (f == a.end_file_frame) return -1;                   /* FILLER lines carry no pixels */
    if (frame_is_empty(a, f)) return -1;                    /* nor do the lines of a dropped frame */
    if (f == a.new_file_frame) { if (i == 0) return -1; i--; }
    const int n0 = (a.height + 1) / 2, n1 = a.height / 2;
    if (i < n0) return 2 * i;
    i -= n0 + 1;
    if (i >= 0 && i < n1) return 2 * i + 1;
    return -1;
}

__device__ inline void ctx_for_line(const FrameArgs &a, BinCtx &c, Bin &b)
{
    c.ps = a.preset; c.mode = a.mode; c.scan_start = 0; c.scan_end = (uint16_t)(a.width - 1);
    c.force_bit_picker = true;      /* binarizer.cpp:82 */
    bin_set_mode(b, a.mode);
    b.scan_start = c.scan_start; b.scan_end = c.scan_end; b.vl_doubled = a.doubled != 0;
}

#ifdef SDV_EMU
__device__ __forceinline__ uint8_t lean_load_u8(const uint8_t *p) { return *p; }
__device__ inline uint32_t lane_read32(uint32_t x, uint32_t idx) { return (uint32_t)__shfl((int)x, (int)idx); }
#else
__device__ __forceinline__ uint8_t lean_load_u8(const uint8_t *p) { return __builtin_nontemporal_load(p); }      /* read once */
__device__ inline uint32_t lane_read32(uint32_t x, uint32_t idx) { return (uint32_t)__builtin_amdgcn_readlane((int)x, (int)uniu(idx)); }
#endif

/* ---- the chain state: sdv_v2d_state (PCM-1) or a struct that begins with one (PCM-16x0: State16, which brings its own v2d_of) ----------- */
__device__ __forceinline__ sdv_v2d_state &v2d_of(sdv_v2d_state &s) { return s; }
__device__ __forceinline__ const sdv_v2d_state &v2d_of(const sdv_v2d_state &s) { return s; }

/* Was frame f+1 started from what frame f handed on?  Like for STC-007 (byte for byte), with one difference: when the worker
 * prescans frame f+1 it resets its Binarizer first (prescanCoordinates :221), so what frame f left preset there does not reach
 * frame f+1 and does not count. */
template <class S> __device__ inline bool link_holds(const FrameArgs &a, int f, const S &out, S next_in)
{
    if (prescan_runs(a, f + 1)) v2d_of(next_in).bin = v2d_of(out).bin;
    uint32_t x[sizeof(S) / 4], y[sizeof(S) / 4];
    __builtin_memcpy(x, &out, sizeof(out));
    __builtin_memcpy(y, &next_in, sizeof(next_in));
    bool same = true;
    for (unsigned i = 0; i < sizeof(S) / 4; i++) same = same && (x[i] == y[i]);
    return same;
}

/* ---- the frame wave -------------------------------------------------------------------------------------------------------- */
/* :772-822 start-of-frame work, with the prescan results of this frame.  note(k, variant): which variant prescan line k was taken from */
template <class Note>
__device__ inline void begin_frame(V2D &v, uint8_t &prescan_ref, const FrameArgs &a, const PrescanRes *prescan, const uint32_t *long_keys, int f, Note note)
{
    v.field_state = FIELD_NEW;
    v.good_coords_in_field = v.pcm_lines_in_field = 0;
    if (v.reset_stats) {
        v.reset_stats = false;
        v.n_last = v.nfv = v.nfi = v.n_long = 0;
        coords_clear(v.frame_avg);
        bin_set_good_parameters_reset(v.bin, a.preset);
    }
    coords_clear(v.frame_avg);
    if (!a.preset.en_force_coords) {
        if (prescan_runs(a, f)) {
            bin_set_good_parameters_reset(v.bin, a.preset);                             /* :221 */
            /* the lines that read valid, sorted like std::sort under CoordinatePair::operator< / by level; the middle ones (:322-336) */
            uint32_t keys[COORD_CHECK_LINES]; uint8_t refs[COORD_CHECK_LINES]; int n = 0;
            for (int k = 0; k < COORD_CHECK_LINES; k++) {
                const int variant = (sweep_flag_matters(a.preset) && v.bin.do_ref_lvl_sweep) ? 1 : 0;
                note(k, variant);
                const PrescanRes r = prescan[((size_t)variant * a.n_total + f) * COORD_CHECK_LINES + k];
                if (uni(r.valid)) { keys[n] = uniu(coords_key(r.start, r.stop)); refs[n] = (uint8_t)uni(r.ref); n++; }
                if (uni(r.pad[1])) v.bin.do_ref_lvl_sweep = a.mode == SDV_MODE_INSANE;
            }
            for (int i = 1; i < n; i++)
                for (int j = i; j > 0; j--) {
                    if (keys[j - 1] > keys[j]) { const uint32_t t = keys[j]; keys[j] = keys[j - 1]; keys[j - 1] = t; }
                    if (refs[j - 1] > refs[j]) { const uint8_t t = refs[j]; refs[j] = refs[j - 1]; refs[j - 1] = t; }
                }
            if (n > 0) { v.frame_avg = key_to_coords(keys[n / 2], a.doubled != 0); prescan_ref = refs[n / 2]; }
        }
        if (!coords_valid(v.frame_avg)) { uint32_t k; if (median_keys(long_keys, v.n_long, &k)) v.frame_avg = key_to_coords(k, a.doubled != 0); }
        else v.bin.in_ref = prescan_ref;                                                /* setReferenceLevel(prescan_ref) */
        if (coords_valid(v.frame_avg)) bin_set_data_coordinates2(v.bin, v.frame_avg.start, v.frame_avg.stop);
    }
}

template <class L> __device__ inline void set_good_parameters(Bin &b, const sdv_bin_preset &ps, const L &l)   /* binarizer.cpp:353-377 */
{
    if (crc_valid_ignore_forced(l)) { b.in_ref = l.ref_level; bin_set_data_coordinates(b, l.coords); bin_set_bw_levels(b, ps, l.black, l.white); }
}

/* what a service line does to the worker's state: Binarizer::processLine :539-568 + VideoToDigital :1006-1114 (the line object and the words of the
 * last line are the format's) */
__device__ __forceinline__ void service_state(V2D &v, const FrameArgs &a, uint8_t srv)
{
    if (srv == SDV_SRV_NEW_FILE || srv == SDV_SRV_END_FILE) {
        v.line_in_field_cnt = 0;
        v.n_last = v.nfv = v.nfi = v.n_long = 0;
        if (srv == SDV_SRV_END_FILE || !coords_valid(v.frame_avg)) bin_set_good_parameters_reset(v.bin, a.preset);
    } else if (srv == SDV_SRV_END_FIELD) {
        v.field_state = FIELD_NEW;
        v.line_in_field_cnt = 0;
        v.good_coords_in_field = 0; v.pcm_lines_in_field = 0;
    }
}

/* a pair of valid coordinates enters the window of the last DEPTH (9 lines; PCM-16x0: 27 parts).  The window moves up by one when it is full:
 * every lane carries one entry (no serial chain through LDS) */
template <int DEPTH> __device__ __forceinline__ void push_last_valid(uint32_t *keys, V2D &v, uint32_t key)
{
    SDV_WAVE_SYNC();
    {
        const int ln = lane_id();
        const bool full = v.n_last == DEPTH;
        const uint32_t moved = (full && ln < DEPTH - 1) ? keys[ln + 1] : 0u;
        SDV_WAVE_SYNC();
        if (full && ln < DEPTH - 1) keys[ln] = moved;
        if (ln == 0) keys[full ? DEPTH - 1 : v.n_last] = key;
    }
    if (v.n_last < DEPTH) v.n_last++;
    SDV_WAVE_SYNC();
}

/* the coordinate damper (:1275-1330): "force bad" for a line whose coordinates are further than three cells from the window's median */
template <class L> __device__ __forceinline__ bool damper_forces_bad(const V2D &v, const FrameArgs &a, const uint32_t *lv_keys, const L &wl)
{
    bool bad = false;
    if (a.coordinate_damper && !a.preset.en_force_coords && (v.n_last > (COORD_HISTORY_DEPTH / 2))) {
        Coords target; coords_clear(target);
        uint32_t k;
        if (median_keys(lv_keys, v.n_last, &k)) target = key_to_coords(k, false);
        if (!coords_valid(target)) target = v.frame_avg;
        if (coords_valid(target)) {
            const int16_t ds = (int16_t)(wl.coords.start - target.start), de = (int16_t)(wl.coords.stop - target.stop);
            const uint8_t in_delta = (uint8_t)(get_ppb(wl) * 3);
            if (((int)ds <= -(int)in_delta) || ((int)ds >= (int)in_delta) || ((int)de <= -(int)in_delta) || ((int)de >= (int)in_delta)) bad = true;
        }
    }
    return bad;
}

/* the coordinates the worker presets behind a line that has data but does not read (:1431-1451) */
__device__ __forceinline__ Coords preset_behind_unreadable(const V2D &v, const FrameArgs &a, const uint32_t *lv_keys)
{
    Coords preset_coords; coords_clear(preset_coords);
    if (!a.preset.en_force_coords) {
        uint32_t k;
        if (median_keys(lv_keys, v.n_last, &k)) preset_coords = key_to_coords(k, a.doubled != 0);
        if (!coords_valid(preset_coords)) preset_coords = v.frame_avg;
    }
    return preset_coords;
}

/* FrameBinDescriptor's counters, by the field of the line */
__device__ __forceinline__ void count_dup(V2D &v, bool even_line) { if (!even_line) v.q_dup_odd++; else v.q_dup_even++; }
__device__ __forceinline__ void count_bad(V2D &v, bool even_line) { if (!even_line) v.q_bad_odd++; else v.q_bad_even++; }
/* the end of the per-line bookkeeping; keep_words(): the format's copy of the words of the last line with PCM in it */
template <class KeepWords> __device__ __forceinline__ void count_line(V2D &v, bool even_line, bool has_pcm, KeepWords keep_words)
{
    if (!even_line) v.q_odd++; else v.q_even++;
    if (has_pcm) {
        if (!even_line) v.q_pcm_odd++; else v.q_pcm_even++;
        v.pcm_lines_in_field++;
        keep_words();
    }
    v.line_in_field_cnt++;
}

/* ---- the tape plays: lines that read from what their predecessor left preset ----------------------------------------------------------- */
/* What depends on the tuning only and not on the format: the levels with their clipping test, the cells the picture cuts off at either end
 * (pickCutBitsUpPCM1 / PCM16X0, binarizer.cpp:6116-7013), the line's pixel scale.  Kept while the tuning stays the same (on a tape that plays:
 * for the whole frame); a format adds the pixels its lanes sample. */
struct LeanBase {
    uint32_t key_coords, key_levels;        /* what the rest was computed for; key_levels = 0xFFFFFFFF: nothing yet */
    uint8_t low, high, bits_l, bits_r;
    bool usable;
    uint32_t psm, hpsm; int16_t pso;
};
__device__ inline void lean_reset(LeanBase &n) { n.key_levels = 0xFFFFFFFFu; n.key_coords = 0; n.usable = false; }
/* true when lines can be read the lean way under the tuning in b (and n describes that tuning).  L: the line type, BITS: its cells;
 * place_x(t), called when the tuning is new: the format's pixel positions, from a line t that carries the scale */
template <class L, int BITS, class PlaceX>
__device__ inline bool lean_prepare(LeanBase &n, const BinCtx &c, const Bin &b, PlaceX place_x)
{
    if (c.ps.en_force_coords) return false;
    if (!(are_bw_levels_preset(b, c.ps) && is_ref_level_preset(b, c.ps) && coords_valid(b.in_coord))) return false;
    if (!(b.in_ref < b.in_white && b.in_ref > b.in_black)) return false;
    if (!(c.scan_end > c.scan_start && BITS <= (c.scan_end - c.scan_start))) return false;
    const uint32_t kc = coords_key(b.in_coord.start, b.in_coord.stop), kl = (uint32_t)b.in_black | ((uint32_t)b.in_white << 8) | ((uint32_t)b.in_ref << 16) | ((uint32_t)(b.in_coord.doubled ? 1 : 0) << 24);
    if (kc != n.key_coords || kl != n.key_levels) {
        n.key_coords = kc; n.key_levels = kl;
        L t;
        t.pixel_start = c.scan_start; t.pixel_stop = c.scan_end;
        set_ppb(t, b.in_coord);
        n.psm = t.psm; n.hpsm = t.hpsm; n.pso = t.pso;
        place_x(t);
        n.low = get_low_level(b.in_ref, 0); n.high = get_high_level(b.in_ref, 0);
        n.usable = !(n.low <= b.in_black) && !(n.high >= b.in_white);
        for (int side = 0; side < 2; side++) {
            const bool left = side == 0;
            int max_cut = left ? c.ps.left_bit_pick : c.ps.right_bit_pick; if (c.mode == SDV_MODE_DRAFT) max_cut /= 2;
            int first = left ? c.scan_start : c.scan_end, bits = 0;
            const int half_ppb = ((int)get_ppb(t) + 1) / 2;
            for (int i = 0; i < max_cut; i++) {
                const int cur = pixel_of(t, left ? i : BITS - 1 - i, 0);
                if ((left ? (cur - first) : (first - cur)) >= half_ppb) break;
                if (i == 0) first = cur;
                bits = i + 1;
            }
            if (left) n.bits_l = (uint8_t)bits; else n.bits_r = (uint8_t)bits;
        }
    }
    return n.usable && c.force_bit_picker;
}

/* ---- the frame's records and its end ------------------------------------------------------------------------------------------------ */
/* the first record of frame f: lines_per_row * height + 3 records per frame, one more behind the NEW_FILE frame */
__device__ __forceinline__ size_t rec_base(const FrameArgs &a, int f, int lines_per_row)
{
    size_t base = (size_t)f * (size_t)(lines_per_row * a.height + 3);
    if (a.new_file_frame >= 0 && f > a.new_file_frame) base += 1;
    return base;
}
/* the median of the frame's valid coordinates is what v2d_end_frame pushes into long_valid_coords (:1668-1682); frame_med[f] = {key, 1} or {0, 0} (nothing) */
__device__ __forceinline__ void store_frame_median(uint2 *frame_med, int f, const uint32_t *fv_keys, int nfv)
{
    __syncthreads();        /* (keys stored to global memory by other lanes than the ones that read them now) */
    uint32_t mk = 0; bool pushed = median_keys(fv_keys, nfv, &mk);
    if (pushed) { const Coords mc = key_to_coords(mk, false); pushed = coords_valid(mc); }
    if (lane_id() == 0) { uint2 m; m.x = pushed ? mk : 0u; m.y = pushed ? 1u : 0u; frame_med[f] = m; }
}

} // namespace sdvmf

/* The five kernels of a format: two builds of prescan and frames_bin - MODE_INSANE (with the reference level sweep) and every other mode - and the lean
 * build of the frame kernel (every mode: what it holds - lines that read from what they inherit - is the same in all of them).
 * PRESCAN_BODY<kInsane>(args, lds, f, k) is the format's prescan line, FRAME_BODY<kInsane, kLean>(args, lds, f) its frame. */
#define SDV_MLF_PRESCAN_KERNEL(NAME, ARGS, LDS, PRESCAN_BODY, INSANE, WAVES) \
__global__ void __launch_bounds__(64, WAVES) NAME(ARGS a) \
{ \
    __shared__ LDS lds; \
    const int i = (int)blockIdx.x, f = a.f.frame_list ? a.f.frame_list[i / sdvmf::COORD_CHECK_LINES] : a.f.frame_lo + i / sdvmf::COORD_CHECK_LINES; \
    PRESCAN_BODY<INSANE>(a, lds, f, i % sdvmf::COORD_CHECK_LINES); \
}
#define SDV_MLF_FRAME_KERNEL(NAME, ARGS, LDS, FRAME_BODY, INSANE, LEAN, WAVES) \
__global__ void __launch_bounds__(64, WAVES) NAME(ARGS a) \
{ \
    __shared__ LDS lds; \
    const int f = a.f.frame_list ? a.f.frame_list[blockIdx.x] : a.f.frame_lo + (int)blockIdx.x; \
    FRAME_BODY<INSANE, LEAN>(a, lds, f); \
}
#define SDV_MLF_KERNELS(FMT, ARGS, LDS, PRESCAN_BODY, FRAME_BODY, PRESCAN_WAVES, BIN_WAVES, LEAN_WAVES) \
SDV_MLF_PRESCAN_KERNEL(sdv_k_##FMT##_prescan, ARGS, LDS, PRESCAN_BODY, false, PRESCAN_WAVES) \
SDV_MLF_FRAME_KERNEL(sdv_k_##FMT##_frames_bin, ARGS, LDS, FRAME_BODY, false, false, BIN_WAVES) \
SDV_MLF_PRESCAN_KERNEL(sdv_k_##FMT##_prescan_insane, ARGS, LDS, PRESCAN_BODY, true, PRESCAN_WAVES) \
SDV_MLF_FRAME_KERNEL(sdv_k_##FMT##_frames_bin_insane, ARGS, LDS, FRAME_BODY, true, false, BIN_WAVES) \
SDV_MLF_FRAME_KERNEL(sdv_k_##FMT##_frames_lean, ARGS, LDS, FRAME_BODY, false, true, LEAN_WAVES)
