/*
 * engine.inc - host side of the decode engine behind the C-ABI of include/sdvpcm.h.
 *
 * Included by exactly one translation unit per build:
 *   - sdvpcm_hip.hip   (product; rt:: = HIP runtime, kernels launched on the GPU)
 *   - tests/emu/emu_engine.cpp (tests only; rt:: = malloc/memcpy + the SIMT emulator)
 * so that the chain-speculation logic below is the same code in both.  What differs between the two - memory, copies, kernel launches, events,
 * streams, the launch sizes - is namespace rt in runtime.inc; this file and the engines behind it name the build only for the __global__ wrappers
 * of the kernels defined here, the device probe of sdv_engine_create and sdv_debug_k1_cycles.
 *
 * Chain speculation (DESIGN.md): the reference decodes a stream strictly line after line because
 * every good line re-tunes the binarizer for the next one (videotodigital.cpp:1369).  All of that
 * feedback is captured by sdv_v2d_state.  The engine decodes the frames of a batch in parallel,
 * each from a *predicted* incoming state (steady-state model: a clean frame leaves the tuning
 * untouched), then checks on the device that every frame's real outgoing state equals the state its
 * successor was started from.  Frames up to the first mismatch are final.  Every place where the chain does not
 * hold becomes an anchor for the next round: the frame behind it takes its predecessor's real outgoing state, the
 * frames up to the next anchor are predicted from there, and all of them are decoded again at once - a lost line
 * re-tunes the binarizer from the pixels that follow it, whatever the tuning was before, so on a damaged tape the
 * anchors are usually right and the number of rounds does not grow with the number of dropouts.  Frames a lean
 * wave gave up are decoded by the full kernel, all of them in one launch.  The loop ends when the whole chain
 * verifies, so the result is always identical to the sequential reference order; only the amount of parallelism
 * depends on the video.  (The STC-007 frame entry and its scheduler: stc007_frames_engine.inc, stc007_chain_plan.h; the marker-less formats':
 * markerless_frames_engine.inc.)
 */

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "ingest_device.h"          /* sdv_k_ingest (sdv_ingest_frames, ingest_engine.inc) */
#include "encode_device.h"          /* sdv_k_encode_words, sdv_k_encode_raster (sdv_encode_frames, encode_engine.inc) */
#include "encode_packed_device.h"   /* sdv_k_encode_raster_packed (the encoders' out_fmt other than SDV_PIX_GRAY8, encode_engine.inc) */
#include "encode_markerless_device.h"   /* sdv_k_mlenc_pcm1_words, sdv_k_mlenc_pcm16_words (sdv_encode_markerless_frames, encode_markerless_engine.inc) */
#include "pcm_preemph_device.h"     /* sdv_k_preemph (sdv_pcm_preemphasis, pcm_condition_engine.inc) */
#include "pcm_resample_device.h"    /* sdv_k_pcmrs (sdv_pcm_resample, pcm_condition_engine.inc) */
#include "runtime.inc"              /* namespace rt: memory, copies, launches, events and streams, for either build */

/* Developer aids (scheduler traces, cycle stamps, launch-shape overrides) are read from the environment only in builds made with
 * -DSDV_DEV_AIDS (build.py: SDVPCM_DEV_AIDS=1, and the test-only emulator build); the product library does not look at the environment. */
#ifdef SDV_DEV_AIDS
static inline const char *dev_env(const char *name) { return getenv(name); }
#else
static inline const char *dev_env(const char *) { return NULL; }
#endif

namespace sdv {

/* ---- model + verification kernels ---------------------------------------------------------- */
struct PredictArgs { sdv_v2d_state *states; int first, hi; uint8_t doubled, min_ref_lvl; const int *first_of; /* per frame of [first, hi): the anchor it is predicted from (NULL: `first`) */
                     uint8_t *skip; const uint8_t *flag; /* (repair rounds) skip[k] = 1: the model gives frame k the state it was last decoded from, and that decode ran to the end of the frame */ };

/* states[k] for k in (first, hi) from states[first]: "every line of the frames in between decodes with
 * the inherited tuning" => presets unchanged, coordinate history saturated with the same pair (predict_state, stc007_device.h). */
__device__ inline void predict_body(const PredictArgs &a, int k)
{
    const int base = a.first_of ? a.first_of[k - a.first] : a.first;
    if (base == k) return;                          /* an anchor: its state has been set from its predecessor's outcome */
    const sdv_v2d_state nw = predict_state(a.states[base], k - base, a.doubled != 0, a.min_ref_lvl);
    if (a.skip) {
        /* A round decodes every frame behind an anchor that changed again; beyond the reach of the histories (16 frames) the model gives most of them
         * the state they had the last time.  Decoding such a frame again can only give what is there (the frame kernels look at nothing else: stc007_device.h,
         * v2d_relink) - unless its last decode did not get to the end of the frame (given up, or waiting for a sweep: VF_ABORTED). */
        const uint32_t *x = reinterpret_cast<const uint32_t *>(&nw), *y = reinterpret_cast<const uint32_t *>(&a.states[k]);
        bool same = true;
        for (unsigned i = 0; i < sizeof(sdv_v2d_state) / 4; i++) same = same && x[i] == y[i];
        if (same) { if ((a.flag[k] & sdv::VF_KIND) != sdv::VF_ABORTED) a.skip[k] = 1; return; }
    }
    a.states[k] = nw;
}

/* integer 2x width doubler (sdv_double_width): a lane takes four source pixels and writes eight */
struct DoubleArgs { const uint8_t *src; size_t src_stride; int width; size_t rows; uint8_t *dst; size_t dst_stride; };
__device__ inline void double_body(const DoubleArgs &a, size_t row, int x4)
{
    const int x = 4 * x4;
    if (row >= a.rows || x >= a.width) return;
    const uint8_t *s = a.src + row * a.src_stride + x;
    uint8_t *d = a.dst + row * a.dst_stride + 2 * (size_t)x;
    const int n = a.width - x < 4 ? a.width - x : 4;
    for (int i = 0; i < n; i++) { const uint8_t v = s[i]; d[2 * i] = v; d[2 * i + 1] = v; }
}

/* anchors: frame list[i] starts from what its predecessor really produced */
struct AnchorArgs { sdv_v2d_state *states_in; const sdv_v2d_state *states_out; const int *list; int n; uint8_t *flag; };
__device__ inline void anchor_body(const AnchorArgs &a, int i) { const int f = a.list[i]; a.states_in[f] = a.states_out[f - 1]; a.flag[f - 1] = VF_OK; /* the link holds now */ }
/* ... with another reference level than its predecessor handed on the last time: the level the predecessor is expected to hand on this time.
 * patch[i] = frame | level << 24 */
/* The history moves on.  The 16-frame coordinate history is a shift register: a frame pushes the pair it measured and hands the rest on one slot
 * down.  The model gives the frames behind an anchor a history full of one pair; what they really get is the anchor's history moved on frame by
 * frame - after a jump of the data window the old pairs leave it one per frame, and a round would find that out one frame at a time.  So behind
 * every anchor of the round the history is moved on along the chain (newest slot: what the state already holds - the model's guess, or what the
 * predecessor pushed the last time), through frames that pushed one pair the last time (refs[3f + 2]), until it meets what is there already.
 * A thread per anchor walks the chain behind it, up to the frame in front of the next anchor (whose state is what its predecessor really handed on:
 * left alone); frames whose start state changed are marked for the host.  (Through round 3 one thread walked all anchors in order - 1 900 anchors on a
 * tape with damage in every frame: up to 5 ms per round.) */
struct HistCarryArgs { sdv_v2d_state *states_in; const uint8_t *refs; const int *anchors; int n_anchors, hi; uint8_t *patched; uint8_t *skip; };
__device__ inline void hist_carry_body(const HistCarryArgs &a, int ai)
{
    if (ai >= a.n_anchors) return;
    const int stop = ai + 1 < a.n_anchors ? a.anchors[ai + 1] : a.hi;       /* states_in[stop] is not written here */
    for (int j = a.anchors[ai]; j + 1 < stop; j++) {
        if (!a.refs[3 * j + 2]) break;
        const sdv_v2d_state &me = a.states_in[j];
        sdv_v2d_state &nx = a.states_in[j + 1];
        if (!(me.n_long_valid == COORD_LONG_HISTORY && nx.n_long_valid == COORD_LONG_HISTORY && me.long_valid_doubled_mask == 0 && nx.long_valid_doubled_mask == 0)) break;
        bool changed = false;
        for (int i = 0; i + 1 < COORD_LONG_HISTORY; i++) {
            const sdv_coord c = me.long_valid[i + 1];
            if (nx.long_valid[i].data_start != c.data_start || nx.long_valid[i].data_stop != c.data_stop) { nx.long_valid[i] = c; changed = true; }
        }
        if (!changed) break;
        a.patched[j + 1] = 1;
        if (a.skip) a.skip[j + 1] = 0;
    }
}
struct RefPatchArgs { sdv_v2d_state *states_in; const uint32_t *patch; int n; };
__device__ inline void ref_patch_body(const RefPatchArgs &a, int i) { const uint32_t p = a.patch[i]; a.states_in[p & 0x00FFFFFFu].bin.in_def_reference = (uint8_t)(p >> 24); }

} // namespace sdv

#ifndef SDV_EMU
__global__ void sdv_k_predict(sdv::PredictArgs a)
{
    int k = a.first + (a.first_of ? 0 : 1) + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k < a.hi) sdv::predict_body(a, k);
}
__global__ void sdv_k_hist_carry(sdv::HistCarryArgs a) { sdv::hist_carry_body(a, (int)(blockIdx.x * blockDim.x + threadIdx.x)); }
__global__ void sdv_k_ref_patch(sdv::RefPatchArgs a)
{
    int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < a.n) sdv::ref_patch_body(a, i);
}
__global__ void sdv_k_double_width(sdv::DoubleArgs a)
{
    sdv::double_body(a, (size_t)blockIdx.y, (int)(blockIdx.x * blockDim.x + threadIdx.x));
}
__global__ void sdv_k_anchor(sdv::AnchorArgs a)
{
    int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < a.n) sdv::anchor_body(a, i);
}
#endif

/* ---- launches of this file's kernels (runtime.inc: the two ways a kernel is launched) --------------- */
/* The frame kernel's builds: lean, the one that settles its sweeps itself (a small round: the sweeps it misses are settled while it runs), with trajectory
 * snapshots, without (no snapshots in this call: sdv_engine::plain_general).  dev_count_frames below mirrors the choice. */
static inline rt::status_t launch_frames(const sdv::FrameArgs &a, rt::stream_t s, bool lean, int list_n = 0)
{
    const int n = a.frame_list ? list_n : a.frame_hi - a.frame_lo;
    if (n <= 0) return rt::OK;
    if (lean) return rt::launch_waves(sdv_k_stc007_frames_lean, (size_t)n, 1, a, s);
    if (a.fat_levels) return rt::launch_waves(sdv_k_stc007_frames_fat, (size_t)n, 1 + sdv::FAT_WORKERS, a, s);
    if (a.tc_hdr) return rt::launch_waves(sdv_k_stc007_frames, (size_t)n, 1, a, s);
    return rt::launch_waves(sdv_k_stc007_frames_plain, (size_t)n, 1, a, s);
}
static inline rt::status_t launch_predict(const sdv::PredictArgs &a, rt::stream_t s)
{
    const int k0 = a.first + (a.first_of ? 0 : 1);
    return RT_LAUNCH_ITEMS(sdv_k_predict, sdv::predict_body, k0, a.hi - k0, 256, s, a);
}

/* ---- engine ---------------------------------------------------------------------------------- */
struct sdv_stitcher;                /* stitch stage state, stitch_engine.inc */
struct sdv_pcm1_stitcher;           /* PCM-1 back half, pcm1_engine.inc */
struct sdv_pcm16_stitcher;          /* PCM-16x0 back half, pcm16_engine.inc */
struct sdv_audio;                   /* AudioProcessor and the stages behind it (audio_engine.inc ...), decode_frames_engine.inc */
struct sdv_vis;                     /* visualiser canvases, vis_engine.inc */
struct sdv_encoder;                 /* the tape sdv_encode_frames writes, encode_engine.inc */
struct sdv_pcm_cond;                /* pre-emphasis and 44 100 -> 44 056 Hz ahead of the encoders, pcm_condition_engine.inc */
struct sdv_engine;
static void stitcher_free(sdv_engine *e);
static void pcm1_free(sdv_engine *e);
static void pcm16_free(sdv_engine *e);
static void audio_free(sdv_engine *e);
static void vis_free(sdv_engine *e);
static void encoder_free(sdv_engine *e);
static void pcm_cond_free(sdv_engine *e);
struct sdv_engine {
    int device = 0;
    std::string last_error;
    sdv_bin_preset preset = {};
    int mode = SDV_MODE_NORMAL;                 /* VideoToDigital ctor, videotodigital.cpp:16 */
    int check_line_dup = 1, coordinate_damper = 1, m2_format = 0;
    sdv_v2d_state chain = {};       /* true state after the last decoded frame of the stream */
    /* device scratch, grown on demand (ensure_capacity: the per-frame buffers grow together) */
    rt::DevBuf<sdv_v2d_state> d_states_in, d_states_out;
    rt::DevBuf<uint32_t> d_scratch;
    rt::PinBuf<uint8_t> h_flag;     /* page-locked mirror of d_flag (the round's read-back queues up behind the kernels) */
    rt::PinBuf<int> h_lists;        /* page-locked staging of the round's lists (lean, full, anchors, first_of, patches: n_frames ints each): copies out of it are queued, not waited for */
    rt::DevBuf<uint8_t> d_refs; rt::PinBuf<uint8_t> h_refs;             /* per frame: reference level in / out, history pushed (3 bytes) */
    rt::DevBuf<uint8_t> d_patched; rt::PinBuf<uint8_t> h_patched;       /* per frame: the history carry gave it another start state (sdv_k_hist_carry) */
    rt::DevBuf<uint8_t> d_skip;                     /* per frame: this round need not decode it again (sdv_k_predict; FrameArgs::skip) */
    rt::DevBuf<uint8_t> d_line_done;                /* sdv_binarize_lines: per line, its record is final */
    rt::DevBuf<uint8_t> d_flag; rt::DevBuf<int> d_first_of, d_list_lean, d_list_full, d_anchors;   /* per frame: flags; a round's lean and full lists (STC-007: both in d_list_lean);
                                     * its anchors, level patches and first_of (STC-007: all three in d_anchors; d_first_of and d_list_full: the PCM-1 / PCM-16x0 frame drivers') */
    /* reference-level sweeps off the frame kernel (stc007_sweep_device.h): pool of requests / outcomes, list head per frame, count; per-level records of a chunk of sweeps */
    rt::DevBuf<sdv::SweepMemo> d_memo; rt::DevBuf<int32_t> d_memo_head, d_memo_count;
    rt::DevBuf<sdv::SweepEnt> d_sweep_levels;       /* (256 records per sweep of a chunk) */
    rt::DevBuf<unsigned long long> d_bw_memo;       /* per line of the batch: what findBlackWhite found there (stc007_device.h, find_black_white) */
    /* trajectory snapshots of the general kernel (stc007_device.h, TcSnap): per frame two sets of snapshots, a header, a second list of coordinate keys */
    rt::DevBuf<sdv::TcSnap> d_tc_snaps; rt::DevBuf<uint32_t> d_tc_hdr, d_tc_keys;
    /* sdv_set_frame_flags: the marks of the next frame entry call (host copy) and their device buffer */
    std::vector<uint8_t> frame_flags; bool frame_flags_pending = false; rt::DevBuf<uint8_t> d_frame_flags;
    /* statistics of the last call */
    sdv_run_info info = {};
    int profiling = 0;
    rt::BounceSlot bounce;          /* page-locked staging of the small synchronous read-backs (rt::d2h) */
    bool worn_tape = false;         /* most frames of the last sdv_binarize_frames call took lines through the general path */
    /* ... and hardly any of their decodes met the frame's last pass (a tape whose damage re-tunes the binarizer for good every few dozen lines): the general
     * kernel's build without the snapshots is a sixth faster there (stc007_device.h, kMeet).  Looked at again with the snapshots every eighth call. */
    bool plain_general = false; unsigned plain_calls = 0;
    sdv_stitcher *stitch = NULL;
    sdv_pcm1_stitcher *pcm1 = NULL;
    /* PCM-16x0 streams: their chain state is longer (pcm16_frames_device.h, State16) */
    sdvp16f::State16 chain16 = {};
    rt::DevBuf<sdvp16f::State16> d_states16_in, d_states16_out;
    rt::DevBuf<uint8_t> d_prescan16;                /* prescan results of the PCM-16x0 frame driver, a median per frame behind them (pcm16_frames_engine.inc) */
    rt::DevBuf<uint8_t> d_sticky16;                 /* per repaired frame: which model (PCM-1 and PCM-16x0 frame drivers) */
    sdv_pcm16_stitcher *pcm16 = NULL;
    sdv_audio *audio = NULL;
    sdv_vis *vis = NULL;
    sdv_encoder *enc = NULL;
    sdv_pcm_cond *cond = NULL;
    rt::Timer timer;                /* sdv_set_profiling: the device time of a call's kernels */
    rt::Event mark;                 /* behind the first round's read-back of sdv_binarize_frames when work of the next stage is queued behind it */
    bool binarize_settled_at_once = false;      /* the last sdv_binarize_frames call of the fused entry needed one round */
#ifdef SDV_DEV_AIDS
    uint32_t dev_counts[16] = {};            /* developer builds: the launches of the last sdv_binarize_frames / sdv_binarize_lines call, by build (DevCount) */
#endif
};

/* Developer builds count, per call, which builds of the frame kernel and the sweep kernels were launched and on how much work (sdv_dev_launch_counts):
 * tests prove with them that a tape reached the build it was made for.  Counted here, in the host code the HIP and the emulator builds share, with the
 * same choice launch_frames makes. */
enum DevCount { DEV_LEAN = 0, DEV_SNAP = 2, DEV_PLAIN = 4, DEV_FAT = 6, DEV_SWEEP_LEVELS = 8, DEV_SWEEP_PICK = 10, DEV_LINES = 12, DEV_N_COUNTS = 14 };
#ifdef SDV_DEV_AIDS
static inline void dev_reset_counts(sdv_engine *e) { memset(e->dev_counts, 0, sizeof(e->dev_counts)); }
static inline void dev_count(sdv_engine *e, int what, size_t work) { e->dev_counts[what]++; e->dev_counts[what + 1] += (uint32_t)work; }     /* launches, then frames / requests / lines */
static inline void dev_count_frames(sdv_engine *e, const sdv::FrameArgs &a, bool lean, int n)
{
    if (n > 0) dev_count(e, lean ? DEV_LEAN : a.fat_levels ? DEV_FAT : a.tc_hdr ? DEV_SNAP : DEV_PLAIN, (size_t)n);
}
#else
static inline void dev_reset_counts(sdv_engine *) {}
static inline void dev_count(sdv_engine *, int, size_t) {}
static inline void dev_count_frames(sdv_engine *, const sdv::FrameArgs &, bool, int) {}
#endif

static thread_local std::string g_last_error;      /* sdv_last_error(NULL): the last failure on the calling thread */
static void set_error(sdv_engine *e, const std::string &msg) { if (e) e->last_error = msg; g_last_error = msg; }

static void chain_reset(sdv_v2d_state *s)
{
    memset(s, 0, sizeof(*s));
    s->bin.in_def_start = sdv::NO_COORD_LEFT; s->bin.in_def_stop = sdv::NO_COORD_RIGHT;
    s->reset_stats = 1;
}

extern "C" {

int sdv_abi_version(void) { return SDV_ABI_VERSION; }

void sdv_default_bin_preset(sdv_bin_preset *p)   /* bin_preset_t::reset, binarizer.cpp:48-65 */
{
    memset(p, 0, sizeof(*p));
    p->max_black_lvl = 160; p->min_white_lvl = 28; p->min_contrast = 10; p->min_ref_lvl = 7; p->max_ref_lvl = 240;
    p->min_valid_crcs = 5; p->mark_max_dist = 6; p->left_bit_pick = 4; p->right_bit_pick = 2;
    p->en_force_coords = 0; p->en_coord_search = 1; p->en_first_line_dup = 1; p->en_good_no_marker = 1;
    p->horiz_start = 0; p->horiz_stop = 0;
}

sdv_engine *sdv_engine_create(int device)
{
#ifndef SDV_EMU
    int count = 0;
    hipError_t err = hipGetDeviceCount(&count);
    if (err != hipSuccess || count <= 0) { set_error(NULL, "sdv_engine_create: no HIP device available (the decode engine has no CPU path)"); return NULL; }
    if (device < 0 || device >= count) { set_error(NULL, "sdv_engine_create: bad device index"); return NULL; }
    { rt::DeviceGuard g(device); if (g.status() != rt::OK) { set_error(NULL, "sdv_engine_create: hipSetDevice failed"); return NULL; } }
#endif
    sdv_engine *e = new sdv_engine();
    e->device = device;
    sdv_default_bin_preset(&e->preset);
    chain_reset(&e->chain);
    chain_reset(&e->chain16.s);
    return e;
}

void sdv_engine_destroy(sdv_engine *e)
{
    if (!e) return;
    rt::DeviceGuard device_guard_(e->device);
    stitcher_free(e);
    pcm1_free(e);
    pcm16_free(e);
    audio_free(e);
    vis_free(e);
    encoder_free(e);
    pcm_cond_free(e);
    delete e;       /* (frees the buffers, the bounce buffer and the events: the guard above is still in place) */
}

const char *sdv_last_error(const sdv_engine *e) { return e ? e->last_error.c_str() : g_last_error.c_str(); }

int sdv_set_bin_preset(sdv_engine *e, const sdv_bin_preset *p)   /* VideoToDigital::setFineSettings, videotodigital.cpp:667-676 */
{
    if (!e || !p) return SDV_ERR_BAD_ARG;
    e->preset = *p;
    e->chain.reset_stats = 1;
    e->chain16.s.reset_stats = 1;
    return SDV_OK;
}
int sdv_needs_double_width(int width) { return width > 10 && width < 959; }       /* MIN_DBL_WIDTH / MAX_DBL_WIDTH (ffmpegwrapper.h:130-131), file sources */
int sdv_double_width(sdv_engine *e, const uint8_t *src, size_t src_row_stride, int width, size_t rows, uint8_t *dst, size_t dst_row_stride, void *stream)
{
    if (!e) return SDV_ERR_BAD_ARG;
    if (rows == 0) return SDV_OK;
    if (!src) { set_error(e, "null video"); return SDV_ERR_NULL_VIDEO; }
    if (!dst) { set_error(e, "null output"); return SDV_ERR_NULL_PCM; }
    if (width <= 0 || src_row_stride < (size_t)width || dst_row_stride < 2 * (size_t)width) { set_error(e, "bad line geometry"); return SDV_ERR_BAD_ARG; }
    SDV_ON_DEVICE(e);
    sdv::DoubleArgs a; a.src = src; a.src_stride = src_row_stride; a.width = width; a.rows = rows; a.dst = dst; a.dst_stride = dst_row_stride;
    const unsigned per_row = (unsigned)((width + 3) / 4);
    for (size_t r0 = 0; r0 < rows; r0 += 65535) {            /* grid.y holds 65 535 rows */
        sdv::DoubleArgs b = a;
        b.src = a.src + r0 * a.src_stride; b.dst = a.dst + r0 * a.dst_stride; b.rows = rows - r0 < 65535 ? rows - r0 : 65535;
        RT_CHECK(RT_LAUNCH_ROWS(sdv_k_double_width, sdv::double_body, b.rows, per_row, 256, (rt::stream_t)stream, b));
    }
    return SDV_OK;
}
int sdv_set_frame_flags(sdv_engine *e, const uint8_t *flags, size_t n)
{
    if (!e || (n > 0 && !flags)) return SDV_ERR_BAD_ARG;
    e->frame_flags.assign(flags, flags + n);
    e->frame_flags_pending = n > 0;
    return SDV_OK;
}
int sdv_set_mode(sdv_engine *e, int mode)   /* VideoToDigital::setBinarizationMode, videotodigital.cpp:607-642 */
{
    if (!e) return SDV_ERR_BAD_ARG;
    if (mode >= SDV_MODE_DRAFT && mode <= SDV_MODE_INSANE) e->mode = mode;
    return SDV_OK;
}
int sdv_set_check_line_dup(sdv_engine *e, int on) { if (!e) return SDV_ERR_BAD_ARG; e->check_line_dup = on != 0; return SDV_OK; }   /* :645-664 */
int sdv_set_pcm_type(sdv_engine *e, int pcm_type, int m2_sample_format)   /* VideoToDigital::setPCMType, :557-604 */
{
    if (!e) return SDV_ERR_BAD_ARG;
    if (pcm_type != SDV_PCM_STC007 && pcm_type != SDV_PCM_PCM1 && pcm_type != SDV_PCM_PCM16X0) { set_error(e, "unknown PCM type"); return SDV_ERR_BAD_ARG; }
    /* the format itself is chosen by the entry point that is called (sdv_binarize_frames / sdv_pcm1_binarize_frames /
     * sdv_pcm16x0_binarize_frames); what the slot does besides is setGoodParameters() + reset_stats */
    e->m2_format = (pcm_type == SDV_PCM_STC007) && m2_sample_format != 0;
    for (sdv_v2d_state *c : { &e->chain, &e->chain16.s }) {
        c->bin.in_def_black = c->bin.in_def_white = c->bin.in_def_reference = 0;
        c->bin.in_def_start = sdv::NO_COORD_LEFT; c->bin.in_def_stop = sdv::NO_COORD_RIGHT; c->bin.in_def_from_doubled = 0;
        c->reset_stats = 1;
    }
    return SDV_OK;
}
int sdv_reset_stream(sdv_engine *e)
{
    if (!e) return SDV_ERR_BAD_ARG;
    chain_reset(&e->chain);
    memset(&e->chain16, 0, sizeof(e->chain16)); chain_reset(&e->chain16.s);
    e->worn_tape = false; e->plain_general = false; e->plain_calls = 0;
    return SDV_OK;
}
int sdv_get_chain_state(const sdv_engine *e, sdv_v2d_state *out) { if (!e || !out) return SDV_ERR_BAD_ARG; *out = e->chain; return SDV_OK; }
int sdv_set_chain_state(sdv_engine *e, const sdv_v2d_state *in) { if (!e || !in) return SDV_ERR_BAD_ARG; e->chain = *in; e->worn_tape = false; return SDV_OK; }
/* the chain state of a PCM-16x0 stream: sdv_v2d_state plus the rest of its 27-entry window of last valid coordinates (192 bytes) */
size_t sdv_pcm16x0_chain_state_size(void) { return sizeof(sdvp16f::State16); }
int sdv_get_pcm16x0_chain_state(const sdv_engine *e, void *out, size_t cap) { if (!e || !out || cap < sizeof(sdvp16f::State16)) return SDV_ERR_BAD_ARG; memcpy(out, &e->chain16, sizeof(e->chain16)); return SDV_OK; }
int sdv_set_pcm16x0_chain_state(sdv_engine *e, const void *in, size_t n) { if (!e || !in || n < sizeof(sdvp16f::State16)) return SDV_ERR_BAD_ARG; memcpy(&e->chain16, in, sizeof(e->chain16)); return SDV_OK; }
int sdv_set_profiling(sdv_engine *e, int on) { if (!e) return SDV_ERR_BAD_ARG; e->profiling = on != 0; return SDV_OK; }
int sdv_get_run_info(const sdv_engine *e, sdv_run_info *out) { if (!e || !out) return SDV_ERR_BAD_ARG; *out = e->info; return SDV_OK; }
#ifdef SDV_DEV_AIDS
/* developer builds: the launch counts of the last call (DevCount: launches and work of the lean, snapshot, plain and five-wave frame kernels, sweep_levels,
 * sweep_pick, stc007_lines passes); copies min(n, DEV_N_COUNTS) of them, returns DEV_N_COUNTS */
int sdv_dev_launch_counts(const sdv_engine *e, uint32_t *out, size_t n)
{
    if (!e || (n > 0 && !out)) return SDV_ERR_BAD_ARG;
    for (size_t i = 0; i < n && i < (size_t)DEV_N_COUNTS; i++) out[i] = e->dev_counts[i];
    return DEV_N_COUNTS;
}
#endif

size_t sdv_records_per_frame(int height) { return (size_t)height + 3; }
size_t sdv_pcm16x0_binarize_records(int height, int n_frames, unsigned flags)
{
    if (height < 0 || n_frames < 0) return 0;
    return (size_t)n_frames * (3 * (size_t)height + 3) + ((flags & SDV_FLAG_NEW_FILE) ? 1 : 0) + ((flags & SDV_FLAG_END_FILE) ? (size_t)height + 4 : 0);
}
size_t sdv_binarize_records(int height, int n_frames, unsigned flags)
{
    if (height < 0 || n_frames < 0) return 0;
    return (size_t)n_frames * ((size_t)height + 3) + ((flags & SDV_FLAG_NEW_FILE) ? 1 : 0) + ((flags & SDV_FLAG_END_FILE) ? (size_t)height + 4 : 0);
}
#if defined(SDV_K1_STAMPS) && !defined(SDV_EMU)
int sdv_debug_k1_cycles(unsigned long long *out24, int reset)
{
    if (hipMemcpyFromSymbol(out24, HIP_SYMBOL(sdv::sdv_k1_cycles), 24 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) { unsigned long long z[24] = { 0 }; if (hipMemcpyToSymbol(HIP_SYMBOL(sdv::sdv_k1_cycles), z, sizeof(z)) != hipSuccess) return -1; }
    return 0;
}
#endif

/* The marks of sdv_set_frame_flags belong to the NEXT frame entry call, whether it succeeds or not (sdvpcm.h): a call that is refused for its
 * geometry or its buffers must not leave them behind for a later, unrelated one - whose frames would silently be decoded as dropped. */
struct FrameFlagsConsumed { sdv_engine *e; explicit FrameFlagsConsumed(sdv_engine *e_) : e(e_) {} ~FrameFlagsConsumed() { if (e) e->frame_flags_pending = false; } };
/* the caller's per-frame marks for this call, on the device (NULL when there are none); consumed */
static int take_frame_flags(sdv_engine *e, size_t n_frames, rt::stream_t s, const uint8_t **out)
{
    *out = NULL;
    if (!e->frame_flags_pending) return SDV_OK;
    e->frame_flags_pending = false;
    e->frame_flags.resize(n_frames, 0);         /* (stays alive until the next sdv_set_frame_flags: the copy below is asynchronous) */
    bool any = false;
    for (size_t i = 0; i < n_frames; i++) any = any || e->frame_flags[i] != 0;
    if (!any) return SDV_OK;
    RT_CHECK(e->d_frame_flags.reserve(n_frames + 64));
    RT_CHECK(rt::h2d(e->d_frame_flags, e->frame_flags.data(), n_frames, s));
    *out = e->d_frame_flags;
    return SDV_OK;
}

/* What every frame entry refuses ahead of its first launch, in this order: no video, no output, the geometry, a line too short for the format, frames that
 * overlap, output buffers too small.  The formats differ in the widest line they take, the narrowest (min_width, with short_line as its refusal), the
 * records a call writes (need_lines) and what they are called (rec_noun). */
static int check_frame_call(sdv_engine *e, const void *luma, const void *out_lines, const void *out_stats, size_t row_stride, size_t frame_stride, int width, int height,
                            int n_frames, unsigned flags, size_t lines_cap, size_t stats_cap,
                            int max_width, int min_width, const char *short_line, size_t need_lines, const char *rec_noun)
{
    if (!luma) { set_error(e, "null video"); return SDV_ERR_NULL_VIDEO; }
    if (!out_lines || !out_stats) { set_error(e, "null output"); return SDV_ERR_NULL_PCM; }
    if (n_frames <= 0 || height < 2 || height > SDV_MAX_HEIGHT || width <= 0 || width > max_width || row_stride < (size_t)width) {
        set_error(e, "bad frame geometry"); return SDV_ERR_BAD_ARG;
    }
    if (width < min_width) { set_error(e, short_line); return SDV_ERR_SHORT_LINE; }
    /* frames must not overlap (the kernels prefetch whole rows of their own frame only) */
    if (n_frames > 1 && frame_stride < (size_t)(height - 1) * row_stride + (size_t)width) { set_error(e, "frame_stride smaller than one frame"); return SDV_ERR_BAD_ARG; }
    const size_t need_stats = (size_t)n_frames + ((flags & SDV_FLAG_END_FILE) ? 1 : 0);
    if (lines_cap < need_lines || stats_cap < need_stats) {
        set_error(e, "output buffers too small: " + std::to_string(need_lines) + " " + rec_noun + " and " + std::to_string(need_stats) + " frame descriptors are needed");
        return SDV_ERR_BAD_ARG;
    }
    return SDV_OK;
}

/* The block a round's one read-back brings (d_flag / h_flag): a flag byte per frame; at the next multiple of 16 the last frame's outgoing state and, behind it,
 * the count of sweep requests and the count of passes that met the frame's last one (16 bytes); then a give-up signature per frame (FrameArgs::sig). */
static inline size_t flag_tail_ofs(size_t n_frames) { return (n_frames + 15) & ~(size_t)15; }
enum : size_t { FLAG_TAIL_BYTES = sizeof(sdv_v2d_state) + 16, FLAG_SIG_OFS = (FLAG_TAIL_BYTES + 15) & ~(size_t)15 };
static inline size_t flag_block_bytes(size_t n_frames) { return flag_tail_ofs(n_frames) + FLAG_SIG_OFS + n_frames + 16; }

static int ensure_capacity(sdv_engine *e, size_t n_frames, size_t height)
{
    RT_CHECK(rt::reserve_all(n_frames, n_frames, e->d_states_in, e->d_states_out));
    RT_CHECK(e->d_flag.reserve(flag_block_bytes(n_frames)));      /* flags, then a copy of the last frame's outgoing state and the count of sweep requests, then the give-up signatures */
    RT_CHECK(e->d_refs.reserve(3 * n_frames)); RT_CHECK(e->h_refs.reserve(3 * n_frames));
    RT_CHECK(e->d_patched.reserve(n_frames)); RT_CHECK(e->h_patched.reserve(n_frames));
    RT_CHECK(e->d_skip.reserve(n_frames));
    RT_CHECK(e->h_flag.reserve(flag_block_bytes(n_frames)));
    RT_CHECK(e->h_lists.reserve(5 * n_frames));
    RT_CHECK(rt::reserve_all(n_frames, n_frames, e->d_first_of, e->d_list_full));
    RT_CHECK(e->d_list_lean.reserve(2 * n_frames));     /* the lean list, the full list behind it: one copy per round (their staging slots lie side by side) */
    RT_CHECK(e->d_anchors.reserve(3 * n_frames));       /* anchors, patches and first_of of a round travel in one copy (their three staging slots lie side by side) */
    RT_CHECK(e->d_scratch.reserve(n_frames * 2 * height));
    return SDV_OK;
}

/* The pool of reference-level sweeps (requests / outcomes), its list heads (a list per line: a lookup meets the entries of its own line only), the
 * per-level records of a chunk of sweeps and the black / white memo: sized for a tape with damage in every frame (the pool grows in the call should a
 * tape ask for more, Stc007FrameCall::settle_sweeps in stc007_frames_engine.inc).  Made when a call first sends a frame to the full kernel - a stream that plays never asks for them
 * (12 bytes per video line: about 59 MB for 10 000 NTSC frames). */
static int ensure_memo_capacity(sdv_engine *e, size_t n_frames, size_t height, bool with_snapshots = true)
{
    RT_CHECK(e->d_memo_head.reserve(n_frames * height));
    RT_CHECK(e->d_memo_count.reserve(4));
    RT_CHECK(e->d_memo.reserve(n_frames * 16 + 4096));
    RT_CHECK(e->d_sweep_levels.reserve((size_t)1024 * 256));
    RT_CHECK(e->d_bw_memo.reserve(n_frames * height));
    /* the snapshots: 16 KB per frame (two sets of 64 entries of 128 bytes) - left out for calls whose frames would need more than 4 GB of them */
    if (!with_snapshots) return SDV_OK;
    if (n_frames * 2 * sdv::TC_ENTRIES * sizeof(sdv::TcSnap) <= ((size_t)4 << 30)) {
        RT_CHECK(e->d_tc_snaps.reserve(n_frames * 2 * sdv::TC_ENTRIES));
        RT_CHECK(e->d_tc_hdr.reserve(n_frames * 2));
    }
    RT_CHECK(e->d_tc_keys.reserve(n_frames * 2 * height));
    return SDV_OK;
}

/* Settle the requests [lo, hi) of the sweep pool, a chunk at a time; sa holds the video and the settings.  The per-level records have room for the 1024
 * sweeps of a tape with a dropout now and then; a chunk that is larger gets room for a whole chunk, once. */
static int settle_sweep_chunks(sdv_engine *e, sdv::SweepArgs sa, int lo, int hi, rt::stream_t s)
{
    enum { CHUNK = 16384 };
    for (; lo < hi; lo += CHUNK) {
        const int cnt = hi - lo < CHUNK ? hi - lo : CHUNK;
        RT_CHECK(e->d_sweep_levels.reserve((size_t)cnt * 256, (size_t)CHUNK * 256));
        sa.memo = e->d_memo; sa.first = lo; sa.count = cnt; sa.levels = e->d_sweep_levels;
        /* the levels (a wave per 64 levels of a line), then chain, vote and pick (a wave per line) */
        RT_LAUNCH64(sdv_k_stc007_sweep_levels, (size_t)cnt * 4u, sa, s);
        RT_LAUNCH64(sdv_k_stc007_sweep_pick, (size_t)cnt, sa, s);
        dev_count(e, DEV_SWEEP_LEVELS, (size_t)cnt); dev_count(e, DEV_SWEEP_PICK, (size_t)cnt);
    }
    return SDV_OK;
}

/* Binarizer::processLine with an STC007Line as output, a wave per line (stc007_device.h, stc_line_body).  The reference-level sweeps the lines ask for are
 * settled between passes like the frame entry's: a pass, the round's requests through the sweep kernels, the lines that waited again - a line asks for one
 * sweep at most (its key is the levels and coordinates it was given), so the second pass is the last. */
int sdv_binarize_lines(sdv_engine *e, const uint8_t *luma, size_t row_stride, int width, size_t n_lines, const sdv_bin_state *presets,
                       uint32_t frame_number, uint16_t first_line, uint16_t line_step, unsigned flags, sdv_line_rec *out_lines, size_t lines_cap, void *stream)
{
    if (!e) return SDV_ERR_BAD_ARG;
    if (!luma) { set_error(e, "null video"); return SDV_ERR_NULL_VIDEO; }
    if (!out_lines) { set_error(e, "null output"); return SDV_ERR_NULL_PCM; }
    if (width <= 0 || width > SDV_MAX_WIDTH || row_stride < (size_t)width) { set_error(e, "bad line geometry"); return SDV_ERR_BAD_ARG; }
    if (width < sdv::BITS_IN_LINE) { set_error(e, "line shorter than the 137 bit cells of an STC-007 line"); return SDV_ERR_SHORT_LINE; }
    if (n_lines == 0) return SDV_OK;
    if (n_lines >= 0x7FFFFFFFu) { set_error(e, "too many lines in one call"); return SDV_ERR_BAD_ARG; }
    if (lines_cap < n_lines) { set_error(e, "output buffer too small: " + std::to_string(n_lines) + " line records are needed"); return SDV_ERR_BAD_ARG; }
    rt::stream_t s = (rt::stream_t)stream;
    SDV_ON_DEVICE(e);
    { const int mrc = ensure_memo_capacity(e, (n_lines + 15) / 16 + 1, 16, false); if (mrc != SDV_OK) return mrc; }       /* a list head per line, an entry per line and to spare */
    RT_CHECK(e->d_line_done.reserve(n_lines, n_lines + n_lines / 8 + 64));
    RT_CHECK(rt::dfill_bytes(e->d_line_done, 0, n_lines, s));
    RT_CHECK(rt::dfill_bytes(e->d_memo_head, 0xFF, n_lines * sizeof(int32_t), s));
    RT_CHECK(rt::dfill_bytes(e->d_memo_count, 0, 16, s));
    sdv::LineArgs7 a;
    memset(&a, 0, sizeof(a));
    a.luma = luma; a.row_stride = row_stride; a.width = width; a.n_lines = (uint32_t)n_lines; a.states = presets;
    a.frame_number = frame_number; a.first_line = first_line; a.line_step = line_step;
    a.doubled = (flags & SDV_FLAG_DOUBLED) ? 1 : 0; a.mode = (uint8_t)e->mode; a.preset = e->preset;
    a.out = out_lines; a.done = e->d_line_done;
    a.memo = e->d_memo; a.memo_head = e->d_memo_head; a.memo_count = e->d_memo_count; a.memo_cap = (int32_t)e->d_memo.cap;
    dev_reset_counts(e);
    int settled = 0;
    for (int pass = 0;; pass++) {
        if (pass > 4) { set_error(e, "the sweeps of the lines did not settle"); return SDV_ERR_HIP; }
        dev_count(e, DEV_LINES, n_lines);
        RT_LAUNCH64(sdv_k_stc007_lines, a.n_lines < rt::STC_LINES_MAX_GRID ? a.n_lines : rt::STC_LINES_MAX_GRID, a, s);     /* (a wave takes the lines a grid apart) */
        int32_t count = 0;
        RT_CHECK(rt::d2h(&count, e->d_memo_count, sizeof(count), s));
        /* (the pool holds a request per line and more: a line asks for one sweep at most - one that did not fit would leave its line waiting for good) */
        if (count > (int32_t)e->d_memo.cap) { set_error(e, "the pool of sweep requests ran over: " + std::to_string(count) + " requests, room for " + std::to_string(e->d_memo.cap)); return SDV_ERR_HIP; }
        if (count <= settled) break;
        sdv::SweepArgs sa;
        memset(&sa, 0, sizeof(sa));
        sa.luma = luma; sa.frame_stride = (size_t)sdv::LINES_PER_MEMO_FRAME * row_stride; sa.row_stride = row_stride; sa.width = width;
        sa.doubled = a.doubled; sa.mode = a.mode; sa.preset = a.preset;
        { const int src = settle_sweep_chunks(e, sa, settled, count, s); if (src != SDV_OK) return src; }
        settled = count;
    }
    /* every line's record is final: a line still waiting for a sweep holds a placeholder record, and the call says so instead of handing it out */
    {
        std::vector<uint8_t> done(n_lines);
        RT_CHECK(rt::d2h(done.data(), e->d_line_done, n_lines, s));
        size_t pending = 0;
        for (size_t i = 0; i < n_lines; i++) pending += done[i] == 0;
        if (pending) { set_error(e, std::to_string(pending) + " of " + std::to_string(n_lines) + " lines were left waiting for a reference-level sweep"); return SDV_ERR_HIP; }
    }
    return SDV_OK;
}

void sdv_default_deint_settings(sdv_deint_settings *st)   /* STC007Deinterleaver::clear, stc007deinterleaver.cpp:83-96 */
{
    memset(st, 0, sizeof(*st));
    st->res_mode = SDV_RES_MODE_14BIT_AUTO; st->ignore_crc = 0; st->force_ecc_check = 1;
    st->en_p_code = 1; st->en_q_code = 1; st->en_cwd = 0;
}

int sdv_deinterleave_blocks(sdv_engine *e, const sdv_deint_line *lines, size_t n_lines, const sdv_deint_settings *settings,
                            sdv_block_rec *out_blocks, size_t n_blocks, void *stream)
{
    if (!e || !settings) return SDV_ERR_BAD_ARG;
    if (!lines) { set_error(e, "null line buffer"); return SDV_ERR_NULL_LINES; }
    if (!out_blocks) { set_error(e, "null block buffer"); return SDV_ERR_NULL_BLOCK; }
    if (n_blocks == 0) return SDV_OK;
    /* processBlock(line_shift) needs size() > MIN_DEINT_DATA + line_shift (stc007deinterleaver.cpp:314-338) */
    if (n_lines <= (size_t)sdvd::MIN_DEINT_DATA + (n_blocks - 1)) { set_error(e, "line buffer too short for the requested blocks"); return SDV_ERR_NO_DATA; }
    sdv_deint_settings st = *settings;
    /* setter coupling of the reference (stc007deinterleaver.cpp:210-260) */
    if (st.en_q_code) st.en_p_code = 1;
    if (!st.en_p_code) { st.en_q_code = 0; st.en_cwd = 0; }
    if (st.res_mode > SDV_RES_MODE_16BIT) { set_error(e, "bad resolution mode"); return SDV_ERR_BAD_ARG; }
    SDV_ON_DEVICE(e);
    sdvd::DeintArgs a; a.lines = lines; a.n_blocks = n_blocks; a.st = st; a.out = out_blocks;
    RT_CHECK(RT_LAUNCH_ITEMS(sdv_k_stc007_deint, sdvd::deint_body, 0, a.n_blocks, 256, (rt::stream_t)stream, a));
    return SDV_OK;
}

} /* extern "C" */

#include "stc007_frames_engine.inc"  /* sdv_binarize_frames */
#include "ingest_engine.inc"         /* sdv_ingest_geometry, sdv_ingest_frames */
#include "encode_engine.inc"         /* sdv_encode_geometry, sdv_encode_frames, sdv_reset_encoder */
#include "encode_markerless_engine.inc"  /* sdv_encode_markerless_geometry, sdv_encode_markerless_frames */
#include "stage_common.inc"          /* what the sample-stream stages share: pcm_condition_engine.inc, audio_engine.inc and the stage files behind it */
#include "pcm_condition_engine.inc"  /* sdv_pcm_preemphasis, sdv_pcm_resample */
