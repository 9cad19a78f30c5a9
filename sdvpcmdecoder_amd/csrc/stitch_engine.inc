/*
 * stitch_engine.inc - host side of the stitch stage (sdv_stitch_frames and friends, include/sdvpcm.h).
 * Included after engine.inc by the same two translation units (product: HIP; tests: SIMT emulator).
 *
 * The reference's STC007DataStitcher::doFrameReassemble handles one frame pair per turn and every turn inherits
 * the previous one's outcome.  Here the turns of a batch run in parallel, one wave each, in rounds:
 *   round 1   every turn starts from the state of a freshly reset stitcher (turn 0: from the stream's real state);
 *   round r   every turn whose input changed is run again from what its predecessor produced in round r-1;
 * until nothing changes.  Turn 0 is exact after round 1, turn j after at most j+1 rounds, so the loop ends with every
 * turn run from exactly its predecessor's final output - the sequential result.  In practice two rounds suffice for
 * a clean tape (the paddings found from scratch equal the inherited ones) and three to four with dropouts (the CWD
 * patches of the 112-line hand-over).  The two 65-deep statistics rings (field order, resolution) are kept on the
 * host, replayed from the per-turn pushes after every round and handed to the turns as the one value they read
 * (getProbableFieldOrder / getProbableResolution, stc007datastitcher.cpp:2057-2198).
 */
#include <chrono>
#include <algorithm>
#include <cstdlib>

namespace sdvs {
/* circarray<uint8_t, 65> (circbuffer.h:30-140) */
struct Ring {
    uint8_t data[65]; size_t fill_cnt, head_i, tail_i; bool is_full;
    uint16_t count[4];          /* how many entries hold value 0..3: the majority questions are asked once per turn */
    void clear() { fill_cnt = head_i = tail_i = 0; is_full = false; count[0] = count[1] = count[2] = count[3] = 0; }
    void push(uint8_t v)
    {
        if (is_full && count[v & 3] == 65) return;      /* every entry holds v already: which of them is "replaced" makes no difference (a tape that plays) */
        if (is_full) count[data[head_i] & 3]--;         /* the slot written below holds the oldest entry */
        data[head_i] = v; count[v & 3]++;
        if (is_full) { tail_i = (tail_i + 1) % 65; head_i = tail_i; }
        else { fill_cnt++; head_i = (head_i + 1) % 65; is_full = head_i == tail_i; }
    }
    void fill(uint8_t v) { clear(); while (!is_full) push(v); }
    uint8_t probable(uint8_t a, uint8_t b, uint8_t none) const      /* getProbableFieldOrder / getProbableResolution */
    {
        const unsigned na = count[a & 3], nb = count[b & 3];
        if (na > 0 || nb > 0) return na < nb ? b : a;
        return none;
    }
};
} // namespace sdvs

struct sdv_stitcher {
    sdv_stitch_settings st;
    sdvs::Ring ring_order, ring_res;
    /* (made by new sdv_stitcher(): everything that is not a buffer starts as zero) */
    rt::DevBuf<sdv_line_rec> d_carry; size_t n_carry;
    rt::DevBuf<sdv_line_rec> d_carry_spare;     /* the next call's carry is built here, then the two swap: no allocation per call */
    rt::DevBuf<sdvs::StepChain> d_chain0;
    rt::DevBuf<sdvs::StepChain> d_chain0_spare; /* a pipelined call of known layout writes the next call's state here ahead of its read-back; swapped in when the call went as assumed */
    /* scratch, grown on demand */
    rt::DevBuf<uint32_t> d_blk_count, d_blk_ofs, d_work, d_frasm_ofs;
    size_t seg_slots;           /* segments every per-segment buffer has room for, and the layout of d_back / h_back (stitch_grow_seg; 0 while they do not agree) */
    uint32_t *d_seg_end;
    rt::DevBuf<uint8_t> d_svc;              /* service type of every record of the call (segment passes) */
    rt::DevBuf<uint64_t> d_pair_ofs;
    rt::DevBuf<sdvs::FrameLocal> d_fl; sdvs::FrameBrief *d_brief; rt::DevBuf<sdvs::StepChain> d_chain[2];
    rt::DevBuf<uint8_t> d_prob_order, d_prob_res; sdvs::StepInfo *d_info;
    rt::DevBuf<sdvs::SLine> d_ws;
    rt::DevBuf<sdvs::SLine> d_fields;
    size_t resident_waves;      /* waves of the turn kernel the device holds at once (0: not asked yet) */
    uint32_t *d_next_work;
    uint32_t guess_pairs, guess_frasm;      /* what every turn of the last call emitted, if they all emitted the same (0: unknown) */
    bool steady;                /* the stream's last turn left usable paddings and field order: later turns can be predicted from it */
    rt::DevBuf<sdv_sample_pair> d_pairs; rt::DevBuf<sdv_frame_asm> d_frasm;
    sdv_stitch_info info;
    /* sdv_set_stitch_block_output: where the data blocks go (the caller's buffer), how many the last call had */
    sdv_block_rec *block_out; size_t block_cap, n_blocks; rt::DevBuf<uint32_t> d_block_ofs;
    /* sdv_set_stitch_line_output: the assembled lines; how many every turn of the last call had (host copy) */
    sdv_asm_line_rec *line_out; size_t line_cap, n_asm_lines; rt::DevBuf<uint32_t> d_asm_cnt, d_asm_ofs; std::vector<uint32_t> *asm_per_turn;
    /* the pipelined call of a stream that plays (sdv_stitch_frames, "1p"): what the last call saw, which the next one assumes */
    /* what the host reads of a call - control words, frame briefs, turn infos, segment ends - lies in one block on the device (d_ctl, d_brief, d_info and
     * d_seg_end point into d_back) and has a page-locked mirror of the same layout: one copy brings all of it */
    rt::DevBuf<uint8_t> d_back; rt::PinBuf<uint8_t> h_back;
    int carry_frames;           /* what waits in d_carry: 0 nothing, 1 exactly one frame (its END_FRAME is the last record), -1 not known */
    uint32_t *d_ctl; double pipe_rps; uint8_t pipe_res, pipe_order; uint32_t pipe_skip, pipe_backoff;
    /* the fused entry: frames the frame kernel put into d_fields itself (stitch_prepare_direct; valid for the one stitch call behind the binarize call) */
    rt::DevBuf<sdv::DirectFrame> d_direct; bool direct_armed; uint32_t direct_ofs, direct_n;
    bool ahead_direct;          /* a call whose device work was queued ahead (STITCH_QUEUE_AHEAD): what direct_armed was then */
    bool direct_count_owed;     /* sdv_stitch_info::direct_frames of the last call is still to be counted from d_direct */
};
enum { SDV_STITCH_RETRY_WITH_RECORDS = 1000, SDV_STITCH_QUEUED_AHEAD = 1001, SDV_STITCH_NOT_QUEUED = 1002 };
/* stitch_frames_impl in two steps (the fused entry): STITCH_QUEUE_AHEAD queues the device work of the pipelined path of a known layout and returns
 * SDV_STITCH_QUEUED_AHEAD (SDV_STITCH_NOT_QUEUED, nothing done, when the call would not take that path); STITCH_TAKE_UP, same arguments, waits for it and does
 * the host's part.  In between nothing of the stream's state has moved: STITCH_WHOLE with the same arguments does the call over. */
enum { STITCH_WHOLE = 0, STITCH_QUEUE_AHEAD = 1, STITCH_TAKE_UP = 2 };      /* stitch_frames_impl: the call could not take the pipelined path its direct frames were written for */

static void stitcher_reset_host(sdv_stitcher *t)     /* STC007DataStitcher::resetState, stc007datastitcher.cpp:69-89 */
{
    t->ring_order.fill(sdvs::ORDER_UNK);
    t->ring_res.fill(sdvs::SRES_UNKNOWN);
}
static void cold_chain(sdvs::StepChain *c)
{
    memset(c, 0, sizeof(*c));
    sdvs::frasm_clear(c->f0);
    c->last_pad_counter = 0xFF; c->broken_countdown = 0; c->tail_n = 0;
}

extern "C" void sdv_default_stitch_settings(sdv_stitch_settings *st);
static sdv_stitcher *stitcher_get(sdv_engine *e)
{
    if (e->stitch) return e->stitch;
    sdv_stitcher *t = new sdv_stitcher();
    sdv_default_stitch_settings(&t->st);
    stitcher_reset_host(t);
    e->stitch = t;
    return t;
}
static void stitcher_free(sdv_engine *e)
{
    sdv_stitcher *t = e->stitch;
    if (!t) return;
    delete t->asm_per_turn;
    delete t;
    e->stitch = NULL;
}

extern "C" {

void sdv_default_stitch_settings(sdv_stitch_settings *st)      /* ctor :20-31, :7228-7236; P/Q as the application switches them on */
{
    memset(st, 0, sizeof(*st));
    st->enable_p = 1; st->enable_q = 1; st->enable_cwd = 1;
    st->max_unch_14 = 0x40; st->max_unch_16 = 0x20;
    st->use_ecc = 1; st->mask_seams = 1; st->broke_mask = 128; st->top_line_fix = 0; st->sample_rate_preset = 1;
}

int sdv_set_stitch_settings(sdv_engine *e, const sdv_stitch_settings *st)
{
    if (!e || !st) return SDV_ERR_BAD_ARG;
    stitcher_get(e)->st = *st;
    return SDV_OK;
}
int sdv_get_stitch_info(const sdv_engine *ce, sdv_stitch_info *out)
{
    if (!ce || !out || !ce->stitch) return SDV_ERR_BAD_ARG;
    sdv_engine *e = const_cast<sdv_engine *>(ce);       /* (a count that is still owed is made now: the engine's copy path, its error text) */
    sdv_stitcher *t = e->stitch;
    if (t->direct_count_owed && t->d_direct && t->direct_n > 0) {      /* (the frame kernel's summaries of the last call are still there) */
        std::vector<sdv::DirectFrame> d(t->direct_n);
        SDV_ON_DEVICE(e);
        RT_CHECK(rt::d2h(d.data(), t->d_direct, d.size() * sizeof(sdv::DirectFrame), (rt::stream_t)0));
        uint32_t c = 0;
        for (const sdv::DirectFrame &x : d) c += x.flag ? 1u : 0u;
        t->info.direct_frames = c; t->direct_count_owed = false;
    }
    *out = t->info;
    return SDV_OK;
}

/* forget the stream: a freshly constructed STC007DataStitcher */
int sdv_reset_stitcher(sdv_engine *e)
{
    if (!e) return SDV_ERR_BAD_ARG;
    SDV_ON_DEVICE(e);
    sdv_stitcher *t = stitcher_get(e);
    stitcher_reset_host(t);
    t->n_carry = 0; t->carry_frames = 0; t->steady = false; t->guess_pairs = t->guess_frasm = 0;
    if (t->d_chain0) { sdvs::StepChain c; cold_chain(&c); RT_CHECK(rt::h2d(t->d_chain0, &c, sizeof(c), (rt::stream_t)0)); RT_CHECK(rt::ssync((rt::stream_t)0)); }
    return SDV_OK;
}

/* ---- the stream's stitch state as one blob: what a process that continues the tape elsewhere (next GPU of a sharded
 * stream, a checkpoint) needs.  The statistics rings are stored oldest-first so that equal histories compare equal. */
struct sdv_stitch_state_blob {
    uint32_t magic, steady;
    uint8_t ring_order[65], ring_res[65], _pad[2];
    sdvs::StepChain chain;
};
size_t sdv_stitch_state_size(void) { return sizeof(sdv_stitch_state_blob); }

int sdv_get_stitch_state(sdv_engine *e, void *out, size_t cap)
{
    if (!e || !out || cap < sizeof(sdv_stitch_state_blob)) return SDV_ERR_BAD_ARG;
    SDV_ON_DEVICE(e);
    sdv_stitcher *t = stitcher_get(e);
    sdv_stitch_state_blob *b = (sdv_stitch_state_blob *)out;
    memset(b, 0, sizeof(*b));
    b->magic = 0x53445653u; b->steady = t->steady ? 1 : 0;
    for (int i = 0; i < 65; i++) { b->ring_order[i] = t->ring_order.data[(i + t->ring_order.tail_i) % 65]; b->ring_res[i] = t->ring_res.data[(i + t->ring_res.tail_i) % 65]; }
    if (t->d_chain0) RT_CHECK(rt::d2h(&b->chain, t->d_chain0, sizeof(sdvs::StepChain), (rt::stream_t)0));
    else cold_chain(&b->chain);
    /* the bytes between the counters and the 16-byte aligned lines (_pad and what the compiler adds behind it) are nobody's: whatever the turn that
     * wrote the chain left there must not make two equal states compare unequal - a rank of a sharded tape would decode its range again for it */
    memset((uint8_t *)&b->chain + offsetof(sdvs::StepChain, _pad), 0, offsetof(sdvs::StepChain, tail) - offsetof(sdvs::StepChain, _pad));
    /* only the lines in use are part of the state */
    for (int i = b->chain.tail_n; i < sdvs::MIN_DEINT; i++) memset(&b->chain.tail[i], 0, sizeof(sdvs::SLine));
    return SDV_OK;
}

/* Continue from a state exported by sdv_get_stitch_state; lines still waiting for their successor frame are dropped. */
int sdv_set_stitch_state(sdv_engine *e, const void *in, size_t n)
{
    if (!e || !in || n < sizeof(sdv_stitch_state_blob)) return SDV_ERR_BAD_ARG;
    const sdv_stitch_state_blob *b = (const sdv_stitch_state_blob *)in;
    if (b->magic != 0x53445653u) { set_error(e, "not a stitch state"); return SDV_ERR_BAD_ARG; }
    SDV_ON_DEVICE(e);           /* (the hand-over chain is allocated here when the stitcher is fresh: on the engine's device, not the caller's) */
    sdv_stitcher *t = stitcher_get(e);
    t->ring_order.clear(); t->ring_res.clear();
    for (int i = 0; i < 65; i++) { t->ring_order.push(b->ring_order[i]); t->ring_res.push(b->ring_res[i]); }
    t->steady = b->steady != 0; t->n_carry = 0; t->carry_frames = 0; t->guess_pairs = t->guess_frasm = 0;
    RT_CHECK(t->d_chain0.reserve(1));
    RT_CHECK(rt::h2d(t->d_chain0, &b->chain, sizeof(sdvs::StepChain), (rt::stream_t)0));
    RT_CHECK(rt::ssync((rt::stream_t)0));
    return SDV_OK;
}

/* "This tape has been playing like this for a long time": fills both statistics rings with their current majority value.
 * Used by a process that joins a stream in the middle after a short warm-up, before it compares its state with the true one. */
int sdv_saturate_stitch_stats(sdv_engine *e)
{
    if (!e) return SDV_ERR_BAD_ARG;
    sdv_stitcher *t = stitcher_get(e);
    uint8_t o = t->ring_order.probable(sdvs::ORDER_TFF, sdvs::ORDER_BFF, sdvs::ORDER_UNK);
    uint8_t r = t->ring_res.probable(sdvs::SRES_14BIT, sdvs::SRES_16BIT, sdvs::SRES_UNKNOWN);
    t->ring_order.fill(o); t->ring_res.fill(r);
    return SDV_OK;
}

int sdv_set_stitch_block_output(sdv_engine *e, sdv_block_rec *out_blocks, size_t blocks_cap)
{
    if (!e) return SDV_ERR_BAD_ARG;
    sdv_stitcher *t = stitcher_get(e);
    t->block_out = out_blocks; t->block_cap = out_blocks ? blocks_cap : 0; t->n_blocks = 0;
    return SDV_OK;
}
size_t sdv_stitch_block_count(sdv_engine *e) { return (e && e->stitch) ? e->stitch->n_blocks : 0; }
int sdv_set_stitch_line_output(sdv_engine *e, sdv_asm_line_rec *out_lines, size_t lines_cap)
{
    if (!e) return SDV_ERR_BAD_ARG;
    sdv_stitcher *t = stitcher_get(e);
    t->line_out = out_lines; t->line_cap = out_lines ? lines_cap : 0; t->n_asm_lines = 0;
    if (t->asm_per_turn) t->asm_per_turn->clear();
    return SDV_OK;
}
size_t sdv_stitch_line_count(sdv_engine *e) { return (e && e->stitch) ? e->stitch->n_asm_lines : 0; }
size_t sdv_stitch_line_counts(sdv_engine *e, uint32_t *per_turn, size_t cap)
{
    if (!e || !e->stitch || !e->stitch->asm_per_turn) return 0;
    const std::vector<uint32_t> &v = *e->stitch->asm_per_turn;
    for (size_t i = 0; i < v.size() && i < cap && per_turn; i++) per_turn[i] = v[i];
    return v.size();
}

} // extern "C"

/* room for n_seg_need frame segments in every per-segment buffer of the stitch stage */
static inline size_t stitch_back_bytes(size_t c) { return 64 + ((c * sizeof(uint32_t) + 63) & ~(size_t)63) + c * (sizeof(sdvs::FrameBrief) + sizeof(sdvs::StepInfo)); }
static int stitch_grow_seg(sdv_engine *e, sdv_stitcher *t, size_t n_seg_need)
{
    if (n_seg_need + 1 <= t->seg_slots) return SDV_OK;
    const size_t c = n_seg_need + 1 + n_seg_need / 8 + 16;         /* head room: the next call of a stream usually brings one frame more (the carried one) */
    t->seg_slots = 0;
    RT_CHECK(rt::reserve_all(c, c, t->d_work, t->d_frasm_ofs, t->d_pair_ofs, t->d_fl, t->d_chain[0], t->d_chain[1], t->d_prob_order, t->d_prob_res));
    RT_CHECK(t->d_fields.reserve(c * 2 * sdvs::FIELD_PITCH)); RT_CHECK(t->d_pairs.reserve(c * sdvs::PAIR_SLOT)); RT_CHECK(t->d_frasm.reserve(c * sdvs::FRASM_SLOT));
    RT_CHECK(t->d_back.reserve(stitch_back_bytes(c))); RT_CHECK(t->h_back.reserve(stitch_back_bytes(c)));
    t->d_ctl = (uint32_t *)t->d_back.p; t->d_next_work = t->d_ctl + sdvs::CTL_NEXT; t->d_seg_end = (uint32_t *)(t->d_back + 64);
    t->d_brief = (sdvs::FrameBrief *)(t->d_back + 64 + ((c * sizeof(uint32_t) + 63) & ~(size_t)63)); t->d_info = (sdvs::StepInfo *)(t->d_brief + c);
    t->seg_slots = c;
    return SDV_OK;
}

/* The fused entry, ahead of its binarize call: may the frame kernel put the frames it captures whole straight into the field buffers?  Yes when the stitch
 * call behind it will take the pipelined path of a stream that plays with a known layout (stitch_frames_impl, "1p": the segment ends are arithmetic, nothing
 * reads a record of those frames).  Returns the buffers for FrameArgs (fields NULL: no). */
static int stitch_prepare_direct(sdv_engine *e, size_t n_frames, size_t recs_per_frame, size_t pairs_cap, size_t frames_cap, void **fields, sdv::DirectFrame **direct, int *seg_ofs)
{
    *fields = NULL; *direct = NULL; *seg_ofs = 0;
    sdv_stitcher *t = stitcher_get(e);
    t->direct_armed = false;
    t->direct_count_owed = false;       /* (d_direct is about to be written, and perhaps regrown, for another call: a count still owed for the last one is gone) */
    if (dev_env("SDV_NO_DIRECT_FIELDS")) return SDV_OK;
    if (t->block_out || t->line_out) return SDV_OK;
    if (!(t->steady && t->pipe_rps > 0 && t->guess_pairs > 0 && t->guess_frasm > 0) || t->pipe_skip > 0 || dev_env("SDV_STITCH_TIMING") || dev_env("SDV_STITCH_NO_PIPE")) return SDV_OK;
    if (t->carry_frames < 0 || (t->carry_frames == 0) != (t->n_carry == 0) || (t->carry_frames == 1 && t->n_carry != recs_per_frame)) return SDV_OK;
    const size_t est_seg = n_frames + (size_t)t->carry_frames;
    if (est_seg < 3 || (uint64_t)(est_seg - 1) * t->guess_pairs > (uint64_t)pairs_cap || (uint64_t)(est_seg - 1) * t->guess_frasm > (uint64_t)frames_cap) return SDV_OK;
    if (recs_per_frame - 3 > 2 * (size_t)sdvs::BUF_FIELD) return SDV_OK;
    { int r = stitch_grow_seg(e, t, est_seg); if (r != SDV_OK) return r; }
    RT_CHECK(t->d_direct.reserve(n_frames, n_frames + n_frames / 8 + 16));
    t->direct_armed = true; t->direct_ofs = (uint32_t)t->carry_frames; t->direct_n = (uint32_t)n_frames;
    *fields = t->d_fields; *direct = t->d_direct; *seg_ofs = t->carry_frames;
    return SDV_OK;
}

/* What sdv_decode_frames knows of the records it hands over (they come straight from sdv_binarize_frames): `lines` holds n_frames frames of
 * recs_per_frame records each, every frame ending in its END_FRAME record, nothing else - the segment passes have nothing to find out. */
struct StitchRegular { size_t recs_per_frame, n_frames; };

static int stitch_frames_impl(sdv_engine *e, const sdv_line_rec *lines, size_t n_lines, sdv_sample_pair *out_pairs, size_t pairs_cap, size_t *n_pairs,
                              sdv_frame_asm *out_frames, size_t frames_cap, size_t *n_frames, void *stream, const StitchRegular *reg, int step = STITCH_WHOLE)
{
    if (!e || !n_pairs || !n_frames) return SDV_ERR_BAD_ARG;
    *n_pairs = 0; *n_frames = 0;
    if (n_lines > 0 && !lines) { set_error(e, "null line buffer"); return SDV_ERR_NULL_LINES; }
    if (!out_pairs || !out_frames) { set_error(e, "null output buffer"); return SDV_ERR_NULL_BLOCK; }
    rt::stream_t s = (rt::stream_t)stream;
    SDV_ON_DEVICE(e);
    sdv_stitcher *t = stitcher_get(e);
    memset(&t->info, 0, sizeof(t->info));
    t->direct_count_owed = false;       /* (owed again only by a call that ends well, below: an error return leaves nothing to count) */
    if (!t->d_chain0) {
        RT_CHECK(t->d_chain0.reserve(1));
        sdvs::StepChain c; cold_chain(&c);
        RT_CHECK(rt::h2d(t->d_chain0, &c, sizeof(c), s));
    }
    const size_t total = t->n_carry + n_lines;
    if (total == 0) return SDV_OK;
    if (total >= 0x3FFFFFFFu) { set_error(e, "too many line records in one call"); return SDV_ERR_BAD_ARG; }
    sdvs::RecSrc src; src.carry = t->d_carry; src.n_carry = (uint32_t)t->n_carry; src.recs = lines;

    const sdv_stitch_settings &st = t->st;
    sdvs::Cfg cfg; memset(&cfg, 0, sizeof(cfg));
    cfg.preset_video_mode = st.video_standard < sdvs::VID_MAX ? st.video_standard : 0;
    cfg.preset_field_order = st.field_order < sdvs::ORDER_MAX ? st.field_order : 0;
    cfg.preset_audio_res = st.resolution_preset < sdvs::SRES_MAX ? st.resolution_preset : 0;
    cfg.en_p = st.enable_p != 0; cfg.en_q = st.enable_q != 0; cfg.en_cwd = st.enable_cwd != 0; cfg.m2 = st.m2_format != 0;
    cfg.ignore_crc = st.use_ecc == 0; cfg.max_unch_14 = st.max_unch_14; cfg.max_unch_16 = st.max_unch_16;
    cfg.mask_seams = st.mask_seams != 0; cfg.broken_mask_dur = st.broke_mask; cfg.fix_cut_above = st.top_line_fix != 0;
    cfg.preset_sample_rate = st.sample_rate_preset;
    /* as many waves as are resident at once: they share the turns through a work queue */
    if (t->resident_waves == 0) t->resident_waves = rt::resident_waves(sdv_k_stitch_step, e->device);
    const size_t max_waves = t->resident_waves;
    auto grow_seg = [&](size_t n_seg_need) -> int { return stitch_grow_seg(e, t, n_seg_need); };
    auto grow_ws = [&](size_t waves) -> int {
        RT_CHECK(t->d_ws.reserve(waves * sdvs::QCAP));
        return SDV_OK;
    };

    /* 1. frame segments: positions of the END_FRAME records */
    const size_t nblk = (total + sdvs::SEG_CHUNK - 1) / sdvs::SEG_CHUNK;
    RT_CHECK(rt::reserve_all(nblk, nblk, t->d_blk_count, t->d_blk_ofs));
    RT_CHECK(t->d_svc.reserve(total, total + total / 4 + 4096));
    sdvs::SegArgs sa; sa.src = src; sa.n_recs = (uint32_t)total; sa.svc = t->d_svc; sa.block_count = t->d_blk_count; sa.block_ofs = t->d_blk_ofs; sa.seg_end = NULL; sa.write = 0; sa.seg_cap = 0;

    std::chrono::steady_clock::time_point ht[8]; for (auto &x : ht) x = std::chrono::steady_clock::now();
#define HT(i) ht[i] = std::chrono::steady_clock::now()
    HT(0);
    size_t n_seg = 0;
    /* the host's view of the read-back block (valid once grow_seg() has run for this call) */
    sdvs::FrameBrief *brief = NULL; uint32_t *seg_end = NULL, *ctl = NULL; sdvs::StepInfo *info = NULL;
    auto pin_back = [&]() {
        ctl = (uint32_t *)t->h_back.p; seg_end = (uint32_t *)(t->h_back + 64);
        brief = (sdvs::FrameBrief *)(t->h_back + 64 + ((t->seg_slots * sizeof(uint32_t) + 63) & ~(size_t)63)); info = (sdvs::StepInfo *)(brief + t->seg_slots);
    };
    sdvs::StepArgs sp; memset(&sp, 0, sizeof(sp));
    sp.cfg = cfg; sp.chain0 = t->d_chain0;
    sp.guess_pairs = t->guess_pairs; sp.guess_frasm = t->guess_frasm;
    bool try_direct = false;

    /* 1p. A stream that plays: the last call left a steady state, a constant yield per turn and the same probable field order and resolution at its
     * end.  Then this call most likely needs no answer from the host at all until its turns are through: the segments are counted on the device, the
     * analysis, the predicted hand-overs and the first round run behind each other, as wide as the last call's records per frame let expect, and the
     * host reads everything back once.  What it finds decides: all assumptions held - go on with the rounds' book-keeping as if round 1 had been run
     * the usual way; the frames are fine but an assumption was not - the rounds start over (3.); the estimate was too low - everything starts over. */
    bool piped = false, piped_round = false, tail_ahead = false;
    bool want_pipe = t->steady && t->pipe_rps > 0 && t->guess_pairs > 0 && t->guess_frasm > 0 && !dev_env("SDV_STITCH_TIMING") && !dev_env("SDV_STITCH_NO_PIPE");
    if (want_pipe && t->pipe_skip > 0) { t->pipe_skip--; want_pipe = false; }
    size_t est_seg = 0;
    /* records of known layout (sdv_decode_frames) behind a carry that is nothing or one whole frame: the segment ends are arithmetic */
    const bool regular = want_pipe && reg && reg->recs_per_frame > 0 && reg->n_frames * reg->recs_per_frame == n_lines && t->carry_frames >= 0 &&
                         (t->carry_frames == 0) == (t->n_carry == 0);
    if (want_pipe) {
        est_seg = regular ? reg->n_frames + (size_t)t->carry_frames : (size_t)((double)total / t->pipe_rps) + 2;
        if (est_seg < 3 || (uint64_t)(est_seg - 1) * t->guess_pairs > (uint64_t)pairs_cap || (uint64_t)(est_seg - 1) * t->guess_frasm > (uint64_t)frames_cap) want_pipe = false;
    }
    /* frames of this call that the frame kernel put into the field buffers itself (stitch_prepare_direct): only the pipelined path of a known layout may run */
    const bool direct_now = step == STITCH_TAKE_UP ? t->ahead_direct : t->direct_armed;
    if (step == STITCH_QUEUE_AHEAD && !(want_pipe && regular)) return SDV_STITCH_NOT_QUEUED;
    t->direct_armed = false;
    if (step == STITCH_QUEUE_AHEAD) t->ahead_direct = direct_now;
    const bool queue_now = step != STITCH_TAKE_UP;          /* (taken up: everything up to the read-back is on the stream already) */
    if (direct_now && (!(want_pipe && regular && est_seg == (size_t)t->direct_n + (size_t)t->direct_ofs) || dev_env("SDV_DIRECT_FORCE_RETRY"))) return SDV_STITCH_RETRY_WITH_RECORDS;
    bool counted = false;       /* the first segment pass has been launched */
    if (!(want_pipe && regular)) { RT_LAUNCH64(sdv_k_stitch_segments, nblk, sa, s); counted = true; }
    if (want_pipe) {
        { int r = grow_seg(est_seg); if (r != SDV_OK) return r; }
        pin_back();
        if (regular && queue_now) {
            sdvs::LayoutArgs la; la.ctl = t->d_ctl; la.seg_end = t->d_seg_end; la.n_seg = (uint32_t)est_seg; la.n_carry = (uint32_t)t->n_carry;
            la.carry_frames = (uint32_t)t->carry_frames; la.recs_per_frame = (uint32_t)reg->recs_per_frame;
            RT_LAUNCH64(sdv_k_stitch_layout, (est_seg + 63) / 64, la, s);       /* control words and segment ends */
        } else if (!regular) {
            sdvs::ScanArgs sc; sc.block_count = t->d_blk_count; sc.block_ofs = t->d_blk_ofs; sc.nblk = (uint32_t)nblk; sc.ctl = t->d_ctl; sc.next_work = t->d_next_work;
            RT_LAUNCH64(sdv_k_stitch_seg_scan, 1, sc, s);
            sa.seg_end = t->d_seg_end; sa.write = 1; sa.seg_cap = (uint32_t)est_seg;
            RT_LAUNCH64(sdv_k_stitch_segments, nblk, sa, s);
        }
        sdvs::AnalyzeArgs aa; aa.src = src; aa.seg_end = t->d_seg_end; aa.n_seg = (uint32_t)est_seg; aa.ctl = t->d_ctl; aa.cfg = cfg; aa.fl = t->d_fl; aa.brief = t->d_brief; aa.fields = t->d_fields;
        aa.timing = NULL;
        aa.direct = direct_now ? t->d_direct.p : NULL; aa.direct_ofs = t->direct_ofs; aa.direct_n = t->direct_n;
        if (e->profiling && queue_now) RT_CHECK(e->timer.start(s));
        if (queue_now) RT_LAUNCH64(sdv_k_stitch_analyze, est_seg, aa, s);
        sdvs::PredictStArgs pa; pa.fields = t->d_fields; pa.fl = t->d_fl; pa.out = t->d_chain[0]; pa.tmpl = t->d_chain0; pa.first = 0; pa.n = (uint32_t)(est_seg - 2);
        pa.ctl = t->d_ctl; pa.est_seg = (uint32_t)est_seg;
        if (queue_now) RT_LAUNCH64(sdv_k_stitch_predict, est_seg - 2, pa, s);
        const size_t waves = std::min(est_seg - 1, max_waves);
        { int r = grow_ws(waves); if (r != SDV_OK) return r; }
        sdvs::StepArgs pp = sp;
        pp.next_work = t->d_next_work;
        pp.fields = t->d_fields; pp.fl = t->d_fl; pp.work = NULL; pp.chain[0] = t->d_chain[0]; pp.chain[1] = t->d_chain[1];
        pp.prob_order = t->d_prob_order; pp.prob_res = t->d_prob_res; pp.pairs = t->d_pairs; pp.frasm = t->d_frasm; pp.info = t->d_info; pp.ws = t->d_ws;
        pp.direct_pairs = out_pairs; pp.direct_frasm = out_frames; pp.n_work = 0; pp.first_round = 0; pp.ctl = t->d_ctl; pp.est_seg = (uint32_t)est_seg; pp.timing = NULL;
        pp.pipe_order = t->pipe_order; pp.pipe_res = t->pipe_res;
        if (queue_now) RT_LAUNCH64(sdv_k_stitch_step, waves, pp, s);
        if (regular) {
            /* what the next call inherits, ahead of the read-back: with the layout known so are the last turn (est_seg - 2, handed over in the second
             * buffers after one round) and the frame that waits for its successor (the last reg->recs_per_frame records).  Both go to spare buffers
             * and are swapped in at the end if the call went as assumed - then nothing is left to do behind the read-back. */
            RT_CHECK(t->d_chain0_spare.reserve(1));
            const size_t cnt = reg->recs_per_frame;
            RT_CHECK(t->d_carry_spare.reserve(cnt, cnt + cnt / 2 + 1024));
            if (queue_now) {
                RT_CHECK(rt::d2d(t->d_chain0_spare, &t->d_chain[1][est_seg - 2], sizeof(sdvs::StepChain), s));
                RT_CHECK(rt::d2d(t->d_carry_spare, lines + (n_lines - cnt), cnt * sizeof(sdv_line_rec), s));
            }
            tail_ahead = true;
        }
        /* control words, segment ends, briefs and infos in one copy */
        if (step == STITCH_QUEUE_AHEAD) { RT_CHECK(rt::d2h_async(t->h_back, t->d_back, stitch_back_bytes(t->seg_slots), s)); return SDV_STITCH_QUEUED_AHEAD; }
        if (step == STITCH_TAKE_UP) RT_CHECK(rt::ssync(s));
        else RT_CHECK(rt::d2h_pinned(t->h_back, t->d_back, stitch_back_bytes(t->seg_slots), s));
        if (ctl[sdvs::CTL_NSEG] >= 2 && ctl[sdvs::CTL_NSEG] <= est_seg) {
            piped = true; n_seg = ctl[sdvs::CTL_NSEG];
            piped_round = ctl[sdvs::CTL_ABORT] == 0;
        }
    }
    auto keep_all = [&]() -> int {      /* nothing to do yet: the records wait for the next call, like lines in the reference's input queue */
        if (n_lines == 0) return SDV_OK;
        if (total > t->d_carry.cap) {       /* (grows with what it holds) */
            rt::DevBuf<sdv_line_rec> nc;
            RT_CHECK(nc.reserve(total + total / 2 + 1024));
            if (t->n_carry) RT_CHECK(rt::d2d(nc, t->d_carry, t->n_carry * sizeof(sdv_line_rec), s));
            RT_CHECK(rt::ssync(s));
            t->d_carry.swap(nc);
        }
        RT_CHECK(rt::d2d(t->d_carry + t->n_carry, lines, n_lines * sizeof(sdv_line_rec), s));
        RT_CHECK(rt::ssync(s));
        t->n_carry = total; t->carry_frames = -1;
        return SDV_OK;
    };
    if (!piped && direct_now) return SDV_STITCH_RETRY_WITH_RECORDS;      /* (nothing of the stream's state has been touched: the caller decodes the frames again, with records) */
    if (!piped) {
        if (!counted) { sa.seg_end = NULL; sa.write = 0; sa.seg_cap = 0; RT_LAUNCH64(sdv_k_stitch_segments, nblk, sa, s); }
        std::vector<uint32_t> blk(nblk);
        RT_CHECK(rt::d2h(blk.data(), t->d_blk_count, nblk * sizeof(uint32_t), s));
        n_seg = 0;
        for (size_t i = 0; i < nblk; i++) { uint32_t c = blk[i]; blk[i] = (uint32_t)n_seg; n_seg += c; }
        if (n_seg < 2) return keep_all();
        { int r = grow_seg(n_seg); if (r != SDV_OK) return r; }
        RT_CHECK(rt::h2d(t->d_blk_ofs, blk.data(), nblk * sizeof(uint32_t), s));
        sa.seg_end = t->d_seg_end; sa.write = 1; sa.seg_cap = 0;
        RT_LAUNCH64(sdv_k_stitch_segments, nblk, sa, s);

        /* 2. frame-local analysis */
        sdvs::AnalyzeArgs aa; aa.src = src; aa.seg_end = t->d_seg_end; aa.n_seg = (uint32_t)n_seg; aa.ctl = NULL; aa.cfg = cfg; aa.fl = t->d_fl; aa.brief = t->d_brief; aa.fields = t->d_fields;
        aa.direct = NULL; aa.direct_ofs = 0; aa.direct_n = 0;
        if (e->profiling) RT_CHECK(e->timer.start(s));
        aa.timing = NULL;
        rt::DevBuf<unsigned long long> d_atiming;
        if (dev_env("SDV_STITCH_TIMING")) { RT_CHECK(d_atiming.reserve(n_seg * 8)); RT_CHECK(rt::dfill_bytes(d_atiming, 0, n_seg * 8 * sizeof(unsigned long long), s)); aa.timing = d_atiming; }
        RT_LAUNCH64(sdv_k_stitch_analyze, n_seg, aa, s);
        if (aa.timing) {        /* developer aid: mean cycles per phase of the analysis of a frame */
            std::vector<unsigned long long> tm(n_seg * 8);
            RT_CHECK(rt::d2h(tm.data(), aa.timing, tm.size() * sizeof(unsigned long long), s));
            double ph[4] = { 0, 0, 0, 0 };
            for (size_t k = 0; k < n_seg; k++) for (int i = 0; i < 4; i++) ph[i] += (double)(tm[k * 8 + i + 1] - tm[k * 8 + i]);
            double st = 0, lp = 0, sc = 0;
            for (size_t k = 0; k < n_seg; k++) { st += (double)(tm[k * 8 + 5] - tm[k * 8 + 3]); lp += (double)(tm[k * 8 + 6] - tm[k * 8 + 5]); sc += (double)tm[k * 8 + 7]; }
            fprintf(stderr, "[analyze timing] cycles/frame: read + stage %.0f  trim %.0f  split + field buffers %.0f  resolution %.0f (first field: staging %.0f, trials %.0f, %.2f steps with a block through processBlock)\n",
                    ph[0] / n_seg, ph[1] / n_seg, ph[2] / n_seg, ph[3] / n_seg, st / n_seg, lp / n_seg, sc / n_seg);
        }
        pin_back();
        RT_CHECK(rt::d2h_async(brief, t->d_brief, n_seg * sizeof(sdvs::FrameBrief), s));
        RT_CHECK(rt::d2h_pinned(seg_end, t->d_seg_end, n_seg * sizeof(uint32_t), s));      /* synchronises both copies */
    }
    HT(1);
    for (size_t k = 0; k < n_seg; k++) {
        if (brief[k].flags & sdvs::FL_BAD_NUMBERS) { set_error(e, "a frame holds lines of another frame number (or is longer than the stitcher's trim buffer)"); return SDV_ERR_UNSUPPORTED; }
        if (k > 0 && brief[k].frame_number <= brief[k - 1].frame_number) { set_error(e, "frame numbers must increase along the stream"); return SDV_ERR_UNSUPPORTED; }
    }
    /* the turns: frame A = segment k, frame B = segment k + 1.  The turn that meets END_FILE flushes the input queue
     * (stc007datastitcher.cpp:7380-7400), so nothing behind it is stitched. */
    size_t n_steps = n_seg - 1;
    bool flushed = false;
    for (size_t k = 0; k < n_steps; k++)
        if ((brief[k].flags | brief[k + 1].flags) & sdvs::FL_END_FILE) { n_steps = k + 1; flushed = true; break; }

    HT(2);
    /* 3. rounds */
    std::vector<uint8_t> prob_order(n_steps), prob_res(n_steps), prob_prev, which(n_steps, 0), push(n_steps, 0);
    sdvs::Ring ro, rr;
    auto replay = [&]() {
        ro = t->ring_order; rr = t->ring_res;
        for (size_t k = 0; k < n_steps; k++) {
            if (brief[k].flags & sdvs::FL_NEW_FILE) { ro.fill(sdvs::ORDER_UNK); rr.fill(sdvs::SRES_UNKNOWN); }
            if (!cfg.m2) for (int p = 0; p < 2; p++) { uint8_t r = brief[k].field_res[p]; if (r == sdvs::SRES_14BIT || r == sdvs::SRES_16BIT) rr.push(r); }
            prob_res[k] = rr.probable(sdvs::SRES_14BIT, sdvs::SRES_16BIT, sdvs::SRES_UNKNOWN);
            prob_order[k] = ro.probable(sdvs::ORDER_TFF, sdvs::ORDER_BFF, sdvs::ORDER_UNK);
            if (push[k] == sdvs::ORDER_TFF || push[k] == sdvs::ORDER_BFF) ro.push(push[k]);
            if ((brief[k].flags | brief[k + 1].flags) & sdvs::FL_END_FILE) { ro.fill(sdvs::ORDER_UNK); rr.fill(sdvs::SRES_UNKNOWN); }
        }
    };
    std::vector<uint32_t> work(n_steps);
    std::vector<uint8_t> dirty(n_steps, 1);
    const size_t waves_cap = std::min(n_steps, max_waves);
    { int r = grow_ws(waves_cap); if (r != SDV_OK) return r; }
    sp.next_work = t->d_next_work;
    sp.fields = t->d_fields; sp.fl = t->d_fl; sp.work = t->d_work; sp.chain[0] = t->d_chain[0]; sp.chain[1] = t->d_chain[1];
    sp.prob_order = t->d_prob_order; sp.prob_res = t->d_prob_res; sp.pairs = t->d_pairs; sp.frasm = t->d_frasm; sp.info = t->d_info; sp.ws = t->d_ws;
    /* a stream in steady state whose last call's turns all emitted the same amount: write the outputs where they belong */
    try_direct = t->steady && t->guess_pairs > 0 && t->guess_frasm > 0 &&
                 (uint64_t)n_steps * t->guess_pairs <= (uint64_t)pairs_cap && (uint64_t)n_steps * t->guess_frasm <= (uint64_t)frames_cap;
    sp.direct_pairs = try_direct ? out_pairs : NULL; sp.direct_frasm = try_direct ? out_frames : NULL;
    rt::DevBuf<unsigned long long> d_timing;
    if (dev_env("SDV_STITCH_TIMING")) { RT_CHECK(d_timing.reserve(n_steps * 8)); RT_CHECK(rt::dfill_bytes(d_timing, 0, n_steps * 8 * sizeof(unsigned long long), s)); }
    sp.timing = d_timing;
    HT(3);
    bool plain = false;     /* every frame and every turn of the call like those of the last one: the two histories stay what they are, no replay needed */
    if (piped_round) {      /* round 1 has run (1p.): was it run on the right assumptions? */
        if (flushed) piped_round = false;       /* (a file boundary makes the kernels stand down: not reached) */
        const uint8_t po = t->pipe_order, pr = t->pipe_res;
        plain = piped_round && !cfg.m2 && (po == sdvs::ORDER_TFF || po == sdvs::ORDER_BFF) && (pr == sdvs::SRES_14BIT || pr == sdvs::SRES_16BIT) &&
                t->ring_order.is_full && t->ring_order.count[po & 3] == 65 && t->ring_res.is_full && t->ring_res.count[pr & 3] == 65;
        if (plain) {
            unsigned odd = 0;
            for (size_t k = 0; k < n_steps; k++)
                odd |= (unsigned)(brief[k].flags & sdvs::FL_NEW_FILE) | (unsigned)(brief[k].field_res[0] ^ pr) | (unsigned)(brief[k].field_res[1] ^ pr) | (unsigned)(info[k].push_order ^ po);
            plain = odd == 0;
        }
        if (piped_round && !plain) {
            for (size_t k = 0; k < n_steps; k++) push[k] = info[k].push_order;
            replay();
            for (size_t k = 0; k < n_steps && piped_round; k++) if (prob_res[k] != t->pipe_res) piped_round = false;
            if (!piped_round) std::fill(push.begin(), push.end(), 0);
        }
    }
    if (want_pipe) {
        if (piped_round) t->pipe_backoff = 0;
        else { t->pipe_backoff = t->pipe_backoff ? std::min<uint32_t>(t->pipe_backoff * 2, 64) : 1; t->pipe_skip = t->pipe_backoff; }
    }
    t->info.pipelined = piped_round ? ((plain ? 2u : 1u) | (step == STITCH_TAKE_UP ? 4u : 0u)) : 0u;
    t->info.direct_frames = 0; t->direct_count_owed = direct_now;      /* (counted when sdv_get_stitch_info asks: a counter the 10 000 analysis waves add to is 0.1 ms of atomics on one address) */
    auto after_round = [&](const std::vector<uint8_t> &ran) -> int {      /* the host's part of a round: hand-over buffers, field order history, who runs again */
        for (size_t k = 0; k < n_steps; k++) if (ran[k]) {
            which[k] ^= 1; push[k] = info[k].push_order;
            if (info[k].bits & sdvs::SI_OVERFLOW) { set_error(e, "stitch queue overflow"); return SDV_ERR_UNSUPPORTED; }
        }
        prob_prev = prob_order;
        replay();
        for (size_t k = 0; k < n_steps; k++) {
            bool d = prob_order[k] != prob_prev[k];
            if (k > 0 && ran[k - 1] && info[k - 1].changed) d = true;
            dirty[k] = d;
        }
        return 0;
    };
    bool prob_res_sent = false;         /* (a pipelined round 1 ran on two constants, not on the arrays) */
    auto run_round = [&](void) -> int {
        size_t nw = 0;
        for (size_t k = 0; k < n_steps; k++)
            if (dirty[k]) work[nw++] = (uint32_t)k | ((k > 0 ? (uint32_t)which[k - 1] : 0u) << 30) | ((uint32_t)which[k] << 31);
        if (nw == 0) return 1;
        RT_CHECK(rt::h2d(t->d_work, work.data(), nw * sizeof(uint32_t), s));
        RT_CHECK(rt::h2d(t->d_prob_order, prob_order.data(), n_steps, s));
        if (!prob_res_sent) { RT_CHECK(rt::h2d(t->d_prob_res, prob_res.data(), n_steps, s)); prob_res_sent = true; }
        sp.n_work = (uint32_t)nw; sp.first_round = 0;
        RT_CHECK(rt::dfill_bytes(t->d_next_work, 0, sizeof(uint32_t), s));
        RT_LAUNCH64(sdv_k_stitch_step, std::min(nw, waves_cap), sp, s);
        RT_CHECK(rt::d2h_pinned(info, t->d_info, n_steps * sizeof(sdvs::StepInfo), s));
        t->info.rounds++; t->info.steps_launched += (uint32_t)nw;
        std::vector<uint8_t> ran(dirty);
        return after_round(ran);
    };
    /* where the predictions come from: the stream's own state if it is steady, else the first turn is run alone */
    if (piped_round && plain) {
        std::fill(prob_order.begin(), prob_order.end(), t->pipe_order); std::fill(prob_res.begin(), prob_res.end(), t->pipe_res);
        std::fill(which.begin(), which.end(), 1); std::fill(push.begin(), push.end(), t->pipe_order);
        ro = t->ring_order; rr = t->ring_res;
        t->info.rounds = 1; t->info.steps_launched = (uint32_t)n_steps;
        unsigned bits = 0;
        for (size_t k = 0; k < n_steps; k++) { bits |= info[k].bits; dirty[k] = k > 0 && info[k - 1].changed; }
        if (bits & sdvs::SI_OVERFLOW) { set_error(e, "stitch queue overflow"); return SDV_ERR_UNSUPPORTED; }
    } else if (piped_round) {
        std::fill(prob_order.begin(), prob_order.end(), t->pipe_order);       /* what round 1 was run on; after_round() compares with the history's replay */
        t->info.rounds = 1; t->info.steps_launched = (uint32_t)n_steps;
        const std::vector<uint8_t> ran(n_steps, 1);
        int r = after_round(ran);
        if (r != 0) return r;
    } else {
        replay();
        sdvs::PredictStArgs pa; pa.fields = t->d_fields; pa.fl = t->d_fl; pa.out = t->d_chain[0]; pa.n = (uint32_t)(n_steps - 1); pa.ctl = NULL; pa.est_seg = 0;
        if (t->steady) { pa.tmpl = t->d_chain0; pa.first = 0; }
        else {
            std::fill(dirty.begin(), dirty.end(), 0); dirty[0] = 1;
            int r = run_round();
            if (r > 1 || r < 0) return r;
            pa.tmpl = &t->d_chain[which[0]][0]; pa.first = 1;
            std::fill(dirty.begin(), dirty.end(), 1); dirty[0] = 0;
        }
        if (pa.n > pa.first) RT_LAUNCH64(sdv_k_stitch_predict, pa.n - pa.first, pa, s);
    }
    for (unsigned round = 0;; round++) {
        if (round > n_steps + 2) { set_error(e, "stitch rounds did not settle"); return SDV_ERR_HIP; }
        int r = run_round();
        if (r == 1) break;
        if (r != 0) return r;
    }

    if (d_timing) {     /* developer aid: mean cycles per phase of a turn (last execution of every turn) */
        std::vector<unsigned long long> tm(n_steps * 8);
        RT_CHECK(rt::d2h(tm.data(), d_timing, tm.size() * sizeof(unsigned long long), s));
        double ph[6] = { 0, 0, 0, 0, 0, 0 };
        for (size_t k = 0; k < n_steps; k++) for (int i = 0; i < 6; i++) ph[i] += (double)(tm[k * 8 + i + 1] - tm[k * 8 + i]);
        fprintf(stderr, "[stitch timing] cycles/turn: load %.0f  stitching %.0f  fill %.0f  cwd %.0f  deinterleave %.0f  handover %.0f\n",
                ph[0] / n_steps, ph[1] / n_steps, ph[2] / n_steps, ph[3] / n_steps, ph[4] / n_steps, ph[5] / n_steps);
    }
    HT(4);
    /* 4. the outputs: already in place when the guess held for every turn, else packed from the per-turn slots */
    bool same = n_steps > 0; unsigned all_bits = 0;
    auto look_at_infos = [&]() {        /* did every turn emit the same amount? any overflow, any miss of the guess? */
        unsigned odd = 0; all_bits = 0;
        for (size_t k = 0; k < n_steps; k++) { odd |= (info[k].n_pairs ^ info[0].n_pairs) | (unsigned)(info[k].n_frasm ^ info[0].n_frasm); all_bits |= info[k].bits; }
        same = n_steps > 0 && odd == 0;
    };
    look_at_infos();
    bool direct_ok = try_direct && same && info[0].n_pairs == t->guess_pairs && info[0].n_frasm == t->guess_frasm && !(all_bits & sdvs::SI_MISS);
    if (try_direct && !direct_ok) {          /* a turn emitted something else (file tags, a change of geometry): once more, into the slots */
        sp.direct_pairs = NULL; sp.direct_frasm = NULL;
        std::fill(dirty.begin(), dirty.end(), 1);
        for (unsigned round = 0;; round++) {
            if (round > n_steps + 2) { set_error(e, "stitch rounds did not settle"); return SDV_ERR_HIP; }
            int r = run_round();
            if (r == 1) break;
            if (r != 0) return r;
        }
        look_at_infos();
    }
    uint64_t np = 0; uint32_t nf = 0;
    if (direct_ok) { np = (uint64_t)n_steps * t->guess_pairs; nf = (uint32_t)(n_steps * t->guess_frasm); }
    else {
        std::vector<uint64_t> pofs(n_steps); std::vector<uint32_t> fofs(n_steps);
        for (size_t k = 0; k < n_steps; k++) { pofs[k] = np; fofs[k] = nf; np += info[k].n_pairs; nf += info[k].n_frasm; }
        if (np > pairs_cap || nf > frames_cap) { set_error(e, "output buffers too small"); *n_pairs = (size_t)np; *n_frames = nf; return SDV_ERR_BAD_ARG; }
        RT_CHECK(rt::h2d(t->d_pair_ofs, pofs.data(), n_steps * sizeof(uint64_t), s));
        RT_CHECK(rt::h2d(t->d_frasm_ofs, fofs.data(), n_steps * sizeof(uint32_t), s));
        sdvs::CompactArgs ca; ca.pairs = t->d_pairs; ca.frasm = t->d_frasm; ca.info = t->d_info; ca.pair_ofs = t->d_pair_ofs; ca.frasm_ofs = t->d_frasm_ofs;
        ca.out_pairs = out_pairs; ca.out_frasm = out_frames; ca.n_steps = (uint32_t)n_steps;
        RT_LAUNCH64(sdv_k_stitch_compact, n_steps, ca, s);
    }
    /* 4b. the visualiser's feed: every turn once more from its final hand-over, this time leaving its data blocks where the stream of all
     * turns has them (a turn's blocks are a third of its pairs, file tags aside).  Costs one more launch of the turn kernel - when asked for. */
    if (t->block_out || t->line_out) {
        /* every turn again from its final hand-over; with the line output first a pass that only counts the lines of every turn */
        for (size_t k = 0; k < n_steps; k++) work[k] = (uint32_t)k | ((k > 0 ? (uint32_t)which[k - 1] : 0u) << 30) | ((uint32_t)which[k] << 31);
        RT_CHECK(rt::h2d(t->d_work, work.data(), n_steps * sizeof(uint32_t), s));
        if (!prob_res_sent) {           /* no round went through the host's arrays (a pipelined call whose first round settled everything) */
            RT_CHECK(rt::h2d(t->d_prob_order, prob_order.data(), n_steps, s));
            RT_CHECK(rt::h2d(t->d_prob_res, prob_res.data(), n_steps, s)); prob_res_sent = true;
        }
        sp.n_work = (uint32_t)n_steps; sp.first_round = 0; sp.timing = NULL;
        std::vector<uint32_t> aofs(n_steps), acnt(n_steps);
        if (t->line_out) {
            RT_CHECK(rt::reserve_all(n_steps, n_steps + n_steps / 4 + 16, t->d_asm_cnt, t->d_asm_ofs));
            RT_CHECK(rt::dfill_bytes(t->d_next_work, 0, sizeof(uint32_t), s));
            sp.asm_cnt = t->d_asm_cnt; sp.asm_lines = NULL; sp.asm_ofs = NULL; sp.blocks = NULL; sp.block_ofs = NULL;
            RT_LAUNCH64(sdv_k_stitch_step, std::min(n_steps, waves_cap), sp, s);
            RT_CHECK(rt::d2h(acnt.data(), t->d_asm_cnt, n_steps * sizeof(uint32_t), s));
            uint64_t na = 0;
            for (size_t k = 0; k < n_steps; k++) { aofs[k] = (uint32_t)na; na += acnt[k]; }
            t->n_asm_lines = (size_t)na;
            if (!t->asm_per_turn) t->asm_per_turn = new std::vector<uint32_t>();
            *t->asm_per_turn = acnt;
            if (na > t->line_cap) { set_error(e, "line buffer too small: " + std::to_string((unsigned long long)na) + " assembled lines are needed"); *n_pairs = (size_t)np; *n_frames = nf; return SDV_ERR_BAD_ARG; }
            RT_CHECK(rt::h2d(t->d_asm_ofs, aofs.data(), n_steps * sizeof(uint32_t), s));
            sp.asm_cnt = NULL; sp.asm_lines = t->line_out; sp.asm_ofs = t->d_asm_ofs;
        }
        std::vector<uint32_t> bofs(n_steps);
        if (t->block_out) {
            uint64_t nb = 0;
            for (size_t k = 0; k < n_steps; k++) { bofs[k] = (uint32_t)nb; nb += info[k].n_pairs / 3u; }
            t->n_blocks = (size_t)nb;
            if (nb > t->block_cap) { set_error(e, "block buffer too small: " + std::to_string((unsigned long long)nb) + " data blocks are needed"); *n_pairs = (size_t)np; *n_frames = nf; return SDV_ERR_BAD_ARG; }
            RT_CHECK(t->d_block_ofs.reserve(n_steps, n_steps + n_steps / 4 + 16));
            RT_CHECK(rt::h2d(t->d_block_ofs, bofs.data(), n_steps * sizeof(uint32_t), s));
            sp.blocks = t->block_out; sp.block_ofs = t->d_block_ofs;
        }
        RT_CHECK(rt::dfill_bytes(t->d_next_work, 0, sizeof(uint32_t), s));
        RT_LAUNCH64(sdv_k_stitch_step, std::min(n_steps, waves_cap), sp, s);
        RT_CHECK(rt::ssync(s));             /* the host vectors above go out of scope with the call */
    }
    {   /* what the next call may assume */
        t->guess_pairs = same ? info[0].n_pairs : 0; t->guess_frasm = same ? info[0].n_frasm : 0;
        if (all_bits & sdvs::SI_OVERFLOW) t->guess_pairs = t->guess_frasm = 0;
    }
    if (e->profiling) {
        RT_CHECK(e->timer.stop(s));
        RT_CHECK(e->timer.elapsed_ms(&t->info.device_ms));      /* (once per call) */
    }

    HT(5);
    /* 5. what the next call inherits */
    t->ring_order = ro; t->ring_res = rr;
    t->pipe_rps = (double)((size_t)seg_end[n_seg - 1] + 1) / (double)n_seg;
    t->pipe_res = rr.probable(sdvs::SRES_14BIT, sdvs::SRES_16BIT, sdvs::SRES_UNKNOWN); t->pipe_order = ro.probable(sdvs::ORDER_TFF, sdvs::ORDER_BFF, sdvs::ORDER_UNK);
    t->steady = !flushed && (info[n_steps - 1].bits & sdvs::SI_STEADY) != 0;
    if (tail_ahead && piped_round && !flushed && t->info.rounds == 1 && n_seg == est_seg && which[n_steps - 1] == 1 && (size_t)seg_end[n_seg - 1] + 1 == total) {
        /* the state and the waiting frame were copied ahead of the read-back (1p.): they are the right ones */
#ifdef SDV_DEV_AIDS
        {   /* (developer builds and the emulator tests check that: the copy made ahead equals the hand-over of the last turn as the rounds left it) */
            std::vector<uint8_t> ahead(sizeof(sdvs::StepChain)), now(sizeof(sdvs::StepChain));
            RT_CHECK(rt::d2h(ahead.data(), t->d_chain0_spare, ahead.size(), s));
            RT_CHECK(rt::d2h(now.data(), &t->d_chain[which[n_steps - 1]][n_steps - 1], now.size(), s));
            if (memcmp(ahead.data(), now.data(), now.size()) != 0) { set_error(e, "internal: the stitch state copied ahead of the read-back is not the last turn's"); return SDV_ERR_HIP; }
        }
#endif
        t->d_chain0.swap(t->d_chain0_spare);
        t->d_carry.swap(t->d_carry_spare);
        t->n_carry = reg->recs_per_frame; t->carry_frames = 1;
    } else {
    RT_CHECK(rt::d2d(t->d_chain0, &t->d_chain[which[n_steps - 1]][n_steps - 1], sizeof(sdvs::StepChain), s));
    if (flushed) { RT_CHECK(rt::ssync(s)); t->n_carry = 0; t->carry_frames = 0; }
    else {
        /* the last frame has no successor yet: it (and any records behind its END_FRAME) waits for the next call */
        const size_t from = (size_t)seg_end[n_seg - 2] + 1, cnt = total - from;
        RT_CHECK(t->d_carry_spare.reserve(cnt, cnt + cnt / 2 + 1024));
        sdv_line_rec *nc = t->d_carry_spare;
        size_t done = 0;
        if (from < t->n_carry) { done = t->n_carry - from; RT_CHECK(rt::d2d(nc, t->d_carry + from, done * sizeof(sdv_line_rec), s)); }
        const size_t lfrom = from + done - t->n_carry;
        RT_CHECK(rt::d2d(nc + done, lines + lfrom, (cnt - done) * sizeof(sdv_line_rec), s));
        RT_CHECK(rt::ssync(s));                       /* the caller may reuse `lines` as soon as the call returns */
        t->d_carry.swap(t->d_carry_spare);
        t->n_carry = cnt; t->carry_frames = (size_t)seg_end[n_seg - 1] + 1 == total ? 1 : -1;
    }
    }
    HT(6); if (dev_env("SDV_STITCH_HOSTTIME")) { fprintf(stderr, "[host us]"); for (int i = 1; i < 7; i++) fprintf(stderr, " %d:%.1f", i, std::chrono::duration<double, std::micro>(ht[i] - ht[i - 1]).count()); fprintf(stderr, "\n"); }
    t->info.steps = (uint32_t)n_steps;
    *n_pairs = (size_t)np; *n_frames = nf;
    return SDV_OK;
}
#undef HT

extern "C" {
int sdv_stitch_frames(sdv_engine *e, const sdv_line_rec *lines, size_t n_lines, sdv_sample_pair *out_pairs, size_t pairs_cap, size_t *n_pairs,
                      sdv_frame_asm *out_frames, size_t frames_cap, size_t *n_frames, void *stream)
{
    return stitch_frames_impl(e, lines, n_lines, out_pairs, pairs_cap, n_pairs, out_frames, frames_cap, n_frames, stream, NULL);
}

} /* extern "C" */
