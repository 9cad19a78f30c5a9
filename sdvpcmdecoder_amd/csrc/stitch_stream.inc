/*
 * stitch_stream.inc - host side of the record stream of the PCM-1 and PCM-16x0 stitch entries (device side: stitch_stream_device.h): the records
 * that wait for their END_FRAME between calls, the two-pass segment search with the host's prefix sum in between, the read-back at the end of a
 * call, and the visualiser's feeds.  pcm1_engine.inc and pcm16_engine.inc include it ahead of themselves, so the include lists of the two translation
 * units need not name it.
 */
#pragma once
template <class Rec> struct RecStream {
    rt::DevBuf<Rec> d_carry; size_t n_carry;        /* records behind the last END_FRAME of the call before */
    rt::DevBuf<Rec> d_carry_spare;
    rt::DevBuf<uint32_t> d_blk_count, d_blk_ofs;
    rt::DevBuf<uint8_t> d_svc;
    rt::DevBuf<uint32_t> d_seg_end, d_marks, d_frasm_ofs; rt::DevBuf<uint64_t> d_pair_ofs;      /* n_seg + 1 entries each */
    rt::DevBuf<uint32_t> d_stat;
    /* what sdv_k_stitch_tail brought back */
    struct Tail { uint32_t stat[4]; uint64_t pairs; uint32_t frames, last_end; };

    sdvss::RecSrc<Rec> src(const Rec *lines) const { sdvss::RecSrc<Rec> r; r.carry = d_carry; r.n_carry = (uint32_t)n_carry; r.recs = lines; return r; }

    /* the arguments of a stitch call; *total: the records of the call with the ones that waited (0: nothing to do).  noun: "line" / "sub-line" */
    int check_call(sdv_engine *e, const Rec *lines, size_t n_lines, const void *out_pairs, const void *out_frames, size_t *n_pairs, size_t *n_frames,
                   const char *noun, size_t *total) const
    {
        *total = 0;
        if (!n_pairs || !n_frames) return SDV_ERR_BAD_ARG;
        *n_pairs = 0; *n_frames = 0;
        if (n_lines > 0 && !lines) { set_error(e, "null line buffer"); return SDV_ERR_NULL_LINES; }
        if (!out_pairs || !out_frames) { set_error(e, "null output buffer"); return SDV_ERR_NULL_BLOCK; }
        if (n_carry + n_lines >= 0x3FFFFFFFu) { set_error(e, std::string("too many ") + noun + " records in one call"); return SDV_ERR_BAD_ARG; }
        *total = n_carry + n_lines;
        return SDV_OK;
    }

    /* frame segments: positions of the END_FRAME records and the file tags of every segment.  Pass 0 counts per chunk, the host sums, pass 1 writes.
     * Args: the kernel's argument type (sdvss::SegArgs<Rec> under the format's name); more: further buffers of n_seg + 1 entries to reserve with the stream's own */
    template <class Args, class Kernel, class... More>
    int segment(sdv_engine *e, Kernel kernel, size_t chunk, const Rec *lines, size_t total, rt::stream_t s, size_t *n_seg_out, More &...more)
    {
        const size_t nblk = (total + chunk - 1) / chunk;
        RT_CHECK(rt::reserve_all(nblk, nblk, d_blk_count, d_blk_ofs));
        RT_CHECK(d_stat.reserve(8));
        RT_CHECK(d_svc.reserve(total, total + total / 4 + 4096));
        Args sa; sa.src = src(lines); sa.n_recs = (uint32_t)total; sa.svc = d_svc; sa.block_count = d_blk_count; sa.block_ofs = d_blk_ofs;
        sa.seg_end = NULL; sa.n_seg = 0; sa.marks = NULL; sa.stat = d_stat; sa.write = 0;
        RT_LAUNCH64(kernel, nblk, sa, s);
        std::vector<uint32_t> blk(nblk);
        RT_CHECK(rt::d2h(blk.data(), d_blk_count, nblk * sizeof(uint32_t), s));
        size_t n_seg = 0;
        for (size_t i = 0; i < nblk; i++) { uint32_t c = blk[i]; blk[i] = (uint32_t)n_seg; n_seg += c; }
        *n_seg_out = n_seg;
        if (n_seg == 0) return SDV_OK;
        RT_CHECK(rt::reserve_all(n_seg + 1, n_seg + 1 + n_seg / 8 + 16, d_seg_end, d_marks, d_frasm_ofs, d_pair_ofs, more...));
        RT_CHECK(rt::h2d(d_blk_ofs, blk.data(), nblk * sizeof(uint32_t), s));
        const uint32_t stat0[4] = { 0, 0xFFFFFFFFu, 0, 0 };
        RT_CHECK(rt::h2d(d_stat, stat0, sizeof(stat0), s));
        RT_CHECK(rt::dfill_bytes(d_marks, 0, (n_seg + 1) * sizeof(uint32_t), s));
        sa.seg_end = d_seg_end; sa.n_seg = (uint32_t)n_seg; sa.marks = d_marks; sa.write = 1;
        RT_LAUNCH64(kernel, nblk, sa, s);
        return SDV_OK;
    }

    /* status words, totals and the last END_FRAME in one small copy (sdv_k_stitch_tail); without a segment: the stream is waited for */
    int read_tail(sdv_engine *e, size_t n_seg, rt::stream_t s, Tail *t)
    {
        memset(t, 0, sizeof(*t));
        if (n_seg == 0) { RT_CHECK(rt::ssync(s)); return SDV_OK; }
        sdv_stitch_tail_args ta; ta.stat = d_stat; ta.pair_total = d_pair_ofs + n_seg; ta.frasm_total = d_frasm_ofs + n_seg; ta.last_end = d_seg_end + (n_seg - 1);
        RT_LAUNCH64(sdv_k_stitch_tail, 1, ta, s);
        uint32_t res[8];
        RT_CHECK(rt::d2h(res, d_stat, sizeof(res), s));
        memcpy(t->stat, res, sizeof(t->stat)); t->pairs = (uint64_t)res[4] | ((uint64_t)res[5] << 32); t->frames = res[6]; t->last_end = res[7];
        return SDV_OK;
    }

    /* records after the last END_FRAME (record last_end; none when the call had no segment) wait for the next call, like lines in the reference's input queue */
    int keep_behind(sdv_engine *e, bool any_seg, uint32_t last_end, const Rec *lines, size_t n_lines, rt::stream_t s)
    {
        const size_t total = n_carry + n_lines, keep_from = any_seg ? (size_t)last_end + 1 : 0, n_keep = total - keep_from;
        if (n_keep > 0) {
            RT_CHECK(d_carry_spare.reserve(n_keep, n_keep + n_keep / 2 + 1024));
            size_t w = 0;
            if (keep_from < n_carry) { RT_CHECK(rt::d2d(d_carry_spare, d_carry + keep_from, (n_carry - keep_from) * sizeof(Rec), s)); w = n_carry - keep_from; }
            const size_t from_lines = keep_from > n_carry ? keep_from - n_carry : 0;
            if (from_lines < n_lines) RT_CHECK(rt::d2d(d_carry_spare + w, lines + from_lines, (n_lines - from_lines) * sizeof(Rec), s));
            RT_CHECK(rt::ssync(s));
            d_carry.swap(d_carry_spare);
        }
        n_carry = n_keep;
        return SDV_OK;
    }
};

/* one of the visualiser's feeds: the caller's buffer and what the last call made of it */
template <class T> struct VisFeed {
    T *p; size_t cap, n;
    void set(T *out, size_t out_cap) { p = out; cap = out ? out_cap : 0; n = 0; }
};
