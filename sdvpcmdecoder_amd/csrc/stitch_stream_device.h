/*
 * stitch_stream_device.h - the record stream of the PCM-1 and PCM-16x0 stitch entries on the device (host side: stitch_stream.inc): the records
 * of a call behind the ones that waited from the call before, the search for the END_FRAME records that cut the stream into frames, the file tags
 * of every frame, and the kernel that gathers what the host reads back at the end of a call.  Written once, on the record type.
 */
#ifndef SDV_STITCH_STREAM_DEVICE_H
#define SDV_STITCH_STREAM_DEVICE_H
#include "../../include/sdvpcm.h"
#include "stc007_stitch_device.h"

namespace sdvss {
using sdvs::lanemask_lt;

/* per-frame marks: the file tags of the segment search; FF_FOREIGN is what a frame kernel adds when it meets records of another frame */
enum { FF_NEW_FILE = 1, FF_END_FILE = 2, FF_FOREIGN = 4 };

/* record i of a call: the records that waited for their END_FRAME first */
template <class Rec> struct RecSrc {
    const Rec *carry; uint32_t n_carry; const Rec *recs;
    __device__ inline const Rec &at(uint32_t i) const { return i < n_carry ? carry[i] : recs[i - n_carry]; }
};

/* ---- segments: positions of the END_FRAME records, and the file tags of every frame ------------------------------- */
/* Pass 0 counts the END_FRAMEs of every chunk of records and leaves each record's service type in a byte array (5 MB for a
 * 10 000-frame batch of PCM-1 instead of the 157 MB of records); after the host's prefix sum, pass 1 works from those bytes: it writes
 * the segment ends and tags segment k (= the number of END_FRAMEs ahead of a record) with the NEW_FILE / END_FILE records in it.
 * The frame kernels, which see the frame numbers, confirm the tags. */
template <class Rec> struct SegArgs { RecSrc<Rec> src; uint32_t n_recs; uint8_t *svc; uint32_t *block_count; const uint32_t *block_ofs; uint32_t *seg_end; uint32_t n_seg; uint32_t *marks; uint32_t *stat; int write; };
template <class Rec, int CHUNK>
__device__ inline void seg_body(const SegArgs<Rec> &a, uint32_t blk, int lane)
{
    const uint32_t lo = blk * CHUNK;
    uint32_t hi = lo + CHUNK; if (hi > a.n_recs) hi = a.n_recs;
    uint32_t cnt = 0;
    const uint32_t base = a.write ? a.block_ofs[blk] : 0u;
#pragma unroll 4
    for (uint32_t c = lo; c < hi; c += 64) {
        const uint32_t i = c + (uint32_t)lane;
        uint8_t srv = SDV_SRV_NO;
        if (i < hi) { if (a.write) srv = a.svc[i]; else { srv = a.src.at(i).service_type; a.svc[i] = srv; } }
        const uint64_t m = __ballot(srv == SDV_SRV_END_FRAME);
        if (a.write) {
            const uint32_t seg = base + cnt + (uint32_t)__popcll(m & lanemask_lt(lane));
            if (srv == SDV_SRV_END_FRAME) a.seg_end[seg] = i;
            else if ((srv == SDV_SRV_NEW_FILE || srv == SDV_SRV_END_FILE) && seg < a.n_seg) {
                atomicOr(&a.marks[seg], srv == SDV_SRV_NEW_FILE ? (uint32_t)FF_NEW_FILE : (uint32_t)FF_END_FILE);
                atomicAdd(&a.stat[2], 1u);
            }
        }
        cnt += (uint32_t)__popcll(m);
    }
    if (!a.write && lane == 0) a.block_count[blk] = cnt;
}
} // namespace sdvss

/* What the host wants to know at the end of a stitch call lies in four places; this puts it behind the four status words so that one small
 * copy brings all of it: stat[4..5] = pairs of the call, stat[6] = frame descriptors, stat[7] = index of the last END_FRAME. */
struct sdv_stitch_tail_args { uint32_t *stat; const uint64_t *pair_total; const uint32_t *frasm_total; const uint32_t *last_end; };
/* (a macro, so that the kernel keeps its place among the kernels of pcm1_stitch_device.h and the library's listing its order) */
#define SDV_STITCH_TAIL_KERNEL \
__global__ void __launch_bounds__(64) sdv_k_stitch_tail(sdv_stitch_tail_args a) \
{ \
    if (threadIdx.x != 0) return; \
    const uint64_t p = *a.pair_total; \
    a.stat[4] = (uint32_t)p; a.stat[5] = (uint32_t)(p >> 32); a.stat[6] = *a.frasm_total; a.stat[7] = *a.last_end; \
}
#endif
