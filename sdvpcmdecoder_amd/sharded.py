"""One tape decoded by several GPUs: contiguous frame ranges per rank, bit-exact with the sequential decode.

The reference decodes a tape strictly in order because both of its workers carry state from frame to frame (VideoToDigital:
binarizer tuning and coordinate histories, 120 bytes; STC007DataStitcher: previous frame's descriptor, statistics rings and the
112 assembled lines that wait in conv_queue for the next frame's blocks - the "field seam").  Sharding therefore speculates once
more, at rank granularity, with the same scheme the engine uses inside a batch:

  0. rank 0 decodes the first frames of its range and all-gathers the state it has then: the binarizer's levels are sticky
     (a line that reads from inherited levels does not measure them again), on a tape that plays they are what the tape's
     first lines measured - the one thing a warm-up further down the tape cannot find out by itself;
  1. rank r > 0 then decodes a short warm-up (the frames just before its range) from that state, discards the
     output and keeps the state it ends in - its *prediction* of the state rank r-1 will hand over;
  2. every rank decodes its own range from that state and all-gathers its final state (the only collective: 120 bytes
     per rank for the binarize stage, ~4 KB per rank - the seam lines - for the stitch stage; RCCL over xGMI on the GPU box);
  3. a rank whose prediction differs from what its predecessor really ended in decodes its range again from the true
     state; repeated until every rank started from exactly its predecessor's final state.

On a tape in steady state the prediction holds (the histories saturate within the warm-up), so step 3 does not run.
The frames a rank needs beyond its range: `warmup` frames before it and one frame after it (the successor every
stitcher turn needs); the last rank appends the end-of-file frame instead."""
from __future__ import annotations

from .abi import PCM_STC007          # sdv_set_pcm_type / sdv_decode_frames: the STC-007 chain


def shard_bounds(n_frames: int, rank: int, world: int):
    return n_frames * rank // world, n_frames * (rank + 1) // world


def check_ranges(n_frames: int, world: int):
    """Every rank needs a frame of its own.  Every rank can work out every rank's bounds, so all of them refuse together and before the
    first collective: a rank that gave up alone would leave the others waiting in the all-gather for a peer that has gone."""
    empty = [r for r in range(world) if shard_bounds(n_frames, r, world)[0] == shard_bounds(n_frames, r, world)[1]]
    if empty:
        raise ValueError(f"a tape of {n_frames} frame(s) does not shard over {world} rank(s): rank(s) {empty} would own no frame")


class ShardedDecoder:
    """`eng`: an engine with the methods of sdvpcmdecoder_amd.Engine (binarize_frames, stitch_frames, reset_stream,
    reset_stitcher, get/set_chain_state, get/set_stitch_state, saturate_stitch_stats).
    `all_gather(bytes) -> list[bytes]`: one entry per rank, in rank order (torch.distributed.all_gather of a uint8 tensor).
    `records_of(lines, a, b)`: rows a..b of a record buffer (tensor or array slicing)."""

    def __init__(self, eng, rank: int, world: int, all_gather, height: int, warmup: int = 20, stitch_warmup: int = 4):
        self.eng, self.rank, self.world, self.all_gather = eng, rank, world, all_gather
        self.height, self.warmup, self.stitch_warmup = height, warmup, stitch_warmup
        self.stats = {"binarize_redo": 0, "stitch_redo": 0, "gathers": 0}

    def frames_needed(self, n_frames: int):
        """(first, last+1) of the frames this rank has to be given: warm-up, own range, successor frame."""
        lo, hi = shard_bounds(n_frames, self.rank, self.world)
        lead = min(self.warmup, lo)
        look = 1 if hi < n_frames else 0
        return lo - lead, hi + look

    def decode(self, luma, n_frames: int, first_frame_no: int = 1):
        """luma: frames frames_needed(n_frames) of the tape (index 0 = frame frames_needed()[0]).
        Returns (pairs, frame_descriptors) of this rank's turns = frames lo..hi-1 of the tape; concatenated over the ranks
        they are the output of one engine decoding the whole tape (NEW_FILE ... END_FILE)."""
        eng, rank, world, rpf = self.eng, self.rank, self.world, self.height + 3
        lo, hi = shard_bounds(n_frames, rank, world)
        f0, f1 = self.frames_needed(n_frames)
        lead, look, n_own = lo - f0, f1 - hi, hi - lo
        last = rank == world - 1
        check_ranges(n_frames, world)
        assert luma.shape[0] == f1 - f0

        # ---- binarize stage ------------------------------------------------------------------------------------------
        eng.reset_stream()
        predicted, warm = None, None
        # The binarizer's levels are sticky: a line that reads from the levels it inherits does not measure them again, so on a tape that plays
        # they are what the first lines of the TAPE measured - nothing a warm-up at frame lo - 20 can find out.  Rank 0 therefore decodes the first
        # frames of its range first and publishes the state it has then; the other ranks start their warm-up from that state instead of from a
        # reset engine: a warm-up without a failing line keeps those levels (right on a tape that plays), one with failing lines measures its own
        # (right wherever the true chain did so at the same lines); its histories are filled by the warm-up's own frames either way.
        head = None
        if world > 1:
            early = bytes(len(eng.get_chain_state()))       # (every rank contributes a buffer of the same size)
            if rank == 0:
                k0 = min(max(self.warmup, 1), n_own)
                head, _ = eng.binarize_frames(luma[:k0], first_frame_no=first_frame_no, new_file=True, end_file=(last and k0 == n_own))
                early = eng.get_chain_state()
            early = self.all_gather(early)[0]
            self.stats["gathers"] += 1
            if rank > 0 and f0 > 0:     # (a warm-up that begins with the tape is the tape's own start: nothing to inherit)
                eng.set_chain_state(early)
        if lead:
            warm, _ = eng.binarize_frames(luma[:lead], first_frame_no=first_frame_no + f0, new_file=False)
            predicted = eng.get_chain_state()

        # ---- the range: binarizer and stitcher back to back inside the engine (sdv_decode_frames), and one all-gather for both stages ------------
        # The stitcher runs straight behind the binarizer, before anybody knows whether the range was decoded from the right state: on a tape that
        # plays it was, and then one all-gather carries what both stages assumed and what they ended with (every rank works out every rank's
        # verdict from it: no second gather to agree on going on).  A rank that assumed wrong runs its range again from the true states.
        s_lead = min(self.stitch_warmup, lead)
        fused = getattr(eng, "decode_frames", None)

        def run_range(s_from=None):
            """-> pairs, frames, final chain state, the stitcher state assumed (None: a fresh stitcher), its final state.
            s_from: the stitcher state to start from instead of the warm-up's guess (the binarizer's state is what the engine holds)."""
            out_p, out_f = [], []
            start = 0
            if s_from is not None:
                eng.set_stitch_state(s_from)
                s_pred = s_from
            else:
                eng.reset_stitcher()
                s_pred = None
                if head is not None:         # rank 0 of several: the frames it decoded first go to the stitcher as records
                    p, f = eng.stitch_frames(head)
                    out_p.append(p); out_f.append(f)
                    start = head.shape[0] // rpf
                elif s_lead:
                    # warm-up turns lo-s_lead .. lo-1 (output discarded); frame lo then waits inside the engine for its successor
                    ends_here = last and n_own == 1
                    first, _ = eng.binarize_frames(luma[lead:lead + 1], first_frame_no=first_frame_no + lo, new_file=False, end_file=ends_here)
                    eng.stitch_frames(_cat(warm[(lead - s_lead) * rpf:], first[:rpf]))
                    eng.saturate_stitch_stats()
                    s_pred = eng.get_stitch_state()     # (before END_FILE: what the predecessor has behind its successor frame, this same frame lo)
                    if ends_here:
                        # a range of the tape's last frame alone: its successor is the filler frame that closes the file, behind frame lo in
                        # `first` - that turn is all this rank puts out
                        p, f = eng.stitch_frames(first[rpf:])
                        out_p.append(p); out_f.append(f)
                    start = 1
            if start < n_own:
                kw = dict(first_frame_no=first_frame_no + lo + start, new_file=(rank == 0 and start == 0), end_file=last)
                if fused is not None:
                    p, f = fused(PCM_STC007, luma[lead + start:lead + n_own], **kw)[:2]
                else:                        # an engine object without the fused entry: the two workers one after the other
                    recs, _ = eng.binarize_frames(luma[lead + start:lead + n_own], **kw)
                    p, f = eng.stitch_frames(recs)
                out_p.append(p); out_f.append(f)
            final = eng.get_chain_state()
            if look:        # the successor frame of this range's last stitcher turn (rank r+1 decodes it again as its first frame)
                if fused is not None:
                    p, f = fused(PCM_STC007, luma[lead + n_own:], first_frame_no=first_frame_no + hi, new_file=False)[:2]
                else:
                    recs, _ = eng.binarize_frames(luma[lead + n_own:], first_frame_no=first_frame_no + hi, new_file=False)
                    p, f = eng.stitch_frames(recs)
                out_p.append(p); out_f.append(f)
            s_final = eng.get_stitch_state()
            pairs, frames = out_p[0], out_f[0]
            for p, f in zip(out_p[1:], out_f[1:]):
                pairs, frames = _cat(pairs, p), _cat(frames, f)
            return pairs, frames, final, s_pred, s_final

        pairs, frames, final, s_pred, s_final = run_range()
        while True:
            nb, ns = len(final), len(s_final)
            blobs = self.all_gather((predicted or bytes(nb)) + final + (s_pred or bytes(ns)) + s_final)
            self.stats["gathers"] += 1
            b_pred = [b[:nb] for b in blobs]; b_fin = [b[nb:2 * nb] for b in blobs]
            t_pred = [b[2 * nb:2 * nb + ns] for b in blobs]; t_fin = [b[2 * nb + ns:] for b in blobs]
            bin_ok = [r == 0 or b_pred[r] == b_fin[r - 1] for r in range(world)]
            st_ok = [r == 0 or t_pred[r] == t_fin[r - 1] for r in range(world)]
            if all(bin_ok) and all(st_ok):
                break
            if not bin_ok[rank]:
                self.stats["binarize_redo"] += 1
                predicted = b_fin[rank - 1]
                eng.set_chain_state(predicted)
                pairs, frames, final, s_pred, s_final = run_range()
            elif all(bin_ok) and not st_ok[rank]:       # (while a binarizer still decodes again, the stitcher states behind it are not final)
                self.stats["stitch_redo"] += 1
                eng.set_chain_state(predicted)                # the records stayed inside the engine: the range runs again, from both true states
                pairs, frames, final, s_pred, s_final = run_range(s_from=t_fin[rank - 1])
        return pairs, frames


class ShardedPcmDecoder:
    """The same for a PCM-1 or PCM-16x0 tape (`fmt` "pcm1" / "pcm16x0").  These formats need no successor frame (a frame is stitched
    from its own lines) and PCM-1's stitcher carries nothing from frame to frame (with automatic line offsets; manual offsets are refused), so what crosses a range boundary is the frame
    driver's chain state (120 / 192 bytes) and, for PCM-16x0, the stitcher's statistics rings (sdv_get_pcm16x0_stitch_state).
    `eng`: the methods of sdvpcmdecoder_amd.Engine for the format (pcm1_binarize_frames, pcm1_bin_to_line_recs, pcm1_stitch_frames,
    get/set_chain_state; pcm16x0_binarize_frames, pcm16x0_stitch_frames, get/set_pcm16x0_chain_state, get/set_pcm16x0_stitch_state,
    saturate_pcm16x0_stitch_stats, set_pcm16x0_stitch_settings); `stitch_settings`: the format's stitch settings (applied where the
    stitcher has to start afresh)."""

    def __init__(self, eng, rank: int, world: int, all_gather, height: int, fmt: str, stitch_settings, warmup: int = 20, stitch_warmup: int = 4):
        assert fmt in ("pcm1", "pcm16x0")
        if fmt == "pcm1" and stitch_settings is not None and not getattr(stitch_settings, "auto_offset", 1):
            # with manual line offsets PCM1DataStitcher's field buffers are stream state (what earlier frames left in them can be put out again):
            # nothing here hands them from rank to rank
            raise ValueError("ShardedPcmDecoder: a PCM-1 tape with manual line offsets does not shard (the stitcher's field buffers carry over from frame to frame)")
        self.eng, self.rank, self.world, self.all_gather, self.fmt = eng, rank, world, all_gather, fmt
        self.height, self.warmup, self.stitch_warmup, self.stitch_settings = height, warmup, stitch_warmup, stitch_settings
        self.rpf = height + 3 if fmt == "pcm1" else 3 * height + 3
        self.stats = {"binarize_redo": 0, "stitch_redo": 0, "gathers": 0}

    def frames_needed(self, n_frames: int):
        lo, hi = shard_bounds(n_frames, self.rank, self.world)
        return lo - min(self.warmup, lo), hi

    def _binarize(self, luma, **kw):
        f = self.eng.pcm1_binarize_frames if self.fmt == "pcm1" else self.eng.pcm16x0_binarize_frames
        return f(luma, **kw)[0]

    def _chain(self, state=None):
        if self.fmt == "pcm1":
            return self.eng.get_chain_state() if state is None else self.eng.set_chain_state(state)
        return self.eng.get_pcm16x0_chain_state() if state is None else self.eng.set_pcm16x0_chain_state(state)

    def _stitch(self, recs):
        if self.fmt == "pcm1":
            return self.eng.pcm1_stitch_frames(self.eng.pcm1_bin_to_line_recs(recs))
        return self.eng.pcm16x0_stitch_frames(recs)

    def decode(self, luma, n_frames: int, first_frame_no: int = 1):
        """luma: frames frames_needed(n_frames) of the tape.  Returns (pairs, frame descriptors) of frames lo..hi-1; concatenated over the
        ranks: the output of one engine decoding the whole tape (NEW_FILE ... END_FILE)."""
        eng, rank, world, rpf = self.eng, self.rank, self.world, self.rpf
        lo, hi = shard_bounds(n_frames, rank, world)
        f0, _ = self.frames_needed(n_frames)
        lead, n_own, last = lo - f0, hi - lo, rank == world - 1
        check_ranges(n_frames, world)
        assert luma.shape[0] == hi - f0
        # ---- binarize stage: as ShardedDecoder ------------------------------------------------------------------------
        eng.reset_stream()
        predicted, warm = None, None
        head = None                         # rank 0 decodes the first frames first and publishes its state: the levels are sticky (ShardedDecoder)
        if world > 1:
            early = bytes(len(self._chain()))
            if rank == 0:
                k0 = min(max(self.warmup, 1), n_own)
                head = self._binarize(luma[:k0], first_frame_no=first_frame_no, new_file=True, end_file=(last and k0 == n_own))
                early = self._chain()
            early = self.all_gather(early)[0]
            self.stats["gathers"] += 1
            if rank > 0 and f0 > 0:
                self._chain(early)
        if lead:
            warm = self._binarize(luma[:lead], first_frame_no=first_frame_no + f0, new_file=False)
            predicted = self._chain()

        def run_range():
            if head is not None:
                k0 = head.shape[0] // rpf
                own = head
                if k0 < n_own:
                    own = _cat(head, self._binarize(luma[k0:n_own], first_frame_no=first_frame_no + k0, new_file=False, end_file=last))
                return own, self._chain()
            own = self._binarize(luma[lead:lead + n_own], first_frame_no=first_frame_no + lo, new_file=(rank == 0), end_file=last)
            return own, self._chain()
        own, final = run_range()
        # ---- stitch stage, and one all-gather for both (as ShardedDecoder) ---------------------------------------------
        pcm1 = self.fmt == "pcm1"               # PCM-1: nothing is carried from frame to frame - the stitcher has no state to check
        s_lead = 0 if pcm1 else min(self.stitch_warmup, lead)
        mode, s_pred, s_final, pairs, frames = "fresh", None, b"", None, None
        while True:
            if mode == "fresh":
                if pcm1:
                    eng.set_pcm1_stitch_settings(self.stitch_settings)
                    pairs, frames = self._stitch(own)
                else:
                    eng.set_pcm16x0_stitch_settings(self.stitch_settings)          # a fresh stitcher
                    s_pred = None
                    if s_lead:
                        self._stitch(warm[(lead - s_lead) * rpf:])              # output discarded
                        eng.saturate_pcm16x0_stitch_stats()
                        s_pred = eng.get_pcm16x0_stitch_state()
                    pairs, frames = self._stitch(own)
                    s_final = eng.get_pcm16x0_stitch_state()
            elif mode == "state":
                eng.set_pcm16x0_stitch_state(s_pred)
                pairs, frames = self._stitch(own)
                s_final = eng.get_pcm16x0_stitch_state()
            mode = None
            nb, ns = len(final), len(s_final)
            blobs = self.all_gather((predicted or bytes(nb)) + final + (s_pred or bytes(ns)) + s_final)
            self.stats["gathers"] += 1
            b_pred = [b[:nb] for b in blobs]; b_fin = [b[nb:2 * nb] for b in blobs]
            t_pred = [b[2 * nb:2 * nb + ns] for b in blobs]; t_fin = [b[2 * nb + ns:] for b in blobs]
            bin_ok = [r == 0 or b_pred[r] == b_fin[r - 1] for r in range(world)]
            st_ok = [r == 0 or t_pred[r] == t_fin[r - 1] for r in range(world)]
            if all(bin_ok) and all(st_ok):
                break
            if not bin_ok[rank]:
                self.stats["binarize_redo"] += 1
                predicted = b_fin[rank - 1]
                self._chain(predicted)
                own, final = run_range()
                mode = "fresh"
            elif all(bin_ok) and not st_ok[rank]:
                self.stats["stitch_redo"] += 1
                s_pred = t_fin[rank - 1]
                mode = "state"
        return pairs, frames


class ShardedBinarizeLoop:
    """The binarize stage of a tape that keeps coming, batch after batch, each batch split over the ranks (what `bench.py --gpus N`
    times): batch s = frames [s*B, (s+1)*B) of the tape, rank r owns its r-th part.  Rank r's incoming state for batch s is rank
    r-1's final state of the same batch (rank 0: the last rank's final state of batch s-1, known exactly).  Each rank simply
    carries on from where its own engine stopped - on a tape in steady state that *is* what the predecessor hands over - then
    the 120-byte final states are all-gathered and every rank checks; a rank that guessed wrong decodes its part again from the
    true state."""

    def __init__(self, eng, rank: int, world: int, all_gather):
        self.eng, self.rank, self.world, self.all_gather = eng, rank, world, all_gather
        self.prev_last = None           # final state of the last rank in the previous batch
        self.redo = 0

    def step(self, luma, first_frame_no: int, new_file: bool = False, **kw):
        eng, rank = self.eng, self.rank
        if rank == 0 and self.prev_last is not None:
            eng.set_chain_state(self.prev_last)
        assumed = eng.get_chain_state()
        out = eng.binarize_frames(luma, first_frame_no=first_frame_no, new_file=new_file and rank == 0, **kw)
        final = eng.get_chain_state()
        while True:
            # one collective per check: every rank publishes what it started from and what it ended in (2 x 120 bytes), so that
            # all ranks see the same verdict for every rank without a second exchange
            both = self.all_gather(bytes(assumed) + bytes(final))
            k = len(both[0]) // 2
            finals = [b[k:] for b in both]
            oks = [r == 0 or both[r][:k] == finals[r - 1] for r in range(self.world)]
            if all(oks):
                break
            if not oks[rank]:
                self.redo += 1
                assumed = finals[rank - 1]
                eng.set_chain_state(assumed)
                out = eng.binarize_frames(luma, first_frame_no=first_frame_no, new_file=False, **kw)
                final = eng.get_chain_state()
        self.prev_last = finals[self.world - 1]
        return out


def torch_all_gather(device=None):
    """all_gather of equally sized byte strings over the default process group (backend nccl = RCCL on the GPU box: pass the
    rank's device; gloo on CPU: leave None)."""
    import torch
    import torch.distributed as dist

    flat_ok = [True]

    def gather(b: bytes):
        world = dist.get_world_size()
        t = torch.frombuffer(bytearray(b), dtype=torch.uint8)
        if device is not None:
            t = t.to(device)
        n = t.numel()
        if flat_ok[0]:
            try:        # one flat output tensor, one copy back to the host
                out = torch.empty(world * n, dtype=torch.uint8, device=t.device)
                dist.all_gather_into_tensor(out, t)
                host = out.cpu().numpy().tobytes()
                return [host[r * n:(r + 1) * n] for r in range(world)]
            except (RuntimeError, NotImplementedError):
                flat_ok[0] = False          # a backend without the flat form: the list form below
        outs = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(outs, t)
        return [o.cpu().numpy().tobytes() for o in outs]
    return gather


def _cat(a, b):
    try:
        import torch
        if isinstance(a, torch.Tensor):
            return torch.cat([a, b], dim=0)
    except ImportError:
        pass
    import numpy as np
    return np.concatenate([a, b])
