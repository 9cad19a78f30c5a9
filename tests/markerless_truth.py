"""Ground truth for damaged PCM-1 and PCM-16x0 (SI, EI) tapes (tests/test_markerless_truth.py), the marker-less counterpart of tests/tape_truth.py: a tape is
made in numpy from PCM we choose (encode_markerless_api.tape_bits / frames_of_bits - never by the code under test), lines of it are destroyed by a damage
plan, and what a decoder makes of it is held against the PCM that went in and against what the plan alone predicts.

Nothing here looks at the decoder's code or at a recorded output.  The rules are the formats' as synth.pcm16x0_encode_fields,
encode_markerless_api.pcm1_sub_line and include/sdvpcm.h state them:

  PCM-16x0  source block b of a frame is its pairs 3 b .. 3 b + 2 and sits on three sub-lines of the frame's 1470 (a line carries the sub-lines 3 l .. 3 l + 2,
            each with a CRC of its own): u, u + 35, u + 70 with u = 105 (b // 35) + b % 35 for SI, b, b + 490, b + 980 for EI.  The middle one is P = L ^ R.
            One unread sub-line: the block comes back whole.  Two or more: it is lost, and the samples that stay invalid are the words of its unread
            audio sub-lines.
  PCM-1     no code: pair n of a field sits on sub-line pcm1_sub_line(n), a third of line sub-line // 3, and is invalid exactly if that line is unread.

and the reference's first-line rule (tape_truth.forced_bad), which profiles/markerless_truth_notes.md derives for these two formats with its source lines."""
import copy
import ctypes as C

import numpy as np

import audio_api as A
import encode_markerless_api as ml
import pcm1_api as p1
import pcm16_api as p16
import tape_truth as tt
from sdvpcmdecoder_amd.abi import PCM_PCM1, PCM_PCM16X0
from stitch_api import PAIR_DTYPE

PCM1, SI, EI = ml.PCM1, ml.SI, ml.EI
BLOCK_OK, VALID, FIXED = tt.BLOCK_OK, tt.VALID, tt.FIXED
PPF, FIELD, LINES = ml.PAIRS_PER_FRAME, ml.FIELD_PAIRS, ml.LINES
LEAD_STITCH, LEAD_AUDIO = 0, 1          # pairs between the NEW_FILE tag and source pair 0: at the stitch output, behind the audio stage (which puts a silent pair in front)
PART_COLUMNS = ((4, 240), (250, 470), (486, 716))       # columns inside the sub-lines 3 l, 3 l + 1, 3 l + 2 of a PCM-16x0 line, window 4 .. 716 (193 cells: 64, 64, the Control Bit, 64)
Q = {PCM1: 15.5, SI: 0.5, EI: 0.5}      # T5's q: rounding, and for PCM-1 the four bits pcm1_kept discards outside -8192 .. 8191 (tape_truth.SINE reaches 12000 and 9000)


# ---- tapes --------------------------------------------------------------------------------------------------------------------------------
def geometry(fmt, order=ml.TFF, flags=0, header=None, height=None, top=0):
    """the descriptor of the issue's set-up: 720 wide, levels 30 / 200, window 4 .. 716; PCM-1 with one Header line unless told; height: both fields whole"""
    header = (1 if fmt == PCM1 else 0) if header is None else header
    return ml.desc(fmt, order, 30, 200, header, flags, 720, 2 * (LINES + header) if height is None else height, 4, 716, top)


def noise(seed, n_pairs):
    """test_encode_markerless._audio: uniform int16, a third of the pairs inside the fine range of PCM-1"""
    pcm = np.random.default_rng(seed).integers(-32768, 32768, size=(n_pairs, 2), dtype=np.int16)
    pcm[::3] >>= 3
    return pcm


def make_tape(d, n_frames, audio, seed=78):
    """-> (pcm (n_frames * 1470, 2) int16, bits (fields, lines, cells), luma (n_frames, height, 720)).  Neither format has a delay: every frame carries its own pairs."""
    pcm = noise(seed, n_frames * PPF) if audio == "noise" else np.rint(tt.sine(n_frames * PPF)).astype(np.int16)
    assert audio in ("noise", "sine")
    bits = ml.tape_bits(pcm, n_frames, d.format, d.header_lines, d.ctrl_flags)
    return pcm, bits, ml.frames_of_bits(bits, d)


def apply_columns(luma, plan, d, x0, x1):
    """a copy of luma with the columns x0 .. x1 - 1 of the plan's rows at the black level"""
    out = luma.copy()
    frame, row = tt.rows_of(plan, d)
    out[frame, row, x0:x1] = d.black
    return out


# ---- the plan's predictions -----------------------------------------------------------------------------------------------------------------
class Truth:
    """What the plan alone says.  plan: bool (field in time, line of the tape's field - Header lines first); parts: the sub-lines of a destroyed PCM-16x0 line
    that are destroyed (apply_columns; default all three).  pcm: the source as the tape can carry it (PCM-1: pcm1_kept).
      dead[f, l]             the line was not read: destroyed by the plan, or forced bad (tape_truth.forced_bad: the first line left alone of a field that does
                             not open with a Header line - every PCM-16x0 field, PCM-1 with header_lines = 0)
      PCM-16x0  unread[F, b, j]   sub-line j (0: first, 1: P, 2: last) of block b of frame F;  lost[F, b]: two or more of them
      sample_unread() / sample_invalid()   (pairs, 2): the sample's own (sub-)line was not read / it cannot come back"""

    def __init__(self, pcm, plan, d, parts=(0, 1, 2)):
        self.fmt, self.d, self.plan, self.src, self.res = d.format, d, plan, pcm, None      # (res: tape_truth's STC-007 resolution; Q states the quantisation here)
        self.pcm = ml.pcm1_kept(pcm) if self.fmt == PCM1 else pcm
        self.header, self.n_frames = d.header_lines, plan.shape[0] // 2
        assert plan.shape == (2 * self.n_frames, LINES + self.header) and len(pcm) == self.n_frames * PPF
        self.forced = tt.forced_bad(plan, d, opens=self.header > 0)
        self.dead = plan | self.forced
        if self.fmt == PCM1:
            self.sub_of_pair = ml.pcm1_sub_line(np.arange(FIELD))                                   # of the field
            self._unread = np.repeat(self.dead[:, self.header + self.sub_of_pair // 3].reshape(-1)[:, None], 2, axis=1)
            self._invalid = self._unread
            return
        sub = np.zeros((2 * self.n_frames, LINES, 3), dtype=bool)
        sub[:, :, list(parts)] = plan[:, :, None]
        self.sub_destroyed = sub.reshape(self.n_frames, 2 * FIELD).copy()                           # by the plan itself: what is read there is not the source's
        sub |= self.forced[:, :, None]
        self.sub_dead = sub.reshape(self.n_frames, 2 * FIELD)                                       # by sub-line of the frame
        b = np.arange(PPF // 3)
        first, step, even = (b, 490, (b % 2) == 1) if self.fmt == EI else ((b // 35) * 105 + b % 35, 35, ((b % 35) % 2) == 1)
        self.sub_of_block = first[:, None] + step * np.arange(3)[None, :]                           # (490, 3)
        self.unread = self.sub_dead[:, self.sub_of_block]                                           # (frames, 490, 3)
        self.n_unread = self.unread.sum(axis=2)
        self.lost = self.n_unread >= 2
        # pair 3 b + k: L sits on the first sub-line where (k odd) != (b even in its interleave), else on the last; R on the other (pcm16x0_encode_fields)
        self.l_first = ((np.arange(3)[None, :] & 1) != 0) != even[:, None]                          # (490, 3)
        l_un = np.where(self.l_first[None], self.unread[:, :, 0:1], self.unread[:, :, 2:3])         # (frames, 490, 3)
        r_un = np.where(self.l_first[None], self.unread[:, :, 2:3], self.unread[:, :, 0:1])
        self._unread = np.stack([l_un, r_un], axis=3).reshape(-1, 2)
        self._invalid = self._unread & np.repeat(self.lost.reshape(-1), 3)[:, None]

    def head(self, n_frames):
        """the truth of the tape's first n_frames frames alone (the audio stage keeps the stream's last pair to itself, so T5 looks at the frames before the last)"""
        t = copy.copy(self)
        t.n_frames, t.pcm, t._unread, t._invalid = n_frames, self.pcm[:n_frames * PPF], self._unread[:n_frames * PPF], self._invalid[:n_frames * PPF]
        return t

    def sample_unread(self):
        return self._unread

    def sample_invalid(self):
        return self._invalid

    def lost_blocks(self):
        """PCM-16x0: the source blocks (three pairs each, counted through the tape) that are lost"""
        return np.flatnonzero(self.lost.reshape(-1)).tolist()

    def same(self, got):
        return got == self.pcm

    def where(self, pair, ch):
        frame, n = divmod(pair, PPF)
        if self.fmt == PCM1:
            f, n = divmod(pair, FIELD)
            u = int(self.sub_of_pair[n])
            return "pair %d %s: field %d block %d sub-line %d, line %d%s" % (pair, "LR"[ch], f, n // 92, u, self.header + u // 3, " (unread)" if self._unread[pair, ch] else "")
        b, k = divmod(n, 3)
        j = 0 if bool(self.l_first[b, k]) == (ch == 0) else 2
        u = int(self.sub_of_block[b, j])
        return "pair %d %s: frame %d block %d (source block %d, %d unread: %s) sub-line %d of the frame = field %d line %d part %d%s" % (
            pair, "LR"[ch], frame, b, pair // 3, int(self.n_unread[frame, b]), "".join("LPR"[i] if x else "-" for i, x in enumerate(self.unread[frame, b])),
            u, 2 * frame + u // FIELD, u % FIELD // 3, u % 3, " (unread)" if self._unread[pair, ch] else "")

    # ---- what the frame descriptors count (notes, "descriptors")
    def valid_lines(self):
        """PCM-1: (frames, 2) data lines read in the field that holds the picture's even rows (odd_valid_lines: the reference counts lines from 1) and in the other"""
        ok = (~self.dead[:, self.header:]).sum(axis=1).reshape(self.n_frames, 2)
        return ok[:, ::-1] if self.d.field_order == ml.BFF else ok

    def drops(self):
        """PCM-16x0, per frame: (blocks_drop, samples_drop, blocks_fix_p) - the descriptor counts sub-blocks: a lost block drops the sub-blocks that hold an invalid
        sample (all three: a sub-line carries a word of each); samples_drop: the invalid samples; a block that is not lost and whose one unread sub-line is an audio
        sub-line the plan destroyed has its three sub-blocks fixed by P.  A forced-bad line still carries the source's words, P finds nothing to repair and the
        sub-block keeps its state (notes, "descriptors") - which also takes for granted that a destroyed sub-line reads as something else than the source."""
        audio = self.unread[:, :, 0].astype(int) + self.unread[:, :, 2]
        destroyed = self.sub_destroyed[:, self.sub_of_block]
        fix = ~self.lost & (audio == 1) & (destroyed[:, :, 0] | destroyed[:, :, 2])
        return 3 * self.lost.sum(axis=1), (audio * self.lost).sum(axis=1) * 3, 3 * fix.sum(axis=1)


def pcm1_longest_run(d, row0, B, frame=1, n_frames=3):
    """the longest run of invalid samples in a channel that a burst of B lines on the rows row0 + 2 i leaves, from the interleave alone"""
    plan = tt.burst_at_row(np.zeros((2 * n_frames, LINES + d.header_lines, 1)), d, frame, row0, B)
    t = Truth(np.zeros((n_frames * PPF, 2), dtype=np.int16), plan, d)
    return max([g for ch in range(2) for _, g in tt.runs_of(t.sample_invalid()[:, ch])] or [0])


def pcm1_first_double(d, row0):
    """the shortest burst at row0 that destroys two neighbouring pairs of a channel"""
    return next(B for B in range(1, 120) if pcm1_longest_run(d, row0, B) >= 2)


# ---- decoders -----------------------------------------------------------------------------------------------------------------------------
def settings(d, **kw):
    order = 2 if d.field_order == ml.BFF else 1
    if d.format == PCM1:
        return p1.default_settings(field_order=order, **kw)
    return p16.default_settings(format=p16.FORMAT_EI if d.format == EI else p16.FORMAT_SI, field_order=order, **kw)


def oracle_decode(oracle_lib, d, luma, st=None, mask_mode=None):
    """the oracle's workers one after the other (test_encode_markerless._oracle_chain, with the stitch settings free) -> (pairs, frame descriptors, n_masked or None)"""
    import pcm1_frames_api as p1f
    import pcm16_frames_api as p16f
    from stream_scenarios import bin_to_line_recs
    st = settings(d) if st is None else st
    if d.format == PCM1:
        recs, _ = p1f.run_cpu(oracle_lib, "orc_", luma, 2, dict(new_file=True, end_file=True))
        pairs, frames = p1.run_cpu(oracle_lib, "orc_", bin_to_line_recs(recs), st)
    else:
        recs, _ = p16f.run_cpu(oracle_lib, "orc_", luma, 2, dict(new_file=True, end_file=True))
        pairs, frames = p16.run_cpu(oracle_lib, "orc_", recs, st)
    if mask_mode is None:
        return pairs, frames, None
    out, _, _, masked, hit = A.run_cpu(oracle_lib, "orc_", pairs, mask_mode, np.array([len(pairs)], dtype=np.uint64), 1)
    assert hit == 0
    return out, frames, masked


def decode(via, lib, d, luma, st=None, mask_mode=None, calls=None):
    """The tape through sdv_decode_frames on a fresh engine, the luma uploaded once into the memory of the call and every call a view of it; calls: frames per
    call (default: one call), NEW_FILE on the first and END_FILE on the last -> (pairs, frame descriptors, n_masked or None)."""
    calls = [len(luma)] if calls is None else calls
    assert sum(calls) == len(luma) and (mask_mode is None or len(calls) == 1)
    pcm_type, frasm = (PCM_PCM1, p1.FRASM1_DTYPE) if d.format == PCM1 else (PCM_PCM16X0, p16.FRASM16_DTYPE)
    st = settings(d) if st is None else st
    with_audio = mask_mode is not None
    eng = C.c_void_p(lib.sdv_engine_create(0))
    assert eng, lib.sdv_last_error(None)
    try:
        lib.sdv_set_pcm_type(eng, pcm_type, 0)
        assert (lib.sdv_set_pcm1_stitch_settings if d.format == PCM1 else lib.sdv_set_pcm16x0_stitch_settings)(eng, C.byref(st)) == 0
        if with_audio:
            assert lib.sdv_set_audio_masking(eng, mask_mode) == 0
        src = via.array(luma)
        _, h, w = luma.shape
        ps, fs, masked, done = [], [], None, 0
        for i, n in enumerate(calls):
            cap = (n + 2) * 1800 + 8192
            pairs, frames, pur = via.zeros(cap, PAIR_DTYPE), via.zeros(n + 16, frasm), via.zeros(8, A.PURGE_DTYPE)
            n_pairs, n_frames, n_pur, n_masked = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_uint64(0)
            flags = (1 if i == 0 else 0) | (4 if i + 1 == len(calls) else 0)
            rc = lib.sdv_decode_frames(eng, pcm_type, via.ptr(src, done * h * w), w, w * h, w, h, n, 1 + done, flags, via.ptr(pairs), cap, C.byref(n_pairs),
                                       via.ptr(frames), len(frames), C.byref(n_frames), None, 0, 1 if with_audio else 0, 1 if with_audio else 0,
                                       via.ptr(pur) if with_audio else None, len(pur) if with_audio else 0, C.byref(n_pur) if with_audio else None,
                                       C.byref(n_masked) if with_audio else None, via.stream())
            assert rc == 0, lib.sdv_last_error(eng)
            ps.append(via.get(pairs, n_pairs.value)); fs.append(via.get(frames, n_frames.value)); done += n
            masked = n_masked.value if with_audio else None
        assert np.array_equal(via.get(src), luma.reshape(-1))           # the frames are read only
    finally:
        lib.sdv_engine_destroy(eng)
    return np.concatenate(ps), np.concatenate(fs), masked


# ---- properties (T1: tape_truth.check_t1; T5: tape_truth.check_t5 with LEAD_AUDIO and Q) ------------------------------------------------------------
def check_t2(t, got, flags, frames, keep=None):
    """T2: every pair (of `keep`, (pairs, 2); default all) exact with SDV_SF_BLOCK_OK | SDV_SF_WORD_VALID; with nothing left out no frame drops a block."""
    k = np.ones(got.shape, dtype=bool) if keep is None else keep
    tt._first(t, (got != t.pcm) & k, "T2: not the source", got, flags)
    tt._first(t, ((flags & (BLOCK_OK | VALID)) != (BLOCK_OK | VALID)) & k, "T2: not BLOCK_OK | WORD_VALID", got, flags)
    if keep is None:
        assert (frames["blocks_drop"] == 0).all() and (frames["samples_drop"] == 0).all(), "T2: blocks_drop %s" % frames["blocks_drop"].tolist()


def check_t3(t, got, flags, frames):
    """T3: the loss is the plan's and nothing more.  The samples without SDV_SF_WORD_VALID are exactly Truth.sample_invalid(); every other sample is the source's
    and valid; SDV_SF_BLOCK_OK is missing on exactly the pairs of a block with an invalid sample (PCM-16x0: the three pairs of a lost block; PCM-1: the 92 of an
    interleave block with an unread line); the descriptors count what the plan counts (Truth.drops / Truth.valid_lines)."""
    invalid = t.sample_invalid()
    tt._first(t, ((flags & VALID) == 0) & ~invalid, "T3: invalid, and the plan says it comes back", got, flags)
    tt._first(t, ((flags & VALID) != 0) & invalid, "T3: valid, and the plan says it is lost", got, flags)
    tt._first(t, (got != t.pcm) & ~invalid, "T3: not the source", got, flags)
    full = frames[frames["service_type"] == 0]
    assert len(full) == t.n_frames
    if t.fmt == PCM1:
        per_block = np.pad(invalid.any(axis=1).reshape(-1, FIELD), ((0, 0), (0, 1))).reshape(-1, 8, 92).any(axis=2)     # 8 blocks a field, the last one pair short
        block_bad = np.repeat(per_block, 92, axis=1)[:, :FIELD].reshape(-1)
        want = np.stack([full["odd_valid_lines"], full["even_valid_lines"]], axis=1)
        assert np.array_equal(want, t.valid_lines()), "T3: odd / even valid lines %s, the plan says %s" % (want.tolist(), t.valid_lines().tolist())
    else:
        block_bad = np.repeat(t.lost.reshape(-1), 3)
        want = t.drops()
        for k, name in enumerate(("blocks_drop", "samples_drop", "blocks_fix_p")):
            assert np.array_equal(full[name], want[k]), "T3: %s %s, the plan says %s" % (name, full[name].tolist(), want[k].tolist())
    tt._first(t, ((flags & BLOCK_OK) == 0) != block_bad[:, None], "T3: BLOCK_OK is not 'no sample of the block is lost'", got, flags)


def check_t4(t, flags):
    """T4 (PCM-16x0): SDV_SF_WORD_FIXED is the reference's isWordCRCOk in a block that came out valid - the opposite of its name, as on STC-007: a sample of a valid
    block WITHOUT it was repaired by P.  Those are exactly the samples of unread audio sub-lines in blocks that are not lost; an invalid block carries none."""
    ok = (flags & BLOCK_OK) != 0
    tt._first(t, (ok & ((flags & FIXED) == 0)) != (ok & t.sample_unread() & ~t.sample_invalid()), "T4: 'valid block, no WORD_FIXED' is not 'repaired by P'", None, flags)
    tt._first(t, ~ok & ((flags & FIXED) != 0), "T4: WORD_FIXED in an invalid block", None, flags)
