"""Ground truth for damaged STC-007 / PCM-F1 tapes (tests/test_tape_truth.py): a tape is made in numpy from PCM we choose (encode_api.tape_words /
tape_frames - never by the code under test), lines of it are destroyed by a damage plan, and what a decoder makes of it is held against the PCM
that went in and against what the plan alone predicts: which words of which block sat on destroyed lines, which blocks read across a seam.

Nothing here looks at the decoder's code or at a recorded output.  The rules the predictions rest on are the format's (block s reads data lines
s + 16 k, k = 0 .. 7: L0 R0 L1 R1 L2 R2 P Q; 16 bit: P in slot 6, the S word in slot 7 of the SAME line as the word it completes) and the
reference's, which profiles/tape_truth_notes.md derives with their source lines."""
import ctypes as C

import numpy as np

import audio_api as A
import encode_api as en
import stitch_api as sa

STC007 = 2
BLOCK_OK, VALID, FIXED, MASKED = A.SF_BLOCK_OK, A.SF_WORD_VALID, A.SF_WORD_FIXED, A.SF_WORD_MASKED
LEAD_STITCH, LEAD_AUDIO = 240, 241      # pairs between the NEW_FILE tag and source pair 0: at the stitch output, behind the audio stage (which puts a silent pair in front)
SINE = ((12000.0, 997.0, 0.0), (9000.0, 440.0, 1.0))          # (amplitude, Hz, phase) of L and R at 44056 Hz
RATE = 44056.0


# ---- tapes --------------------------------------------------------------------------------------------------------------------------------
def geometry(std=en.NTSC, res=en.BIT14, ctrl=0, order=en.TFF, height=None, top=0):
    """the descriptor of the issue's set-up: 720 wide, levels 30 / 200, window 12 .. 708; height: both fields whole (490 / 588, + 2 with the control
    block) unless given"""
    height = 2 * (en.LPF[std] + ctrl) if height is None else height
    return en.desc(std, res, ctrl, 0, order, 30, 200, (0, 0, 0, 0, 0), 720, height, 12, 708, top)


def lead(d, audio_stage=False):
    """where source pair 0 comes out on the undamaged tape of geometry d: every line cut off the top of the first field takes a block off the lead-in"""
    return (LEAD_AUDIO if audio_stage else LEAD_STITCH) - 3 * d.top_line


def sine(n):
    """the real-valued signal (n, 2)"""
    t = np.arange(n, dtype=np.float64)
    return np.stack([a * np.sin(2 * np.pi * f * t / RATE + ph) for a, f, ph in SINE], axis=1)


def make_tape(std, res, n_frames, audio, seed=1, d=None):
    """-> (pcm (n, 2) int16, w9 (fields, lines, 9), luma (n_frames, height, 720)).  audio: "noise" (seeded uniform int16) or "sine"; 14 bit: the two
    low bits cleared.  The last frame carries no pairs: the interleave delay drains."""
    d = geometry(std, res) if d is None else d
    assert (d.video_standard, d.resolution) == (std, res)
    n = (n_frames - 1) * en.pairs_per_frame(std)
    if audio == "noise":
        pcm = np.random.default_rng(seed).integers(-32768, 32768, size=(n, 2), dtype=np.int16)
    else:
        assert audio == "sine"
        pcm = np.rint(sine(n)).astype(np.int16)
    if res == en.BIT14:
        pcm = pcm & ~3
    w9 = en.tape_words(pcm, n_frames, std, res, d.ctrl_block)
    return pcm, w9, en.tape_frames(w9, d)


# ---- damage plans: bool (field, line of the tape's field - the control line, if any, is line 0) ----------------------------------------------
def no_damage(w9):
    return np.zeros(w9.shape[:2], dtype=bool)


def burst(w9, frame, field, first_line, B):
    """B consecutive lines of one field (0: the first in time) of one frame"""
    plan = no_damage(w9)
    assert first_line + B <= plan.shape[1]
    plan[2 * frame + field, first_line:first_line + B] = True
    return plan


def burst_at_row(w9, d, frame, row0, B):
    """... given as the picture rows row0 + 2 i"""
    return burst(w9, frame, (row0 & 1) ^ (1 if d.field_order == en.BFF else 0), d.top_line + row0 // 2, B)


def scattered(w9, p, seed):
    return np.random.default_rng(seed).random(w9.shape[:2]) < p


def window(w9, d):
    """the lines a capture of d.height rows from d.top_line on does not hold"""
    plan = no_damage(w9)
    line = np.arange(plan.shape[1])
    plan[:, (line < d.top_line) | (line >= d.top_line + d.height // 2)] = True
    return plan


def rows_of(plan, d):
    """(frame, row) of the destroyed lines that the picture shows"""
    field, line = np.nonzero(plan)
    row = 2 * (line - d.top_line) + ((field & 1) ^ (1 if d.field_order == en.BFF else 0))
    keep = (row >= 0) & (row < (d.height & ~1))
    return field[keep] // 2, row[keep]


def apply(luma, plan, d, how="black", seed=0):
    """a copy of luma with the plan's rows at the black level, or with their data window filled with seeded random bytes"""
    out = luma.copy()
    frame, row = rows_of(plan, d)
    if how == "black":
        out[frame, row] = d.black
    else:
        assert how == "random"
        out[frame, row, d.data_start:d.data_stop] = np.random.default_rng(seed).integers(0, 256, size=(len(row), d.data_stop - d.data_start), dtype=np.uint8)
    return out


def forced_bad(plan, d, opens=None):
    """The lines the reference's VideoToDigital hands on as bad although they read well.  A field that does not open with its control block (or header)
    is "unsafe" from its first line with PCM on: the dropout compensator of the player may have copied that line from above the picture.  The first line
    of such a field whose CRC is good is forced bad, and only a good CRC ends the state (videotodigital.cpp:1156-1166, :1193-1203 with en_first_line_dup,
    :1391-1395).  So: per field, the first captured line the plan leaves alone - unless that line is the control line.  Its words still reach the blocks,
    but with the line-CRC state 'bad': to every block it is one more unread word.  opens: the fields open with such a line (default: the STC-007 descriptor's
    ctrl_block; tests/markerless_truth.py hands in PCM-1's header_lines - the rule is the same in all three branches of VideoToDigital)."""
    opens = d.ctrl_block if opens is None else opens
    out = np.zeros_like(plan)
    last = min(plan.shape[1], d.top_line + d.height // 2)
    for f in range(plan.shape[0]):
        alive = np.flatnonzero(~plan[f, d.top_line:last])
        if len(alive) and not (opens and d.top_line + alive[0] == 0):
            out[f, d.top_line + alive[0]] = True
    return out


class Truth:
    """What the plan alone says about every source block s (three pairs: pcm[3 s : 3 s + 3]):
      unread[s, k]      word k of block s sat on a line the decoder cannot have read: destroyed by the plan, or forced bad (forced_bad above)
                        (14 bit: k = 0 .. 7; 16 bit: k = 0 .. 6, the S bits ride on the same line as the word they complete)
      field_seam[s]     its first and its last line lie in different fields;  frame_seam[s]: ... in different frames
      lost[s]           more unread words than the code repairs: three of eight at 14 bit (P and Q locate nothing, they repair two known positions,
                        stc007deinterleaver.cpp:479-620), two of seven at 16 bit (P alone).  Which words stay invalid: the unread audio words."""

    def __init__(self, pcm, plan, d):
        self.pcm, self.plan, self.d = pcm, plan, d
        self.res, self.ctrl, self.lpf = d.resolution, d.ctrl_block, en.LPF[d.video_standard]
        self.n_words = 7 if self.res == en.BIT16 else 8
        self.n_blocks = (len(pcm) + 2) // 3
        dead = (plan | forced_bad(plan, d))[:, self.ctrl:].reshape(-1)            # by data line of the tape
        m = np.arange(self.n_blocks)[:, None] + 16 * np.arange(8)[None, :]
        assert m.max() < len(dead), "the tape's last frame has to drain the delay"
        self.data_line = m
        self.unread = dead[m]
        self.unread[:, self.n_words:] = False
        field = m // self.lpf
        self.field_seam = field[:, 0] != field[:, self.n_words - 1]
        self.frame_seam = field[:, 0] // 2 != field[:, self.n_words - 1] // 2
        self.n_unread = self.unread.sum(axis=1)
        self.n_unread_audio = self.unread[:, :6].sum(axis=1)
        self.lost = self.n_unread >= (2 if self.res == en.BIT16 else 3)

    def line_of(self, s, k):
        m = int(self.data_line[s, k])
        return m // self.lpf, m % self.lpf + self.ctrl

    def where(self, pair, ch):
        s, k = pair // 3, 2 * (pair % 3) + ch
        return "pair %d %s: block %d word %d, field %d line %d%s" % ((pair, "LR"[ch], s, k) + self.line_of(s, k) + (" (unread)" if self.unread[s, k] else "",))

    def sample_unread(self):
        """(pairs, 2): the sample's own line was not read"""
        return self.unread[:, :6].reshape(-1, 2)[:len(self.pcm)]

    def sample_invalid(self):
        """(pairs, 2): the samples that cannot come back: the unread audio words of the lost blocks"""
        return (self.unread[:, :6] & self.lost[:, None]).reshape(-1, 2)[:len(self.pcm)]

    def lost_blocks(self):
        return np.flatnonzero(self.lost).tolist()

    def same(self, got):
        """T1's rule of equality, (pairs, 2): 14 bit exact, 16 bit in the upper 14 bits"""
        return (got >> 2) == (self.pcm >> 2) if self.res == en.BIT16 else got == self.pcm

    def fixes(self):
        """(blocks repaired by P, by Q) as the deinterleaver's task selection counts them (stc007deinterleaver.cpp:479-620, :718, :921, STC007DataBlock::AUD_FIX_P /
        AUD_FIX_Q): a block that is not lost and has n unread audio words is repaired by P if n == 1 and P itself was read, by Q if n == 2, or if
        n == 1 and P was not read (14 bit only; at 16 bit those are lost).  A block that lost only P and / or Q has them recomputed and counts as neither.
        The forced-bad first lines are in: the undamaged tape has its fixes too, and the caller subtracts them."""
        p_gone = self.unread[:, 6]
        fix_p = ~self.lost & (self.n_unread_audio == 1) & ~p_gone
        fix_q = ~self.lost & ((self.n_unread_audio == 2) | ((self.n_unread_audio == 1) & p_gone))
        return int(fix_p.sum()), int(fix_q.sum())


# ---- decoders -----------------------------------------------------------------------------------------------------------------------------
def oracle_decode(oracle_lib, luma, mask_mode=None):
    """the oracle's workers one after the other -> (pairs, frame descriptors, n_masked or None)"""
    from oracle_run import oracle_binarize
    recs, _ = oracle_binarize(luma, mode=2, first_frame_no=1, new_file=True, end_file=True)
    pairs, frames = sa.run_cpu(oracle_lib, "orc_", recs, sa.default_settings())
    if mask_mode is None:
        return pairs, frames, None
    out, _, _, masked, hit = A.run_cpu(oracle_lib, "orc_", pairs, mask_mode, np.array([len(pairs)], dtype=np.uint64), 1)
    assert hit == 0
    return out, frames, masked


def new_engine(lib, mask_mode=None):
    eng = C.c_void_p(lib.sdv_engine_create(0))
    assert eng, lib.sdv_last_error(None)
    lib.sdv_set_pcm_type(eng, STC007, 0)
    if mask_mode is not None:
        assert lib.sdv_set_audio_masking(eng, mask_mode) == 0
    return eng


def decode_call(via, lib, eng, src, at, shape, first_frame_no, flags, with_audio=False):
    """one sdv_decode_frames call over the frames that start `at` bytes into the buffer `src` of the call's own memory -> (pairs, descriptors, n_masked)"""
    n, h, w = shape
    cap = (n + 2) * 2100 + 8192
    pairs, frames, pur = via.zeros(cap, sa.PAIR_DTYPE), via.zeros(n + 16, sa.FRASM_DTYPE), via.zeros(8, A.PURGE_DTYPE)
    n_pairs, n_frames, n_pur, n_masked = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_uint64(0)
    rc = lib.sdv_decode_frames(eng, STC007, via.ptr(src, at), w, w * h, w, h, n, first_frame_no, flags, via.ptr(pairs), cap, C.byref(n_pairs),
                               via.ptr(frames), len(frames), C.byref(n_frames), None, 0, 1 if with_audio else 0, 1 if with_audio else 0,
                               via.ptr(pur) if with_audio else None, len(pur) if with_audio else 0, C.byref(n_pur) if with_audio else None,
                               C.byref(n_masked) if with_audio else None, via.stream())
    assert rc == 0, lib.sdv_last_error(eng)
    return via.get(pairs, n_pairs.value), via.get(frames, n_frames.value), n_masked.value if with_audio else None


def decode(via, lib, luma, mask_mode=None, calls=None):
    """The tape through sdv_decode_frames on a fresh engine, the luma uploaded once into the memory of the call and every call a view of it; calls: frames
    per call (default: one call), NEW_FILE on the first and END_FILE on the last."""
    calls = [len(luma)] if calls is None else calls
    assert sum(calls) == len(luma) and (mask_mode is None or len(calls) == 1)
    eng = new_engine(lib, mask_mode)
    try:
        src = via.array(luma)
        ps, fs, masked, done = [], [], None, 0
        for i, n in enumerate(calls):
            p, f, masked = decode_call(via, lib, eng, src, done * luma.shape[1] * luma.shape[2], (n,) + luma.shape[1:], 1 + done,
                                       (1 if i == 0 else 0) | (4 if i + 1 == len(calls) else 0), mask_mode is not None)
            ps.append(p); fs.append(f); done += n
        assert np.array_equal(via.get(src), luma.reshape(-1))           # the frames are read only
    finally:
        lib.sdv_engine_destroy(eng)
    return np.concatenate(ps), np.concatenate(fs), masked


# ---- alignment ----------------------------------------------------------------------------------------------------------------------------
def align(decoded, pcm, search=1024):
    """(offset of source pair 0 among the audio pairs of the stream - the stream of one file, NEW_FILE tag first, if it still has its tags -, audio words (n, 2), sample flags (n, 2)) of the source's span.
    The offset is the one at which the most samples agree - matching the first pairs fails once those are damaged - and it has to be the only one."""
    audio = decoded[decoded["service_type"] == 0]
    n = len(pcm)
    assert len(audio) >= n, "%d audio pairs decoded, %d encoded" % (len(audio), n)
    words = audio["audio_word"]
    hits = np.array([int((words[o:o + n] == pcm).sum()) for o in range(min(search, len(audio) - n) + 1)])
    best = int(hits.argmax())
    assert hits[best] > n // 2 and (np.delete(hits, best) < hits[best] // 2).all(), "no single offset: the best agree in %s samples" % np.sort(hits)[-3:]
    return best, words[best:best + n].copy(), audio["sample_flags"][best:best + n].copy()


# ---- properties ---------------------------------------------------------------------------------------------------------------------------
def _first(t, bad, what, got=None, flags=None):
    """raises on the first offending sample of the (pairs, 2) mask `bad`"""
    if bad.any():
        pair, ch = (int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: %d samples, the first %s; source %d%s%s" % (
            what, int(bad.sum()), t.where(pair, ch), t.pcm[pair, ch], "" if got is None else ", decoded %d" % got[pair, ch],
            "" if flags is None else ", flags 0x%X" % flags[pair, ch]))


def check_t1(t, got, flags):
    """T1: nothing wrong is called valid.  Every sample with SDV_SF_WORD_VALID is the source's: exactly at 14 bit, in its upper 14 bits at 16 bit (the two
    low bits travel in the S word and are not covered by P)."""
    _first(t, ((flags & VALID) != 0) & ~t.same(got), "T1: valid and not the source", got, flags)


def check_t2(t, got, flags, frames, but=()):
    """T2: inside the code's reach everything comes back: every pair exact with SDV_SF_BLOCK_OK | SDV_SF_WORD_VALID, no frame drops a block.  `but`: source
    blocks left out (T3's predicted losses)."""
    keep = np.ones(len(t.pcm), dtype=bool)
    for s in but:
        keep[3 * s:3 * s + 3] = False
    _first(t, (got != t.pcm) & keep[:, None], "T2: not the source", got, flags)
    _first(t, ((flags & (BLOCK_OK | VALID)) != (BLOCK_OK | VALID)) & keep[:, None], "T2: not BLOCK_OK | WORD_VALID", got, flags)
    if not but:
        assert (frames["blocks_drop"] == 0).all(), "T2: blocks_drop %s" % frames["blocks_drop"].tolist()


def lost_blocks(flags):
    """source blocks with a sample that is not VALID"""
    bad = ((flags & VALID) == 0).any(axis=1)
    return sorted(set((np.flatnonzero(bad) // 3).tolist()))


def check_t3(t, got, flags, frames, predicted):
    """T3: just outside the reach the loss is the predicted one: the blocks with a sample that is not VALID are `predicted` (from the plan), every other pair
    obeys T2, and the descriptors count as many dropped blocks."""
    assert lost_blocks(flags) == sorted(predicted), "T3: lost %s, the plan says %s" % (lost_blocks(flags), sorted(predicted))
    check_t2(t, got, flags, frames, but=predicted)
    assert int(frames["blocks_drop"].sum()) == len(predicted), "T3: blocks_drop %s" % frames["blocks_drop"].tolist()


def check_t4(t, flags, seams_may_be_unsafe=False):
    """T4: the flags say where the damage was.  SDV_SF_WORD_FIXED is the reference's isWordLineCRCOk (STC007DataStitcher::outputSamplePair fills word_fixed
    from it, stc007datastitcher.cpp:6545-6546) - the OPPOSITE of its name: in a block that came out valid it is set exactly on the samples whose own tape line
    was read; the samples of an invalid block carry none.  seams_may_be_unsafe: a block that reads across a field seam may instead carry none at all - where
    the stitcher could not prove the padding of a seam it marks every block across it unsafe (performDeinterleave, stc007datastitcher.cpp:6734-6766), and
    markAsUnsafe clears every line-CRC state (stc007datablock.cpp:168-201).  Which seams: that is the padding search's business, not the plan's."""
    ok = ((flags & BLOCK_OK) != 0)
    block_ok = ok.reshape(-1)[:len(ok) // 3 * 6].reshape(-1, 6)
    assert (block_ok.all(axis=1) | ~block_ok.any(axis=1)).all(), "T4: BLOCK_OK differs inside a block"
    bad = ((flags & FIXED) != 0) != (ok & ~t.sample_unread())
    if seams_may_be_unsafe:
        n = len(flags) // 3
        none = ((flags[:3 * n] & FIXED) == 0).reshape(n, 6).all(axis=1) & t.field_seam[:n]
        bad[:3 * n] &= ~np.repeat(none, 3)[:, None]
    _first(t, bad, "T4: WORD_FIXED is not 'the line was read'", None, flags)


# ---- the audio stage against the signal -----------------------------------------------------------------------------------------------------
def runs_of(mask):
    """[(start, length)] of the runs of True in a 1-d mask"""
    m = np.concatenate([[False], mask, [False]])
    edge = np.flatnonzero(m[1:] != m[:-1])
    return [(int(a), int(b - a)) for a, b in zip(edge[0::2], edge[1::2])]


def interpolation_bound(ch, g, res, q=None):
    """A w^2 (g + 1)^2 / 8 + 2 q + 1: the chord error of a straight line over g + 1 sample steps of A sin(w n) (max |f''| h^2 / 8), the quantisation q of
    the two ends (0.5 for rounding; 14 bit: + 3 for the cleared bits; another format states its own q) and one for the integer arithmetic"""
    a, f, _ = SINE[ch]
    w = 2 * np.pi * f / RATE
    return a * w * w * (g + 1) ** 2 / 8 + 2 * ((0.5 if res == en.BIT16 else 3.5) if q is None else q) + 1


def check_t5(t, decoded, n_masked, mode, invalid, lead_audio=None, q=None):
    """T5: the audio stage against the signal.  decoded: the pair stream behind the audio stage, n_masked: what the call reported, invalid (pairs, 2): the
    samples the stitch output had marked invalid.  Every sample is the source's (T1's rule) and unmasked, or masked; *n_masked counts the MASKED flags;
    HOLD_WORD repeats the nearest earlier unmasked sample of the channel, INTER_LIN_WORD stays within interpolation_bound of the real-valued sine,
    MUTE_WORD leaves the source's sample or 0 - and a 0 that is not the source's only where the stitch output was invalid (it may lack MASKED: a sample
    that was 0 already is not flagged).  lead_audio, q: where source pair 0 comes out and the quantisation of a format that is not STC-007."""
    lead_audio = lead(t.d, True) if lead_audio is None else lead_audio
    off, got, flags = align(decoded, t.pcm)
    assert off == lead_audio, "source pair 0 at %d behind the audio stage, %d on the undamaged tape" % (off, lead_audio)
    audio = decoded[decoded["service_type"] == 0]
    assert n_masked == int(((audio["sample_flags"] & MASKED) != 0).sum()), "T5: *n_masked"
    masked_all = (audio["sample_flags"] & MASKED) != 0
    assert not masked_all[:off].any() and not masked_all[off + len(t.pcm):].any(), "T5: masked samples outside the source's span"
    masked = (flags & MASKED) != 0
    if mode == A.DROP_MUTE_WORD:
        _first(t, ~t.same(got) & (got != 0), "T5 mute: neither the source nor 0", got, flags)
        _first(t, ~t.same(got) & ~invalid, "T5 mute: altered where the stitch output was valid", got, flags)
        _first(t, masked & ~invalid, "T5 mute: masked where the stitch output was valid", got, flags)
        return
    _first(t, masked != invalid, "T5: masked is not 'the stitch output was invalid'", got, flags)
    _first(t, ~masked & ~t.same(got), "T5: unmasked and not the source", got, flags)
    real = sine(len(t.pcm))
    for ch in range(2):
        for start, g in runs_of(masked[:, ch]):
            assert start > 0 and start + g < len(t.pcm), "T5: a masked run at the edge of the source's span"
            for i in range(start, start + g):
                if mode == A.DROP_HOLD_WORD:
                    assert got[i, ch] == got[start - 1, ch], "T5 hold: %s holds %d, the sample before the run is %d" % (t.where(i, ch), got[i, ch], got[start - 1, ch])
                else:
                    assert mode == A.DROP_INTER_LIN_WORD
                    err, bound = abs(float(got[i, ch]) - real[i, ch]), interpolation_bound(ch, g, t.res, q)
                    assert err <= bound, "T5 interpolation: %s in a run of %d is %.1f off the signal, the bound is %.1f" % (t.where(i, ch), g, err, bound)
