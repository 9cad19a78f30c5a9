"""Ground truth for the PCM-1 and PCM-16x0 (SI, EI) decode paths: damaged tapes must decode to their source.

The other suites of these formats prove "the same bytes as the oracle", and the oracle is a hand port of the reference.  Here the right answer is known for
every sample: tests/markerless_truth.py makes a tape in numpy from PCM we choose (encode_markerless_api.tape_bits / frames_of_bits, never the code under test),
destroys lines of it by a damage plan and predicts from the plan alone what can come back.  Every property is asserted first on the oracle, then on what
sdv_decode_frames makes of the luma in the call's own memory - the emulator build (test_emu_*) and the GPU (test_gpu_*), one body each (tests/test_twins.py) -
and the bytewise comparison with the oracle stays: these tapes are new inputs for the parity check too.

  T1  nothing wrong is called valid           T4  PCM-16x0: "valid block, no SDV_SF_WORD_FIXED" sits on what P repaired
  T2  inside the code's reach all comes back  T5  the audio stage masks what was invalid, and stays near the signal
  T3  just outside, the loss is the plan's    T6  a tape in calls is the tape in one call

profiles/markerless_truth_notes.md has the rules as derived from the reference, what was measured on the oracle and the plans taken out of a property."""
import functools

import numpy as np
import pytest

import audio_api as A
import device_calls as dc
import encode_markerless_api as ml
import markerless_truth as mt
import tape_truth as tt

PCM1, SI, EI, TFF, BFF = mt.PCM1, mt.SI, mt.EI, ml.TFF, ml.BFF


def _c(fmt, plan, order=TFF, n=3, how="black", hseed=0, audio="noise", flags=0, header=None, top=0, height=None, parts=(0, 1, 2), st=()):
    """a tape: format, damage plan, field order, frames, black rows or random bytes (hseed), audio, Control Bit flags, Header lines, the capture's first line and
    height, the sub-lines of a PCM-16x0 line the plan's rows lose, stitch settings other than the default"""
    return dict(fmt=fmt, plan=plan, order=order, n=n, how=how, hseed=hseed, audio=audio, flags=flags, header=header, top=top, height=height, parts=parts, st=st)


MANUAL = (("auto_offset", 0), ("odd_offset", -1), ("even_offset", -1))      # PCM-1 captured from line 2 on: one data line is missing above each field
# ---- the matrix: ("burst", row0, B[, frame]): B lines of one field of frame 1 on the picture rows row0 + 2 i ---------------------------------------
REACH = {                       # T2 (+ T1, T3's counts, T4): the plan predicts no loss
    "si_clean": _c(SI, ("none",)), "ei_clean": _c(EI, ("none",)), "pcm1_clean": _c(PCM1, ("none",)), "pcm1_bff_clean": _c(PCM1, ("none",), order=BFF),
    "si_b1": _c(SI, ("burst", 100, 1)), "si_b5": _c(SI, ("burst", 100, 5)), "si_b11": _c(SI, ("burst", 100, 11)),
    "si_bff_b11": _c(SI, ("burst", 100, 11), order=BFF), "si_b11_r101": _c(SI, ("burst", 101, 11)),
    "si_b11_frame0": _c(SI, ("burst", 100, 11, 0)), "si_b11_frame2_r300": _c(SI, ("burst", 300, 11, 2)),
    "si_random_b11": _c(SI, ("burst", 100, 11), how="random", hseed=11),
    "si_b40_part0": _c(SI, ("burst", 100, 40), parts=(0,)), "si_b40_part1": _c(SI, ("burst", 100, 40), parts=(1,)),       # one sub-line of three: columns 4 .. 240, 250 .. 470
    # lines 70 .. 74 of the field hold a copy of the Control Bits (35 i .. 35 i + 3): the pairs still carry rate and emphasis
    "si_flags_b5_r140": _c(SI, ("burst", 140, 5), flags=ml.RATE_44100 | ml.EMPHASIS), "ei_flags_b5_r140": _c(EI, ("burst", 140, 5), flags=ml.RATE_44100 | ml.EMPHASIS),
    "ei_b1": _c(EI, ("burst", 100, 1)), "ei_b12": _c(EI, ("burst", 100, 12)), "ei_b20": _c(EI, ("burst", 100, 20)), "ei_b31": _c(EI, ("burst", 100, 31)),
    "ei_bff_b20": _c(EI, ("burst", 100, 20), order=BFF), "ei_r100_r101_b10": _c(EI, ("bursts", (100, 10), (101, 10))),
    "ei_top2": _c(EI, ("none",), top=2, height=486), "ei_top2_b12": _c(EI, ("burst", 100, 12), top=2, height=486),
}
EDGE = {                        # T3 (+ T1, T4): the plan predicts which samples are lost
    "si_b12": _c(SI, ("burst", 100, 12)), "si_b13": _c(SI, ("burst", 100, 13)), "si_b20": _c(SI, ("burst", 100, 20)), "si_bff_b12": _c(SI, ("burst", 100, 12), order=BFF),
    "ei_two_bursts_163_apart": _c(EI, ("bursts", (100, 20), (100 + 2 * 163, 20))),
    # the long black burst: the first line of the NEXT field is the forced-bad one, and it holds the P words of the blocks whose first sub-lines are lines 81, 82
    "ei_b32": _c(EI, ("burst", 100, 32)), "ei_b33": _c(EI, ("burst", 100, 33)), "ei_b34": _c(EI, ("burst", 100, 34)), "ei_b35": _c(EI, ("burst", 100, 35)),
    "ei_b80": _c(EI, ("burst", 100, 80)),
    # PCM-1 fields that do not open with a Header line: the forced-bad first line is part of the prediction
    "pcm1_no_header": _c(PCM1, ("none",), header=0), "pcm1_no_header_b5": _c(PCM1, ("burst", 100, 5), header=0),
    "pcm1_header_row_black": _c(PCM1, ("burst", 0, 1)),
    "pcm1_top2_manual": _c(PCM1, ("none",), top=2, height=486, st=MANUAL), "pcm1_top2_manual_b5": _c(PCM1, ("burst", 100, 5), top=2, height=486, st=MANUAL),
}
# PCM-1: a black line costs its six samples.  A burst at row 100 first destroys two neighbouring pairs of a channel at the length the interleave gives; the
# bursts on either side of it are in the matrix beside the issue's
PCM1_DOUBLE = mt.pcm1_first_double(mt.geometry(PCM1), 100)
PCM1_BURSTS = {}
for _B in (1, 5, 15, 16, 20, PCM1_DOUBLE - 1, PCM1_DOUBLE):
    PCM1_BURSTS["pcm1_b%d" % _B] = _c(PCM1, ("burst", 100, _B))
    PCM1_BURSTS["pcm1_bff_b%d" % _B] = _c(PCM1, ("burst", 100, _B), order=BFF)
EDGE.update(PCM1_BURSTS)
HEAVY = {                       # T1: whatever comes back as valid is the source's
    "ei_random_b20": _c(EI, ("burst", 100, 20), how="random", hseed=7), "ei_random_b100": _c(EI, ("burst", 100, 100), how="random", hseed=7),
    "ei_b100": _c(EI, ("burst", 100, 100)),            # T1 only, by name: the padding of the frame is no longer proven and its first two blocks are masked (notes)
}
# scattered rows: (share, plan seed, frames).  The seeds are those on which the oracle neither moves the stream (black first rows of a field) nor meets a CRC
# collision (random bytes); notes, "seeds"
SCATTER = {PCM1: ((0.02, 15, 5), (0.05, 15, 5), (0.2, 15, 3)), SI: ((0.02, 3, 5), (0.05, 4, 5), (0.2, 10, 3)), EI: ((0.02, 3, 5), (0.05, 4, 5), (0.2, 5, 3))}
# Taken out of every property, by name (notes, "plans taken out"): what the reference itself does
PARITY_ONLY = {
    "si_top2": _c(SI, ("none",), top=2, height=486),                       # no way to tell the PCM-16x0 stitcher how many lines are missing above a field
    "pcm1_top2_auto": _c(PCM1, ("none",), top=2, height=486),              # ... and PCM-1's automatic offset pads a field without Header at the top
    "si_rows_0_2_4_black": _c(SI, ("burst", 0, 3)), "pcm1_rows_2_4_black": _c(PCM1, ("burst", 2, 2)),        # black first rows move the field
}
for _fmt, _nm in ((PCM1, "pcm1"), (SI, "si"), (EI, "ei")):
    for _p, _seed, _n in SCATTER[_fmt]:
        HEAVY["%s_scattered_%d_black" % (_nm, round(100 * _p))] = _c(_fmt, ("scattered", _p, _seed), n=_n)
        _into = PARITY_ONLY if (_fmt == PCM1 and _p > 0.02) else HEAVY      # PCM-1: one random line in 25 finds a level and a position at which its CRC fits
        _into["%s_scattered_%d_random" % (_nm, round(100 * _p))] = _c(_fmt, ("scattered", _p, _seed), n=_n, how="random", hseed=_seed)
EXACT = tuple(k for k in HEAVY if k.endswith("_black") and "scattered" in k)        # on these the oracle's loss is the plan's as well: T3 too
CASES = dict(REACH, **EDGE, **HEAVY, **PARITY_ONLY)
assert len(CASES) == len(REACH) + len(EDGE) + len(HEAVY) + len(PARITY_ONLY) and 6 * len(PARITY_ONLY) <= len(CASES)
MATRIX = sorted(CASES)
EMU_MATRIX = [k for k in MATRIX if not (k.endswith(("scattered_5_random", "scattered_20_random")))]        # 8 .. 11 s each on the emulator: the GPU twin's alone


# ---- tapes and the oracle's answers, made once -----------------------------------------------------------------------------------------------------
def _descriptor(c):
    return mt.geometry(c["fmt"], c["order"], c["flags"], c["header"], c["height"], c["top"])


def _plan(c, bits, d):
    kind = c["plan"][0]
    if kind == "none":
        return tt.no_damage(bits)
    if kind == "burst":
        return tt.burst_at_row(bits, d, c["plan"][3] if len(c["plan"]) > 3 else 1, c["plan"][1], c["plan"][2])
    if kind == "bursts":
        return np.logical_or.reduce([tt.burst_at_row(bits, d, 1, row0, B) for row0, B in c["plan"][1:]])
    assert kind == "scattered"
    return tt.scattered(bits, c["plan"][1], c["plan"][2])


@functools.lru_cache(maxsize=None)
def _tape(name):
    """(truth, damaged luma, stitch settings) of a case; the lines a short capture does not hold are part of every plan of its geometry"""
    c = CASES[name]
    d = _descriptor(c)
    pcm, bits, luma = mt.make_tape(d, c["n"], c["audio"])
    plan = _plan(c, bits, d) | tt.window(bits, d)
    if c["parts"] != (0, 1, 2):
        assert len(c["parts"]) == 1
        damaged = mt.apply_columns(luma, plan, d, *mt.PART_COLUMNS[c["parts"][0]])
    else:
        damaged = tt.apply(luma, plan, d, c["how"], c["hseed"])
    return mt.Truth(pcm, plan, d, c["parts"]), damaged, mt.settings(d, **dict(c["st"]))


_decoded = {}


def _decode(who, name, make):
    """one decode per decoder and tape"""
    if (who, name) not in _decoded:
        _decoded[(who, name)] = make()
    return _decoded[(who, name)]


def _both(lib, via, oracle_lib, name, mask_mode=None):
    """[(who, pairs, descriptors, n_masked)]: the oracle first, then sdv_decode_frames through `via` - which has to give the oracle's bytes"""
    t, luma, st = _tape(name)
    want = _decode("oracle", (name, mask_mode), lambda: mt.oracle_decode(oracle_lib, t.d, luma, st, mask_mode))
    got = _decode(via.name, (name, mask_mode), lambda: mt.decode(via, lib, t.d, luma, st, mask_mode))
    assert got[0].tobytes() == want[0].tobytes(), "%s: the pair stream differs from the oracle's" % name
    assert got[1].tobytes() == want[1].tobytes(), "%s: the frame descriptors differ from the oracle's" % name
    assert got[2] == want[2], "%s: *n_masked %s, the oracle's %s" % (name, got[2], want[2])
    return [("oracle",) + tuple(want), (via.name,) + tuple(got)]


def _aligned(t, pairs, name, who):
    assert pairs["service_type"][0] == A.SRV_NEW_FILE and pairs["service_type"][-1] == A.SRV_END_FILE
    off, got, flags = tt.align(pairs, t.pcm, search=64)
    assert off == mt.LEAD_STITCH, "%s on %s: source pair 0 at %d" % (name, who, off)
    return got, flags


# ---- T1 - T4 on the stitch output --------------------------------------------------------------------------------------------------------------
def _truth(lib, via, oracle_lib, name):
    """One tape of the matrix at the stitch output (with_audio = 0); source pair 0 is audio pair 0.  REACH: the plan loses nothing; T1, T2, T3's descriptor counts,
    T4.  EDGE: T1, T3 with the samples markerless_truth.Truth predicts, T4; PCM-1: the longest invalid run of a channel is the plan's.  HEAVY: T1 - and on the
    black scattered plans the loss is the plan's as well.  PARITY_ONLY: the bytes of the oracle."""
    t, _, _ = _tape(name)
    c = CASES[name]
    for who, pairs, frames, _ in _both(lib, via, oracle_lib, name):
        if name in PARITY_ONLY:
            continue
        got, flags = _aligned(t, pairs, name, who)
        tt.check_t1(t, got, flags)
        if name in REACH:
            assert not t.sample_invalid().any(), "%s: the plan itself loses samples" % name
            mt.check_t2(t, got, flags, frames)
        elif name in EDGE:
            assert t.sample_invalid().any(), "%s: the plan loses nothing" % name
        if name in REACH or name in EDGE or name in EXACT:
            mt.check_t3(t, got, flags, frames)
            if t.fmt != PCM1:
                mt.check_t4(t, flags)
            else:
                if name in PCM1_BURSTS:
                    longest = max(g for ch in range(2) for _, g in tt.runs_of((flags[:, ch] & tt.VALID) == 0))
                    want = mt.pcm1_longest_run(t.d, 100, c["plan"][2])
                    assert (want >= 2) == (c["plan"][2] >= PCM1_DOUBLE) and longest == want, "%s on %s: the longest invalid run is %d, the plan's %d" % (name, who, longest, want)
        if c["flags"]:
            audio = pairs[pairs["service_type"] == 0]
            assert (audio["sample_rate"] == (44100 if c["flags"] & ml.RATE_44100 else 44056)).all() and (audio["emphasis"] == (1 if c["flags"] & ml.EMPHASIS else 0)).all()


@pytest.mark.parametrize("name", EMU_MATRIX)
def test_emu_truth(name, emu_lib, oracle_lib):
    _truth(dc.emu_lib_of(emu_lib), dc.HOST, oracle_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", MATRIX)
def test_gpu_truth(name, oracle_lib):
    _truth(dc.product_lib(), dc.DEVICE, oracle_lib, name)


# ---- T5: the audio stage -----------------------------------------------------------------------------------------------------------------------
# name: (case, samples the stitch output marks invalid: the plan's count and the issue's)
AUDIO = {"pcm1_sine_b1": (_c(PCM1, ("burst", 100, 1), audio="sine"), 6), "pcm1_sine_b15": (_c(PCM1, ("burst", 100, 15), audio="sine"), 90),
         "pcm1_sine_b16": (_c(PCM1, ("burst", 100, 16), audio="sine"), 96),
         "si_sine_b12": (_c(SI, ("burst", 100, 12), audio="sine"), 3), "si_sine_b13": (_c(SI, ("burst", 100, 13), audio="sine"), 12)}
CASES.update({k: v[0] for k, v in AUDIO.items()})
WORD_MODES = {"hold": A.DROP_HOLD_WORD, "lin": A.DROP_INTER_LIN_WORD, "mute": A.DROP_MUTE_WORD}
AUDIO_RUNS = [(n, m) for n in sorted(AUDIO) for m in sorted(WORD_MODES)]


def _audio_stage(lib, via, oracle_lib, name, mode):
    """A tape_truth.SINE tape through sdv_decode_frames with with_audio = 1 (tape_truth.check_t5): *n_masked counts the MASKED flags, every sample is the source's or
    masked, the masked ones are exactly those the stitch output marked invalid - which are the plan's; HOLD repeats the sample before the run, INTER_LIN stays within
    A w^2 (g + 1)^2 / 8 + 2 q + 1 of the real-valued sine (q = 0.5 for PCM-16x0; 15.5 for PCM-1, whose companding drops four bits above 8191: the sine reaches
    12000 and 9000), MUTE leaves the source or 0.  The audio stage puts a silent pair in front and keeps the stream's last pair: the frames before the last are held
    against the source."""
    t, _, _ = _tape(name)
    invalid = None
    for who, pairs, frames, _ in _both(lib, via, oracle_lib, name):             # the stitch output of the same tape
        got, flags = _aligned(t, pairs, name, who)
        invalid = (flags & tt.VALID) == 0
        tt.check_t1(t, got, flags)
        assert np.array_equal(invalid, t.sample_invalid()) and int(invalid.sum()) == AUDIO[name][1], "%s on %s: %d invalid samples" % (name, who, invalid.sum())
        assert set(g for ch in range(2) for _, g in tt.runs_of(invalid[:, ch])) == {1}
    head = t.head(t.n_frames - 1)
    assert head.sample_invalid().sum() == invalid.sum()                         # the burst lies in frame 1
    for who, pairs, frames, n_masked in _both(lib, via, oracle_lib, name, mode):
        tt.check_t5(head, pairs, n_masked, mode, invalid[:len(head.pcm)], lead_audio=mt.LEAD_AUDIO, q=mt.Q[t.fmt])


@pytest.mark.parametrize("name,mode", AUDIO_RUNS)
def test_emu_audio_stage(name, mode, emu_lib, oracle_lib):
    _audio_stage(dc.emu_lib_of(emu_lib), dc.HOST, oracle_lib, name, WORD_MODES[mode])


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", AUDIO_RUNS)
def test_gpu_audio_stage(name, mode, oracle_lib):
    _audio_stage(dc.product_lib(), dc.DEVICE, oracle_lib, name, WORD_MODES[mode])


# ---- T6: streaming -----------------------------------------------------------------------------------------------------------------------------
# 2 % of the rows black, the plan seeds of the matrix; the 6-frame tapes in calls of 1, 2, 3 are the emulator twin's: half of the 12 in calls of 1, 2, 3, 6
STREAMS = {"%s_%d_frames" % (nm, n): (_c(fmt, ("scattered", 0.02, SCATTER[fmt][0][1]), n=n), calls)
           for fmt, nm in ((PCM1, "pcm1"), (SI, "si"), (EI, "ei")) for n, calls in ((6, [1, 2, 3]), (12, [1, 2, 3, 6]))}
CASES.update({"stream_" + k: v[0] for k, v in STREAMS.items()})


def _streaming(lib, via, oracle_lib, name):
    """A noise tape with 2 % of its rows black, uploaded once and decoded in calls that are views of it (NEW_FILE on the first, END_FILE on the last): the bytes of
    the one-call decode, which are the oracle's, and T1 on them - and T3: on these six tapes the oracle's loss is the plan's."""
    t, luma, st = _tape("stream_" + name)
    (_, want_p, want_f, _), (_, one_p, one_f, _) = _both(lib, via, oracle_lib, "stream_" + name)
    got_p, got_f, _ = mt.decode(via, lib, t.d, luma, st, calls=STREAMS[name][1])
    assert got_p.tobytes() == one_p.tobytes() and got_f.tobytes() == one_f.tobytes()
    for pairs, frames in ((want_p, want_f), (got_p, got_f)):
        got, flags = _aligned(t, pairs, name, via.name)
        tt.check_t1(t, got, flags)
        mt.check_t3(t, got, flags, frames)


@pytest.mark.parametrize("name", sorted(k for k in STREAMS if k.endswith("_6_frames")))
def test_emu_streaming(name, emu_lib, oracle_lib):
    _streaming(dc.emu_lib_of(emu_lib), dc.HOST, oracle_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(STREAMS))
def test_gpu_streaming(name, oracle_lib):
    _streaming(dc.product_lib(), dc.DEVICE, oracle_lib, name)
