"""Ground truth for the STC-007 decode path: damaged tapes must decode to their source.

The other suites prove "the same bytes as the oracle", and the oracle is a hand port of the reference.  Here the right answer is known for every sample:
tests/tape_truth.py makes a tape in numpy from PCM we choose (encode_api.tape_words / tape_frames, never the code under test), destroys lines of it by
a damage plan and predicts from the plan alone what can come back.  Every property is asserted first on the oracle, then on what sdv_decode_frames
makes of the luma in the call's own memory - the emulator build (test_emu_*) and the GPU (test_gpu_*), one body each (tests/test_twins.py) - and the
bytewise comparison with the oracle stays: these tapes are new inputs for the parity check too.

  T1  nothing wrong is called valid          T4  SDV_SF_WORD_FIXED and blocks_fix_p / _q say where the damage was
  T2  inside the code's reach all comes back  T5  the audio stage masks what was invalid, and stays near the signal
  T3  just outside, the loss is the plan's    T6  a tape in calls is the tape in one call

profiles/tape_truth_notes.md has the rules as derived from the reference, what was measured on the oracle and the plans taken out of a property."""
import functools

import numpy as np
import pytest

import audio_api as A
import device_calls as dc
import encode_api as en
import tape_truth as tt

NTSC, PAL, B14, B16, TFF, BFF = en.NTSC, en.PAL, en.BIT14, en.BIT16, en.TFF, en.BFF


def _c(plan, std=NTSC, res=B14, ctrl=0, order=TFF, audio="noise", n=4, how="black", height=None, top=0, seed=1):
    return dict(plan=plan, std=std, res=res, ctrl=ctrl, order=order, audio=audio, n=n, how=how, height=height, top=top, seed=seed)


def _geometries(plan, **kw):
    """a case on NTSC, on PAL (294 lines a field), with the control block on, and bottom field first.  BFF runs with the control block: without it the reference
    puts the first two frames of an UNDAMAGED file together top field first (notes, "plans taken out")."""
    return {"ntsc": _c(plan, **kw), "pal": _c(plan, std=PAL, **kw), "ctrl": _c(plan, ctrl=1, **kw), "bff_ctrl": _c(plan, ctrl=1, order=BFF, **kw)}


# ---- the matrix ---------------------------------------------------------------------------------------------------------------------------------
# ("burst", row0, B): B lines of one field of frame 1 on the picture rows row0 + 2 i
REACH = {}                      # T2 (+ T1, T4): the plan predicts no loss
for _row0, _B in ((100, 1), (100, 16), (100, 17), (100, 24), (100, 30), (200, 32)):
    for _g, _case in _geometries(("burst", _row0, _B)).items():
        REACH["14bit_%s_b%d_r%d" % (_g, _B, _row0)] = _case
for _g, _case in _geometries(("burst", 100, 1), res=B16).items():
    REACH["16bit_%s_b1_r100" % _g] = _case
# 16 bit: the longest bursts the oracle returns exactly for noise and for a sine alike (measured for 1 .. 20 lines): 14 lines at row 100, 13 at row 200
for _audio in ("noise", "sine"):
    REACH["16bit_%s_b14_r100" % _audio] = _c(("burst", 100, 14), res=B16, audio=_audio)
    REACH["16bit_%s_b13_r200" % _audio] = _c(("burst", 200, 13), res=B16, audio=_audio)
REACH["16bit_window_top2"] = _c(("window",), res=B16, height=486, top=2, n=3)        # test_encode's ntsc_16bit_top2: lines 0 and 1 of every field cut off
REACH["14bit_window_top2"] = _c(("window",), height=486, top=2, n=3)
REACH["14bit_random_bytes_b30_r100"] = _c(("burst", 100, 30), how="random", seed=11)   # (seed 11: no CRC collision on the oracle, the decode is exact)

EDGE = {}                       # T3 (+ T1, T4): the plan predicts which blocks are lost
for _B in (31, 32, 33, 40, 48):
    EDGE["14bit_ntsc_b%d_r100" % _B] = _c(("burst", 100, _B))
EDGE["14bit_pal_b31_r100"] = _c(("burst", 100, 31), std=PAL)
EDGE["14bit_ctrl_b33_r100"] = _c(("burst", 100, 33), ctrl=1)          # with the control block the first data line is read: 31 and 32 lines lose nothing (REACH)
EDGE["16bit_noise_b15_r100"] = _c(("burst", 100, 15), res=B16)        # the one above the longest exact burst at row 100
EDGE["16bit_sine_b15_r100"] = _c(("burst", 100, 15), res=B16, audio="sine")
for _B in (31, 32):
    for _g in ("ctrl", "bff_ctrl"):
        REACH["14bit_%s_b%d_r100" % (_g, _B)] = _geometries(("burst", 100, _B))[_g]
REACH["14bit_pal_ctrl_b30_r100"] = _c(("burst", 100, 30), std=PAL, ctrl=1)
REACH["14bit_pal_bff_ctrl_b30_r100"] = _c(("burst", 100, 30), std=PAL, ctrl=1, order=BFF)

HEAVY = {                       # T1 alone: whatever comes back as valid is the source's
    "14bit_scattered_2_black": _c(("scattered", 0.02, 3), n=5), "14bit_scattered_5_black": _c(("scattered", 0.05, 4), n=5),
    "14bit_scattered_5_random": _c(("scattered", 0.05, 4), n=5, how="random", seed=4),
    "14bit_scattered_20_random": _c(("scattered", 0.2, 5), n=3, how="random", seed=5),        # (seeds 4, 5: no CRC collision on the oracle)
    "14bit_sine_scattered_5_black": _c(("scattered", 0.05, 4), n=5, audio="sine"),
    "16bit_scattered_2_black": _c(("scattered", 0.02, 3), n=5, res=B16), "16bit_scattered_5_black": _c(("scattered", 0.05, 4), n=5, res=B16),
    "16bit_scattered_5_random": _c(("scattered", 0.05, 4), n=5, res=B16, how="random", seed=4),
    "16bit_sine_scattered_5_black": _c(("scattered", 0.05, 4), n=5, res=B16, audio="sine"),
    "16bit_b14_r200": _c(("burst", 200, 14), res=B16),      # the one above the longest exact burst at row 200: the field is taken for 14 bit, the low bits go
    "16bit_b16_r100": _c(("burst", 100, 16), res=B16), "16bit_sine_b16_r200": _c(("burst", 200, 16), res=B16, audio="sine"),
}
# Taken out of T1, by name (notes, "plans taken out"): what the reference itself does - the real reference gives the oracle's bytes on them.
PARITY_ONLY = {
    "14bit_scattered_20_black": _c(("scattered", 0.2, 5), n=3),                # black first / last lines move the trim, the padding is guessed one line off
    "16bit_scattered_20_black": _c(("scattered", 0.2, 5), n=3, res=B16),       # ... and fields taken for 14 bit "repair" two words with the S word as Q
    "16bit_scattered_20_random": _c(("scattered", 0.2, 5), n=3, res=B16, how="random", seed=5),
    "14bit_bff_b16_r100": _c(("burst", 100, 16), order=BFF),                   # BFF without the control block: the first two frames of the file are put together TFF
}
CASES = dict(REACH, **EDGE, **HEAVY, **PARITY_ONLY)
assert len(CASES) == len(REACH) + len(EDGE) + len(HEAVY) + len(PARITY_ONLY)
MATRIX = sorted(CASES)


# ---- tapes and the oracle's answers, made once -----------------------------------------------------------------------------------------------------
def _descriptor(c):
    return tt.geometry(c["std"], c["res"], c["ctrl"], c["order"], c["height"], c["top"])


def _plan(c, w9, d):
    kind = c["plan"][0]
    if kind == "burst":
        return tt.burst_at_row(w9, d, 1, c["plan"][1], c["plan"][2])
    if kind == "scattered":
        return tt.scattered(w9, c["plan"][1], c["plan"][2])
    assert kind == "window"
    return tt.window(w9, d)


@functools.lru_cache(maxsize=None)
def _tape(name):
    """(truth, damaged luma) of a case; the lines a short capture does not hold are part of every plan of its geometry"""
    c = CASES[name]
    d = _descriptor(c)
    pcm, w9, luma = tt.make_tape(c["std"], c["res"], c["n"], c["audio"], c["seed"] if c["audio"] == "noise" else 1, d)
    plan = _plan(c, w9, d) | tt.window(w9, d)
    return tt.Truth(pcm, plan, d), tt.apply(luma, plan, d, c["how"], c["seed"])


def _clean(name):
    """the name of the undamaged tape of a case's geometry and audio: cases that share it share its decodes"""
    c = dict(CASES[name], plan=("window",), how="black")
    if c["audio"] == "sine":
        c["seed"] = 1
    key = "clean:" + ",".join("%s=%s" % (k, c[k]) for k in sorted(c) if k not in ("plan", "how"))
    CASES.setdefault(key, c)
    return key


_decoded = {}


def _decode(who, name, make):
    """one decode per decoder and tape"""
    if (who, name) not in _decoded:
        _decoded[(who, name)] = make()
    return _decoded[(who, name)]


def _both(lib, via, oracle_lib, name, mask_mode=None):
    """[(who, pairs, descriptors, n_masked)]: the oracle first, then sdv_decode_frames through `via` - which has to give the oracle's bytes"""
    t, luma = _tape(name)
    want = _decode("oracle", (name, mask_mode), lambda: tt.oracle_decode(oracle_lib, luma, mask_mode))
    got = _decode(via.name, (name, mask_mode), lambda: tt.decode(via, lib, luma, mask_mode))
    assert got[0].tobytes() == want[0].tobytes(), "%s: the pair stream differs from the oracle's" % name
    assert got[1].tobytes() == want[1].tobytes(), "%s: the frame descriptors differ from the oracle's" % name
    assert got[2] == want[2], "%s: *n_masked %s, the oracle's %s" % (name, got[2], want[2])
    return [("oracle",) + tuple(want), (via.name,) + tuple(got)]


def _aligned(t, pairs, name, who):
    assert pairs["service_type"][0] == A.SRV_NEW_FILE and pairs["service_type"][-1] == A.SRV_END_FILE
    off, got, flags = tt.align(pairs, t.pcm)
    assert off == tt.lead(t.d), "%s on %s: source pair 0 at %d, %d on the undamaged tape" % (name, who, off, tt.lead(t.d))
    return got, flags


def _fix_counts(t, frames, clean_t, clean_frames, name, who):
    """T4, the descriptors: blocks_fix_p / blocks_fix_q summed over the tape, minus the undamaged tape's (its forced-bad first lines are repaired by P, 12 blocks a
    frame), are the plan's counts (tape_truth.Truth.fixes: the rule)"""
    got = tuple(int(frames[k].sum()) - int(clean_frames[k].sum()) for k in ("blocks_fix_p", "blocks_fix_q"))
    want = tuple(a - b for a, b in zip(t.fixes(), clean_t.fixes()))
    assert got == want, "%s on %s: the damage adds (P, Q) fixes %s, the plan says %s" % (name, who, got, want)
    assert (frames["blocks_fix_cwd"] == 0).all()


# ---- T1 - T4 on the stitch output --------------------------------------------------------------------------------------------------------------
def _truth(lib, via, oracle_lib, name):
    """One tape of the matrix at the stitch output (with_audio = 0).  The undamaged tape of its geometry: exact, source pair 0 is 240 pairs behind the NEW_FILE tag.
    REACH: T1, T2, T4.  EDGE: T1, T3 with the blocks tape_truth.Truth.lost predicts (three unread words of eight at 14 bit, two of seven at 16 bit, the
    forced-bad first line of a field without control block counted in), T4.  HEAVY: T1.  PARITY_ONLY: the bytes of the oracle."""
    t, _ = _tape(name)
    if name in REACH or name in EDGE:
        clean_t, _ = _tape(_clean(name))
        clean = _both(lib, via, oracle_lib, _clean(name))
        for who, pairs, frames, _ in clean:
            got, flags = _aligned(clean_t, pairs, "the undamaged tape of " + name, who)
            tt.check_t2(clean_t, got, flags, frames)
            tt.check_t4(clean_t, flags)
    for (who, pairs, frames, _), k in zip(_both(lib, via, oracle_lib, name), (0, 1)):
        if name in PARITY_ONLY:
            continue
        got, flags = _aligned(t, pairs, name, who)
        tt.check_t1(t, got, flags)
        if name in REACH:
            assert not t.lost.any(), "%s: the plan itself loses blocks %s" % (name, t.lost_blocks())
            tt.check_t2(t, got, flags, frames)
        elif name in EDGE:
            assert t.lost.any(), "%s: the plan loses nothing" % name
            tt.check_t3(t, got, flags, frames, t.lost_blocks())
            tt._first(t, ((flags & tt.VALID) == 0) != t.sample_invalid(), "T3: the invalid samples are not the unread words of the lost blocks", got, flags)
        if name in REACH or name in EDGE:
            tt.check_t4(t, flags)
            _fix_counts(t, frames, clean_t, clean[k][2], name, who)
        elif name == "16bit_b14_r200":
            assert tt.lost_blocks(flags) and not t.lost.any()       # past the reach, though the plan leaves every block repairable: notes, "16 bit"


@pytest.mark.parametrize("name", MATRIX)
def test_emu_truth(name, emu_lib, oracle_lib):
    _truth(dc.emu_lib_of(emu_lib), dc.HOST, oracle_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", MATRIX)
def test_gpu_truth(name, oracle_lib):
    _truth(dc.product_lib(), dc.DEVICE, oracle_lib, name)


# ---- T5: the audio stage -----------------------------------------------------------------------------------------------------------------------
# name: (case, samples the stitch output marks invalid).  14 bit: the counts are the plan's (Truth.sample_invalid) and the issue's; 16 bit: measured on the
# oracle - the stitcher distrusts every block across the frame seam there (notes, "16 bit"), which the plan does not predict
AUDIO = {"14bit_sine_b32_r100": (_c(("burst", 100, 32), audio="sine"), 6), "14bit_sine_b48_r200": (_c(("burst", 200, 48), audio="sine"), 240),
         "16bit_sine_b16_r100": (_c(("burst", 100, 16), res=B16, audio="sine"), None)}
LONG = {"16bit_sine_b16_r200_long": _c(("burst", 200, 16), res=B16, audio="sine")}       # a run of several hundred samples: bytes only
CASES.update({k: v[0] for k, v in AUDIO.items()}, **LONG)
WORD_MODES = {"hold": A.DROP_HOLD_WORD, "lin": A.DROP_INTER_LIN_WORD, "mute": A.DROP_MUTE_WORD}
BLOCK_MODES = {"hold_block": A.DROP_HOLD_BLOCK, "lin_block": A.DROP_INTER_LIN_BLOCK, "mute_block": A.DROP_MUTE_BLOCK}
AUDIO_RUNS = [(n, m) for n in sorted(AUDIO) + sorted(LONG) for m in sorted(WORD_MODES)] + \
             [(n, m) for n in ("14bit_sine_b48_r200",) + tuple(sorted(LONG)) for m in sorted(BLOCK_MODES)]


def _audio_stage(lib, via, oracle_lib, name, mode):
    """A sine tape through sdv_decode_frames with with_audio = 1.  Word modes (tape_truth.check_t5): *n_masked counts the MASKED flags, every sample is the
    source's or masked, the masked ones are exactly those the stitch output marked invalid; HOLD repeats the sample before the run, INTER_LIN stays within
    A w^2 (g + 1)^2 / 8 + 2 q + 1 of the real-valued sine for every masked sample (derived, not measured: 122 + 2 q for a single sample at 997 Hz), MUTE
    leaves the source or 0.  Block modes and the long 16-bit stretch: the oracle's bytes only, their ramps are not bounded here."""
    t, _ = _tape(name)
    if name in AUDIO and mode in WORD_MODES.values():
        invalid = None
        for who, pairs, frames, _ in _both(lib, via, oracle_lib, name):             # the stitch output of the same tape
            got, flags = _aligned(t, pairs, name, who)
            invalid = (flags & tt.VALID) == 0
            tt.check_t1(t, got, flags)
            if t.res == B14:
                assert np.array_equal(invalid, t.sample_invalid()) and int(invalid.sum()) == AUDIO[name][1], "%s: %d invalid samples" % (name, invalid.sum())
                assert set(g for ch in range(2) for _, g in tt.runs_of(invalid[:, ch])) <= {1, 2}
            else:
                assert invalid[t.sample_invalid()].all() and int(invalid.sum()) > 0
    for who, pairs, frames, n_masked in _both(lib, via, oracle_lib, name, mode):
        if name in AUDIO and mode in WORD_MODES.values():
            tt.check_t5(t, pairs, n_masked, mode, invalid)


@pytest.mark.parametrize("name,mode", AUDIO_RUNS)
def test_emu_audio_stage(name, mode, emu_lib, oracle_lib):
    _audio_stage(dc.emu_lib_of(emu_lib), dc.HOST, oracle_lib, name, dict(WORD_MODES, **BLOCK_MODES)[mode])


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", AUDIO_RUNS)
def test_gpu_audio_stage(name, mode, oracle_lib):
    _audio_stage(dc.product_lib(), dc.DEVICE, oracle_lib, name, dict(WORD_MODES, **BLOCK_MODES)[mode])


# ---- T6: streaming -----------------------------------------------------------------------------------------------------------------------------
STREAMS = {"6_frames": (_c(("scattered", 0.02, 20), n=6), [1, 2, 3]),          # the emulator twin's: half of the 12, for the time the emulator takes
           "12_frames": (_c(("scattered", 0.02, 21), n=12), [1, 2, 3, 6]), "40_frames": (_c(("scattered", 0.02, 22), n=40), [1, 7, 32])}
CASES.update({"stream_" + k: v[0] for k, v in STREAMS.items()})


def _streaming(lib, via, oracle_lib, name):
    """A 14-bit noise tape with 2 % of its lines black, uploaded once and decoded in calls that are views of it (NEW_FILE on the first, END_FILE on the last):
    the bytes of the one-call decode, which are the oracle's, and T1 and T4 on them."""
    t, luma = _tape("stream_" + name)
    (_, want_p, want_f, _), (_, one_p, one_f, _) = _both(lib, via, oracle_lib, "stream_" + name)
    got_p, got_f, _ = tt.decode(via, lib, luma, calls=STREAMS[name][1])
    assert got_p.tobytes() == one_p.tobytes() and got_f.tobytes() == one_f.tobytes()
    for pairs in (want_p, got_p):
        got, flags = _aligned(t, pairs, name, via.name)
        tt.check_t1(t, got, flags)
        tt.check_t4(t, flags, seams_may_be_unsafe=True)


@pytest.mark.parametrize("name", ["6_frames"])
def test_emu_streaming(name, emu_lib, oracle_lib):
    _streaming(dc.emu_lib_of(emu_lib), dc.HOST, oracle_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["6_frames", "12_frames", "40_frames"])
def test_gpu_streaming(name, oracle_lib):
    _streaming(dc.product_lib(), dc.DEVICE, oracle_lib, name)
