"""The stages of the engine, each with its compact cases, for tests/test_memory_history.py: no result may depend on what memory held before the call.

The engines' device and pinned buffers (rt::DevBuf / rt::PinBuf, csrc/runtime.inc) are handed out unzeroed, and the design relies on every kernel
writing an entry before anything reads it.  A fresh engine in a young process hides a read of a never-written counter or flag behind the zero pages
it usually gets; so does a caller's output buffer that starts zeroed.  The table below runs every stage

  (a) with every allocation of the engine prefilled with a byte (sdv_emu_poison_alloc on the emulator build; SDV_POISON_ALLOC and the developer build
      of the HIP library on the GPU, in a child process: gpu_child),
  (b) on an engine with a past: a larger case with other settings first, the stage's start-over entry, then the compact cases forwards and backwards,
  (c) through caller buffers that start as 0xA5 bytes (device_calls.Host / Device with dirty=True),

and every output is held to the reference the stage's own test module holds it to: the plain-C oracle, the float64 walks of the sample-stream modules with
their `check`, the numpy references of the encoders and the ingest stage.  Nothing here restates a reference.

A stage is (cases, past, start_over, run): run(lib, eng, c, case, check) makes the calls of one case on the engine `eng` of the library `lib` (bound with
abi.bind) through the memory `c` (a device_calls.Calls) and asserts - naming the field and the record - that the outputs are the reference's; check=False
(the past) only makes the calls.  LDS is out of reach from the host and not covered."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import time

import numpy as np

import audio_api as A
import device_calls as dc
import engine_api as ea
import libs
from sdvpcmdecoder_amd import abi
from stitch_api import PAIR_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON_BYTES = (0x55, 0xFF)
STC007, PCM1, PCM16X0 = abi.PCM_STC007, abi.PCM_PCM1, abi.PCM_PCM16X0


def memory(kind, dirty=False):
    """The calls of device_calls over host or device memory; dirty: output buffers start as PATTERN bytes."""
    return dc.Calls(dc.Host(dirty) if kind == "host" else dc.Device(dirty))


def same(what, got, want):
    """Byte equality of two record arrays, padding included; the message names the first record and the first field that differ."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert len(got) == len(want), "%s: %d records, the reference has %d" % (what, len(got), len(want))
    if got.tobytes() == want.tobytes():
        return
    size = got.dtype.itemsize
    a, b = got.view(np.uint8).reshape(len(got), -1), want.view(np.uint8).reshape(len(want), -1)
    assert a.shape == b.shape, "%s: records of %d bytes, the reference's have %d" % (what, a.shape[1], b.shape[1])
    i = int(np.nonzero((a != b).any(axis=1))[0][0])
    for nm in got.dtype.names or ():
        if np.asarray(got[nm][i]).tobytes() != np.asarray(want[nm][i]).tobytes():
            raise AssertionError("%s: record %d of %d, field %s: %s, the reference has %s" % (what, i, len(got), nm, got[nm][i], want[nm][i]))
    at = int(np.nonzero(a[i] != b[i])[0][0])
    raise AssertionError("%s: record %d of %d, byte %d of %d (no named field: padding): 0x%02X, the reference has 0x%02X" % (what, i, len(got), at, size, a[i, at], b[i, at]))


def _ok(lib, eng, rc):
    assert rc == 0, lib.sdv_last_error(eng)


# ---- sdv_binarize_frames ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bf_case(case):
    """-> [(luma, flags, wanted records, wanted stats) per call]"""
    import kernel_path_tapes as kt
    from oracle_run import oracle_binarize
    from sdvpcmdecoder_amd import synth
    if case == "worn_3x64":                 # damage in every frame: the sweep pool, the memos and the snapshots are in play
        luma = kt.worn_tape(3, 64, seed=32)
        return [(luma, 1) + tuple(oracle_binarize(luma, mode=2))]
    if case == "worn_10x64":
        return [(kt.worn_tape(10, 64), 1, None, None)]
    assert case == "end_of_file_and_next_source"        # the tapes of test_emu_end_of_file_frame_and_next_source: a second source behind an END_FILE call
    luma, _, _ = synth.stc007_frames(n_frames=3, seed=21, height=48, noise_sigma=3.0)
    luma2, _, _ = synth.stc007_frames(n_frames=2, seed=22, height=48, x0=20, x1=690)
    orc = libs.load_oracle()
    orc.orc_v2d_new.restype = C.c_void_p
    h = C.c_void_p(orc.orc_v2d_new())
    orc.orc_v2d_set_mode.argtypes = [C.c_void_p, C.c_int]
    orc.orc_v2d_set_mode(h, 2)
    w1 = oracle_binarize(luma, handle=h, new_file=True, end_file=True)
    w2 = oracle_binarize(luma2, handle=h, new_file=True, first_frame_no=1)
    return [(luma, 1 | 4) + tuple(w1), (luma2, 1) + tuple(w2)]


def _binarize_frames(lib, eng, c, case, check=True):
    assert lib.sdv_set_mode(eng, 2) == 0
    for k, (luma, flags, want, want_stats) in enumerate(_bf_case(case)):
        rc, recs, stats = c.binarize(lib, eng, luma, flags=flags)
        _ok(lib, eng, rc)
        if check:
            same("call %d: line records" % k, recs, want)
            same("call %d: frame stats" % k, stats.view(np.uint8), np.frombuffer(want_stats.tobytes(), dtype=np.uint8))
    if case.startswith("worn"):
        info = ea.RunInfo()
        assert lib.sdv_get_run_info(eng, C.byref(info)) == 0
        assert info.sweeps > 0 and info.frames_general > 0, "the tape did not reach the sweep pool"


# ---- sdv_binarize_lines -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bl_case(case):
    """-> (rows, frame, first line, line step, wanted records): the 96-line call of test_gpu_kernel_paths (cold lines, every second line of frame 9), and a
    larger one for the past"""
    import kernel_path_tapes as kt
    from sdvpcmdecoder_amd import synth
    from test_stc_lines import _oracle_lines
    luma, _, _ = synth.stc007_frames(1, seed=17, noise_sigma=4.0)
    rows = np.ascontiguousarray(kt.unreadable_cells(luma, every=97).reshape(-1, 720))
    if case == "lines_300":
        return np.ascontiguousarray(rows[100:400]), 3, 101, 1, None
    small = np.ascontiguousarray(rows[:96])
    return small, 9, 5, 2, _oracle_lines(small, None, 2, first_line=5, line_step=2, frame=9)


def _binarize_lines(lib, eng, c, case, check=True):
    rows, frame, first, step, want = _bl_case(case)
    assert lib.sdv_set_mode(eng, 2) == 0
    src, out = c.array(rows), c.zeros(len(rows), libs.LINE_DTYPE)
    _ok(lib, eng, lib.sdv_binarize_lines(eng, c.ptr(src), rows.shape[1], rows.shape[1], len(rows), None, frame, first, step, 0, c.ptr(out), len(out), c.stream()))
    got = c.get(out)
    if check:
        same("line records", got, want)


# ---- the three stitchers ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stitch_case(case):
    import stitch_api as sa
    import stitch_cases as sc
    from oracle_run import oracle_binarize
    recs, st = sc.make_input(case, lambda luma: oracle_binarize(luma, mode=2))
    return recs, st, (sa.run_cpu(libs.load_oracle(), "orc_", recs, st) if case != "ntsc_drift" else None)


def _stitch(lib, eng, c, case, check=True):
    recs, st, want = _stitch_case(case)
    rc, pairs, frames = c.stitch(lib, eng, recs, st)
    _ok(lib, eng, rc)
    if check:
        same("pairs", pairs, want[0])
        same("frame descriptors", frames, want[1])


@functools.lru_cache(maxsize=None)
def _pcm1_case(case):
    import pcm1_api as p1
    recs, st = p1.make_input(case)
    return recs, st, (p1.run_cpu_vis(libs.load_oracle(), "orc_", recs, st) if case != "manual_lost_many" else None)


def _pcm1_stitch(lib, eng, c, case, check=True):
    """with block and line outputs armed"""
    recs, st, want = _pcm1_case(case)
    rc, pairs, frames, blocks, lines = c.pcm1_stitch_vis(lib, eng, recs, st)
    _ok(lib, eng, rc)
    if check:
        same("pairs", pairs, want[0])
        same("frame descriptors", frames, want[1])
        same("blocks", blocks, want[2])
        same("sub-lines", lines, want[3])


@functools.lru_cache(maxsize=None)
def _pcm16_case(case):
    import pcm16_api as p16
    recs, st = p16.make_input(case)
    return recs, st, (p16.run_cpu_vis(libs.load_oracle(), "orc_", recs, st) if case != "ei_wander" else None)


def _pcm16_stitch(lib, eng, c, case, check=True):
    """with the block output armed"""
    recs, st, want = _pcm16_case(case)
    rc, pairs, frames, blocks = c.pcm16_stitch_vis(lib, eng, recs, st)
    _ok(lib, eng, rc)
    if check:
        same("pairs", pairs, want[0])
        same("frame descriptors", frames, want[1])
        same("blocks", blocks, want[2])


# ---- the PCM-1 and PCM-16x0 frame drivers ---------------------------------------------------------------------------------------------------------
def _frames_api(fmt):
    import pcm1_frames_api
    import pcm16_frames_api
    return pcm1_frames_api if fmt == PCM1 else pcm16_frames_api


@functools.lru_cache(maxsize=None)
def _frames_case(fmt, case):
    pf = _frames_api(fmt)
    luma, mode, st = pf.make_input(case)
    return luma, mode, st, (pf.run_cpu(libs.load_oracle(), "orc_", luma, mode, st) if case != "ntsc_full" else None)


def _frames_driver(fmt):
    def run(lib, eng, c, case, check=True):
        luma, mode, st, want = _frames_case(fmt, case)
        rc, recs, stats = c.frames(lib, _frames_api(fmt), eng, luma, mode, st)
        _ok(lib, eng, rc)
        if check:
            same("line records", recs, want[0])
            same("frame stats", stats, want[1])
    return run


# ---- sdv_decode_frames ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _decode_case(fmt):
    """The smallest tape of test_decode_frames per type, and the oracle's workers one after the other -> (luma, pairs, frame descriptors, frame stats)"""
    import pcm1_api as p1
    import pcm16_api as p16
    import test_decode_frames as td
    from stream_scenarios import bin_to_line_recs
    orc = libs.load_oracle()
    luma = np.ascontiguousarray(td._tape(fmt, 3))
    if fmt == STC007:
        return (luma,) + tuple(td._oracle_chain(orc, luma))
    pf = _frames_api(fmt)
    recs, stats = pf.run_cpu(orc, "orc_", luma, 2, dict(new_file=True, end_file=True))
    pairs, frames = p1.run_cpu(orc, "orc_", bin_to_line_recs(recs), p1.default_settings()) if fmt == PCM1 else p16.run_cpu(orc, "orc_", recs, p16.default_settings())
    return luma, pairs, frames, stats


def _decode_reset(lib, eng, c):
    """every stage of the fused entry starts over, with the settings it has by default"""
    import pcm1_api as p1
    import pcm16_api as p16
    assert lib.sdv_reset_stream(eng) == 0 and lib.sdv_reset_stitcher(eng) == 0
    assert lib.sdv_set_pcm1_stitch_settings(eng, C.byref(p1.default_settings())) == 0
    assert lib.sdv_set_pcm16x0_stitch_settings(eng, C.byref(p16.default_settings())) == 0


def _decode(lib, eng, c, case, check=True):
    import test_decode_frames as td
    fmt = {"stc007": STC007, "pcm1": PCM1, "pcm16x0": PCM16X0}[case]
    luma, want_p, want_f, want_s = _decode_case(fmt)
    assert lib.sdv_set_mode(eng, 2) == 0 and lib.sdv_set_pcm_type(eng, fmt, 0) == 0
    pairs, frames, stats, _, _ = td._fused_host(lib, eng, fmt, luma, with_audio=False, via=c)
    if check:
        same("pairs", pairs, want_p)
        same("frame descriptors", frames, want_f)
        same("frame stats", stats.view(np.uint8), np.frombuffer(want_s.tobytes(), dtype=np.uint8))
    return pairs.tobytes() + frames.tobytes() + stats.tobytes()


# ---- sdv_audio_process ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _audio_case(case):
    """the 9000-pair tape of test_alloc_failure in its two calls -> (pairs, mode, wanted out, purges, masked)"""
    import conceal_walk
    from test_alloc_failure import STREAM_CUTS, audio_process_tape
    if case == "long_hold":
        return A.tape([A.audio(20000, 51, runs=((500, 9, 0), (12000, 40, 1)), p_bad=0.02), "E"]), abi.DROP_HOLD_WORD, None, None, None
    pairs, ends = audio_process_tape(), np.array(STREAM_CUTS[1:], dtype=np.uint64)
    if case == "inter_lin_word":
        out, _, pur, masked, hit = A.run_cpu(libs.load_oracle(), "orc_", pairs, abi.DROP_INTER_LIN_WORD, ends, 1)
        assert hit == 0
        return pairs, abi.DROP_INTER_LIN_WORD, out, pur, masked
    out, pur, masked, _ = conceal_walk.run(pairs, abi.DROP_INTER_CUBIC_WORD, [int(e) for e in ends], 1)
    return pairs, abi.DROP_INTER_CUBIC_WORD, out, pur, masked


def _audio_process(lib, eng, c, case, check=True):
    from test_alloc_failure import STREAM_CUTS
    pairs, mode, want, want_pur, want_masked = _audio_case(case)
    assert lib.sdv_set_audio_masking(eng, mode) == 0
    cuts = (0, len(pairs)) if not check else STREAM_CUTS
    outs, purs, masked, got = [], [], 0, 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        rc, o, p, m, _, _ = c.audio(lib, eng, pairs[a:b], 1 if b == cuts[-1] else 0)
        _ok(lib, eng, rc)
        p = p.copy()
        p["first_pair"] += got
        p["tag_index"] += a
        outs.append(o.copy()); purs.append(p); masked += m
        got += len(o)
    if check:
        same("pairs", np.concatenate(outs), want)
        same("purges", np.concatenate(purs), want_pur)
        assert masked == want_masked, "masked samples: %d, the reference has %d" % (masked, want_masked)


# ---- the sample-stream stages: 9000 pairs in the two calls of STREAM_CUTS ---------------------------------------------------------------------------
def _in_calls(n, check):
    from test_alloc_failure import STREAM_CUTS
    cuts = STREAM_CUTS if check else (0, n)
    return [(a, b, b == cuts[-1]) for a, b in zip(cuts[:-1], cuts[1:])]


@functools.lru_cache(maxsize=None)
def _deemph_case(case):
    import test_deemphasis as TD
    from test_alloc_failure import deemphasis_tape
    if case == "noise_auto_44100":
        return TD.stream("noise", 20000, seed=7, rate=44100, emphasis=1), TD.AUTO, None
    pairs = deemphasis_tape()
    return pairs, TD.FORCE, TD.walk(pairs, TD.FORCE)[0]


def _deemphasis(lib, eng, c, case, check=True):
    import test_deemphasis as TD
    pairs, mode, want = _deemph_case(case)
    assert lib.sdv_set_deemphasis(eng, mode) == 0
    got = []
    for a, b, _ in _in_calls(len(pairs), check):
        src, out = c.array(pairs[a:b]), c.zeros(b - a, PAIR_DTYPE)
        _ok(lib, eng, lib.sdv_audio_deemphasis(eng, c.ptr(src), b - a, c.ptr(out), c.stream()))
        got.append(c.get(out))
    if check:
        TD.check(np.concatenate(got), want)


@functools.lru_cache(maxsize=None)
def _resample_case(mode):
    import test_deskew as DS
    import test_resample as R
    from test_alloc_failure import resample_tape
    if mode == "past":
        return R.stream("noise", 20000, seed=9), R.ON | DS.LEFT, None
    pairs = resample_tape()
    return pairs, mode, (R.walk(pairs) if mode == R.ON else DS.expected(pairs, mode))


def _resample(lib, eng, c, case, check=True):
    import test_deskew as DS
    import test_resample as R
    pairs, mode, want = _resample_case(case if case == "past" else int(case[4:]))
    assert lib.sdv_set_resample(eng, mode) == 0
    got = []
    for a, b, last in _in_calls(len(pairs), check):
        cap = lib.sdv_audio_resample_room(eng, b - a)
        src, out, n_out = c.array(pairs[a:b]), c.zeros(cap, PAIR_DTYPE), C.c_size_t(0)
        _ok(lib, eng, lib.sdv_audio_resample(eng, c.ptr(src), b - a, 1 if last else 0, c.ptr(out), cap, C.byref(n_out), c.stream()))
        got.append(c.get(out, n_out.value))
    if check:
        (R.check if mode == R.ON else DS.check)(np.concatenate(got), want)


@functools.lru_cache(maxsize=None)
def _pcm_case(stage, case):
    import test_pcm_preemphasis as TP
    import test_pcm_resample as TR
    from test_alloc_failure import pcm_tape
    if case == "noise_20000":
        return TR.signal("noise", 20000, seed=3), None
    pcm = pcm_tape()
    return pcm, (TP.walk(pcm, 44100)[0] if stage == "preemphasis" else TR.walk(pcm))


def _preemphasis(lib, eng, c, case, check=True):
    import pcm_condition_api as P
    pcm, want = _pcm_case("preemphasis", case)
    got = []
    for a, b, _ in _in_calls(len(pcm), check):
        src, out = c.array(pcm[a:b]), c.zeros(2 * (b - a), np.int16)
        _ok(lib, eng, lib.sdv_pcm_preemphasis(eng, c.ptr(src), b - a, 44100 if check else 44056, c.ptr(out), c.stream()))
        got.append(c.get(out).reshape(-1, 2))
    if check:
        P.check(np.concatenate(got), want)


def _pcm_resample(lib, eng, c, case, check=True):
    import pcm_condition_api as P
    pcm, want = _pcm_case("resample", case)
    got = []
    for a, b, last in _in_calls(len(pcm), check):
        cap = lib.sdv_pcm_resample_room(eng, b - a)
        src, out, n_out = c.array(pcm[a:b]), c.zeros(2 * cap, np.int16), C.c_size_t(0)
        _ok(lib, eng, lib.sdv_pcm_resample(eng, c.ptr(src), b - a, 1 if last else 0, c.ptr(out), cap, C.byref(n_out), c.stream()))
        got.append(c.get(out, 2 * n_out.value).reshape(-1, 2))
    if check:
        P.check(np.concatenate(got), want)


# ---- the visualiser: one kind of each family, on what the stitch cases above read and produced -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _vis_case(case):
    import render_api as ra
    if case == "stc_lines_drift":
        recs = _stitch_case("ntsc_drift")[0]
        return ra.STC007, np.ascontiguousarray(recs[:int(np.nonzero(recs["service_type"] == 5)[0][2]) + 1]), None, None      # (three frames of another tape)
    if case == "stc_lines":
        recs = _stitch_case("ntsc_bad10_no_pq")[0]
        return ra.STC007, recs, None, ra.run_oracle(ra.STC007, recs)[0]
    if case == "pcm1_blocks":
        blocks = np.ascontiguousarray(_pcm1_case("clean")[2][2])
        per = np.full(len(blocks) // 16, 16, dtype=np.uint32)
        return ra.PCM1_BLOCKS, blocks, per, ra.run_oracle_blocks(ra.PCM1_BLOCKS, blocks, per)[0]
    kind, lines, per = ra.make_asm_input("asm_bad10_cwd")           # (the assembled lines of ntsc_bad10_no_pq)
    return kind, lines, per, ra.run_oracle_asm(kind, lines, per)[0]


def _vis(lib, eng, c, case, check=True):
    kind, recs, per, want = _vis_case(case)
    assert lib.sdv_vis_reset(eng, kind, c.stream()) == 0
    if per is None:
        rc, got, _ = c.render_lines(lib, eng, kind, recs)
    else:
        fn = "sdv_vis_render_blocks" if case == "pcm1_blocks" else "sdv_vis_render_asm_lines"
        rc, got = c.render_rows(lib, fn, eng, kind, c.array(recs), len(recs), per)
    _ok(lib, eng, rc)
    if check:
        assert got.shape == want.shape, (got.shape, want.shape)
        bad = np.argwhere(got != want)
        assert not len(bad), "canvas %d, row %d, pixel %d: 0x%08X, the reference has 0x%08X (%d pixels differ)" % (
            tuple(bad[0]) + (got[tuple(bad[0])], want[tuple(bad[0])], len(bad)))


def _vis_reset(lib, eng, c):
    import render_api as ra
    for kind in (ra.STC007, ra.PCM1_BLOCKS, ra.STC007_ASM_NTSC):
        assert lib.sdv_vis_reset(eng, kind, c.stream()) == 0


# ---- the encoders and the ingest stage: widths 137 and 720, two frames of height 6 to 48 --------------------------------------------------------------
ENCODE_SHAPES = {"137x6": (137, 6, 10, 130), "720x48": (720, 48, 12, 708)}      # width, height, data window


def _encode(lib, eng, c, case, check=True):
    import encode_api as en
    assert lib.sdv_reset_encoder(eng) == en.OK
    rng = np.random.default_rng(600)
    if case == "pal_16bit_720x100":
        d = en.desc(en.PAL, en.BIT16, 1, 0, en.BFF, 16, 235, (1, 2, 3, 4, 5), 720, 100, 0, 720, 0)
        pcm = rng.integers(-32768, 32768, size=(en.pairs_per_frame(en.PAL), 2), dtype=np.int16)
        en.run_call(c, lib, eng, d, pcm, len(pcm), 1, en.tape_frames(en.tape_words(pcm, 1, en.PAL, en.BIT16, 1, 0, (1, 2, 3, 4, 5)), d))
        return
    w, h, start, stop = ENCODE_SHAPES[case]
    d = en.desc(width=w, height=h, data_start=start, data_stop=stop)
    pcm = rng.integers(-32768, 32768, size=(2 * en.pairs_per_frame(en.NTSC), 2), dtype=np.int16) & ~3
    en.run_call(c, lib, eng, d, pcm, len(pcm), 2, en.tape_frames(en.tape_words(pcm, 2), d), dst_off=3, dst_pad=6, frame_pad=10)


def _encode_markerless(lib, eng, c, case, check=True):
    import encode_api as en
    import encode_markerless_api as ml
    assert lib.sdv_reset_encoder(eng) == en.OK
    rng = np.random.default_rng(601)
    fmt, shape = case.split("_")
    fmt = {"pcm1": ml.PCM1, "si": ml.SI, "ei": ml.EI}[fmt]
    w, h, start, stop = ENCODE_SHAPES[shape] if shape in ENCODE_SHAPES else (720, 100, 4, 716)
    d = ml.desc(fmt, width=w, height=h, data_start=start, data_stop=stop)
    pcm = rng.integers(-32768, 32768, size=(2 * ml.PAIRS_PER_FRAME, 2), dtype=np.int16)
    ml.run_call(c, lib, eng, d, pcm, len(pcm), 2, ml.tape_frames(pcm, 2, d), dst_off=3, dst_pad=6, frame_pad=10)


def _encode_packed(lib, eng, c, case, check=True):
    import encode_api as en
    import encode_packed_api as ep
    import test_encode_packed as TEP
    assert lib.sdv_reset_encoder(eng) == en.OK
    fmt, shape = case.split("_")
    w, h, start, stop = ENCODE_SHAPES[shape]
    enc = "stc_ntsc_14bit_ctrl" if fmt == "v210" else "pcm16x0_si"
    pcm = TEP._two_frames(enc)[0]
    d, planes = TEP._desc_and_planes(enc, 0, 30, 200, w, h, start, stop, 0)
    ep.with_fmt(d, ep.PACKED[fmt])
    ep.run_call(c, lib, eng, d, pcm, len(pcm), 2, planes, dst_off=3, dst_pad=6, frame_pad=10)


def _ingest(lib, eng, c, case, check=True):
    import ingest_api as ia
    fmt, shape = case.split("_")
    w, h = ENCODE_SHAPES[shape][:2] if shape in ENCODE_SHAPES else (1920, 64)
    ia.run_case(c, lib, eng, np.random.default_rng(602), ia.FORMATS[fmt], w, h, n=2, double=ia.ON if fmt == "v210" else ia.OFF, dst_off=1, dst_pad=6)


# ---- the table ------------------------------------------------------------------------------------------------------------------------------------
class Stage:
    def __init__(self, run, cases, past=None, start_over=None, allocates=True):
        self.run, self.cases, self.past, self.start_over = run, list(cases), past, start_over
        self.allocates = allocates          # False: the stage owns no engine memory (nothing for (a) to fill; (b) and (c) still hold)


def _entry(*names):
    def start_over(lib, eng, c):
        for nm in names:
            assert getattr(lib, nm)(eng) == 0, nm
    return start_over


def _frame_cases(fmt):
    """the first case of the driver's table and the one with the most repaired frames: jitter_draft launches 14 frames for its 4 in four rounds (PCM-1) and 13
    in three (PCM-16x0, as many as dropouts_draft) - counted on the emulator from sdv_get_run_info over every case of the tables"""
    cases = list(_frames_api(fmt).CASES)
    return [cases[0], "jitter_draft"]


STAGES = {
    "binarize_frames": Stage(_binarize_frames, ["worn_3x64", "end_of_file_and_next_source"], "worn_10x64", _entry("sdv_reset_stream")),
    "binarize_lines": Stage(_binarize_lines, ["lines_96"], "lines_300", _entry("sdv_reset_stream")),
    "stitch_frames": Stage(_stitch, ["ntsc_bad10_no_pq"], "ntsc_drift", _entry("sdv_reset_stitcher")),
    # (their start-over entry is sdv_set_pcm1_stitch_settings / sdv_set_pcm16x0_stitch_settings: every case begins with it)
    "pcm1_stitch_frames": Stage(_pcm1_stitch, ["clean"], "manual_lost_many"),
    "pcm16x0_stitch_frames": Stage(_pcm16_stitch, ["si_bad10"], "ei_wander"),
    "pcm1_binarize_frames": Stage(_frames_driver(PCM1), _frame_cases(PCM1), "ntsc_full", _entry("sdv_reset_stream")),
    "pcm16x0_binarize_frames": Stage(_frames_driver(PCM16X0), _frame_cases(PCM16X0), "ntsc_full", _entry("sdv_reset_stream")),
    "decode_frames": Stage(_decode, ["stc007", "pcm1", "pcm16x0"], None, _decode_reset),
    "audio_process": Stage(_audio_process, ["inter_lin_word", "inter_cubic_word"], "long_hold", _entry("sdv_reset_audio")),
    "audio_deemphasis": Stage(_deemphasis, ["tape_force"], "noise_auto_44100", _entry("sdv_reset_deemphasis")),
    "audio_resample": Stage(_resample, ["mode1", "mode4", "mode5"], "past", _entry("sdv_reset_resample")),
    "pcm_preemphasis": Stage(_preemphasis, ["tape_44100"], "noise_20000", _entry("sdv_reset_preemphasis")),
    "pcm_resample": Stage(_pcm_resample, ["tape"], "noise_20000", _entry("sdv_reset_pcm_resample")),
    "vis_render": Stage(_vis, ["stc_lines", "pcm1_blocks", "stc_asm_lines"], "stc_lines_drift", _vis_reset),
    "encode_frames": Stage(_encode, list(ENCODE_SHAPES), "pal_16bit_720x100", _entry("sdv_reset_encoder")),
    "encode_markerless_frames": Stage(_encode_markerless, ["pcm1_137x6", "si_720x48"], "ei_past", _entry("sdv_reset_encoder")),
    "encode_packed": Stage(_encode_packed, ["v210_137x6", "v210_720x48"], "uyvy422_720x48", _entry("sdv_reset_encoder")),
    "ingest_frames": Stage(_ingest, ["v210_137x6", "v210_720x48"], "gray8_past", allocates=False),       # (one kernel from the caller's buffer to the caller's buffer)
}
POISONED_STAGES = [name for name, stage in STAGES.items() if stage.allocates]


# ---- the three properties ---------------------------------------------------------------------------------------------------------------------------
def run_fresh(lib, c, name):
    """(a): every case of a stage on an engine of its own - with the allocations poisoned every buffer the case touches is a new, prefilled one."""
    stage = STAGES[name]
    for case in stage.cases:
        eng = lib.sdv_engine_create(0)
        assert eng, lib.sdv_last_error(None)
        try:
            stage.run(lib, eng, c, case)
        except AssertionError as ex:
            raise AssertionError("%s, case %s: %s" % (name, case, ex)) from ex
        finally:
            lib.sdv_engine_destroy(eng)


def run_with_a_past(lib, c, name):
    """(b): one engine; the past, the start-over entry, then every compact case in table order and in reverse, with start-over between them."""
    stage = STAGES[name]
    eng = lib.sdv_engine_create(0)
    assert eng, lib.sdv_last_error(None)
    try:
        if stage.past is not None:
            stage.run(lib, eng, c, stage.past, check=False)
        for k, case in enumerate(stage.cases + stage.cases[::-1]):
            if stage.start_over is not None:
                stage.start_over(lib, eng, c)
            try:
                stage.run(lib, eng, c, case)
            except AssertionError as ex:
                raise AssertionError("%s, case %s (turn %d behind the past %s): %s" % (name, case, k, stage.past, ex)) from ex
    finally:
        lib.sdv_engine_destroy(eng)


def run_formats_on_one_engine(lib, c):
    """An STC-007 tape through sdv_decode_frames, then a PCM-16x0 tape, then the STC-007 tape again, on one engine: the chain states and the prescan buffers
    are shared between the formats.  The two STC-007 outputs are byte-equal to each other and (inside _decode) to the oracle."""
    eng = lib.sdv_engine_create(0)
    assert eng, lib.sdv_last_error(None)
    try:
        got = []
        for case in ("stc007", "pcm16x0", "stc007"):
            _decode_reset(lib, eng, c)
            try:
                got.append(_decode(lib, eng, c, case))
            except AssertionError as ex:
                raise AssertionError("decode_frames, %s behind %d other tapes: %s" % (case, len(got), ex)) from ex
        assert got[0] == got[2]
    finally:
        lib.sdv_engine_destroy(eng)


# ---- (a) on the GPU: the developer build in a process of its own ----------------------------------------------------------------------------------------
_CHILD = r"""
import ctypes as C, json, os, sys
sys.path[:0] = [sys.argv[1], os.path.join(sys.argv[1], "tests")]
import numpy as np
import device_calls as dc
import memory_history as mh
lib, byte = dc.product_lib(), int(os.environ["SDV_POISON_ALLOC"], 0)
assert lib._name == os.environ["SDVPCM_LIB"], lib._name
def poisoned():
    n, b = C.c_uint64(0), C.c_uint64(0)
    assert lib.sdv_dev_poisoned(C.byref(n), C.byref(b)) == byte
    return n.value, b.value
for pinned in (0, 1):
    fresh = np.zeros(4099, dtype=np.uint8)
    assert lib.sdv_dev_peek_fresh(pinned, fresh.size, fresh.ctypes.data) == 0
    print("PEEK " + json.dumps({"pinned": pinned, "bytes": fresh.size, "all": bool((fresh == byte).all()), "first": int(fresh[0])}), flush=True)
    assert (fresh == byte).all(), "the fill did not land in %s memory" % ("pinned" if pinned else "device")
for name in sys.argv[2:]:
    n0, b0 = poisoned()
    try:
        mh.run_fresh(lib, dc.DEVICE, name)
    except AssertionError as ex:
        print("MISMATCH " + str(ex), flush=True)
        sys.exit(3)
    n1, b1 = poisoned()
    print("POISONED " + json.dumps({"stage": name, "allocations": n1 - n0, "bytes": b1 - b0}), flush=True)
print("HISTORY_OK")
"""


def gpu_child(byte, names, timeout):
    """The stages `names` in table order under SDV_POISON_ALLOC=byte through the developer build -> (exit status, {stage: (allocations, bytes)}, peeks, output)"""
    dev = os.path.join(ROOT, "sdvpcmdecoder_amd", "libsdvpcm_hip_dev.so")
    assert os.path.exists(dev), "no developer build of the HIP library (sdvpcmdecoder_amd/build.py: build_hip_dev, run by build())"
    env = dict(os.environ); env["SDVPCM_LIB"] = dev; env["SDV_POISON_ALLOC"] = "0x%02X" % byte
    t0 = time.time()
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT] + list(names), env=env, capture_output=True, text=True, timeout=timeout)
    filled, peeks = {}, []
    for line in r.stdout.splitlines():
        if line.startswith("POISONED "):
            rec = json.loads(line[9:])
            filled[rec["stage"]] = (rec["allocations"], rec["bytes"])
        elif line.startswith("PEEK "):
            peeks.append(json.loads(line[5:]))
        if line.startswith(("POISONED ", "PEEK ", "MISMATCH ")):
            print(line)
    print("child with 0x%02X: exit status %d after %.1f s" % (byte, r.returncode, time.time() - t0))
    return r.returncode, filled, peeks, r.stdout[-3000:] + r.stderr[-4000:]
