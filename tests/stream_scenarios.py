"""The scenario table of tests/test_stream_contract.py: every streamed entry point of include/sdvpcm.h as one small, ordinary call (or chain
of calls) with two tapes - A, which is decoded, and B, which only ever lies in the input buffers before A is copied there - and the oracle's
result for both.  A scenario is written once against a small context (`ctx.ptr`, `ctx.out`, `ctx.engine`, `ctx.s`) that the GPU tests fill with
torch tensors and a side stream and the CPU twins with numpy arrays and the emulator build, which ignores the stream argument.

    make(tape, orc) -> (inputs, want)   inputs: name -> numpy array that goes into device memory; want: the oracle's outputs (numpy arrays)
    run(ctx, dev, inp) -> outputs       dev: name -> device buffer holding inputs[name]; inp: tape A's numpy inputs (shapes, host-side arrays);
                                        outputs: (device buffer, bytes) per entry of `want` - or a numpy array for what the call hands back on the host
    kinds                               what every output holds (KINDS), for the "A and B differ record for record" precondition
    complete                            the last call is documented "returns when the outputs are complete" (sdvpcm.h)
"""
import ctypes as C
import functools

import numpy as np

import audio_api as au
import deint_api as da
import engine_api as ea
import libs
import oracle_run
import pcm1_api as p1
import pcm1_frames_api as p1f
import pcm1_front_api as p1l
import pcm16_api as p16
import pcm16_frames_api as p16f
import pcm16_front_api as p16l
import render_api as ra
import stitch_api as sa
from sdvpcmdecoder_amd import abi, synth

VP, I, U16, U32 = C.c_void_p, C.c_int, C.c_uint16, C.c_uint32
PCM1, PCM16X0, STC007 = abi.PCM_PCM1, abi.PCM_PCM16X0, abi.PCM_STC007


def bind(lib):
    """The C-ABI of the product library or of its emulator build through a handle of its own."""
    return abi.bind(C.CDLL(lib._name))


def ok(ctx, h, rc):
    assert rc == 0, (rc, ctx.lib.sdv_last_error(h))


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


# What an output holds.  Records that carry something of the tape must differ between tape A and tape B, every one of them: the tapes have other
# samples, other data coordinates and other frame numbers.  "pairs" / "pcm": sample pairs that are no file tag and are not silent on both tapes (the
# stitchers put out silence for what they could not decode, on any tape); the record types with a service_type: the records that are no service
# line / file tag; "purges" (positions of the file tags) and "masked_count" (a count handed back on the host) say nothing of the tape's content.
PCM_DTYPE = np.dtype([("audio_word", "<i2", (2,))])
KINDS = {"line": libs.LINE_DTYPE, "bin1": p1l.BIN1_DTYPE, "bin16": p16l.BIN16_DTYPE, "pairs": sa.PAIR_DTYPE, "pcm": PCM_DTYPE, "frasm": sa.FRASM_DTYPE,
         "frasm1": p1.FRASM1_DTYPE, "frasm16": p16.FRASM16_DTYPE, "stats": ea.STATS_DTYPE, "block": da.BLOCK_DTYPE, "canvas": None,
         "purges": au.PURGE_DTYPE, "masked_count": np.dtype("<u8")}
POSITIONAL = ("purges", "masked_count")


def tape_records(kind, a, b):
    """-> (records of both outputs that carry something of the tape, how many of them differ, records compared)."""
    if kind == "canvas":
        n = min(len(a), len(b))
        ra_, rb_ = as_bytes(a).reshape(len(a), -1)[:n], as_bytes(b).reshape(len(b), -1)[:n]
        return n, int((ra_ != rb_).any(axis=1).sum()), n
    dt = KINDS[kind]
    a, b = np.frombuffer(as_bytes(a).tobytes(), dtype=dt), np.frombuffer(as_bytes(b).tobytes(), dtype=dt)
    n = min(len(a), len(b))
    a, b = a[:n], b[:n]
    carries = np.ones(n, dtype=bool)
    if "service_type" in dt.names:
        carries &= (a["service_type"] == 0) & (b["service_type"] == 0)
    if kind in ("pairs", "pcm"):
        carries &= (a["audio_word"] != 0).any(axis=1) | (b["audio_word"] != 0).any(axis=1)
    differ = (a.view(np.uint8).reshape(n, dt.itemsize) != b.view(np.uint8).reshape(n, dt.itemsize)).any(axis=1)
    return int(carries.sum()), int((carries & differ).sum()), n


class Scenario:
    def __init__(self, name, make, run, kinds, complete):
        assert all(k in KINDS for k in kinds)
        self.name, self._make, self.run, self.kinds, self.complete = name, make, run, kinds, complete

    @functools.lru_cache(maxsize=None)
    def made(self, tape):
        inputs, want = self._make(tape, libs.load_oracle())
        return {k: np.ascontiguousarray(v) for k, v in inputs.items()}, [np.ascontiguousarray(w) for w in want]

    def __repr__(self):
        return self.name


SCENARIOS = []


def scenario(name, kinds, complete):
    def deco(cls):
        SCENARIOS.append(Scenario(name, cls.make, cls.run, kinds, complete))
        return cls
    return deco


def tape_kw(tape, seed, **kw):
    """Tape B: another seed and other data coordinates (the window of the data cells starts and ends elsewhere)."""
    if tape == "B":
        kw = dict(kw, seed=seed + 1000, x0=kw.get("x0", 12) + 7, x1=kw.get("x1", 708) - 9)
    else:
        kw = dict(kw, seed=seed)
    return kw


def first_no(tape):
    return 1 if tape == "A" else 301


# ---- the frame entries ------------------------------------------------------------------------------------------------------------
def call_frames(ctx, h, fn, luma_buf, shape, first_frame_no, flags, rec_bytes, n_recs, n_stats):
    n, hgt, w = shape
    recs, stats = ctx.out(n_recs * rec_bytes), ctx.out(n_stats * 32)
    ok(ctx, h, getattr(ctx.lib, fn)(h, ctx.ptr(luma_buf), w, w * hgt, w, hgt, n, first_frame_no, flags, ctx.ptr(recs), n_recs, ctx.ptr(stats), n_stats, ctx.s))
    return [(recs, n_recs * rec_bytes), (stats, n_stats * 32)]


def stc_frames(mode, seed, lost):
    class S:
        @staticmethod
        def make(tape, orc):
            luma = synth.stc007_frames(6, height=60, noise_sigma=7.0, blur=1, **tape_kw(tape, seed))[0].copy()
            if lost:
                luma[:, lost::11] = 16              # lost lines: the lines behind them do not read from what was handed on (INSANE: a sweep each)
            recs, stats = oracle_run.oracle_binarize(luma, mode=mode, first_frame_no=first_no(tape), new_file=True)
            return {"luma": luma}, [recs, stats]

        @staticmethod
        def run(ctx, dev, inp):
            h = ctx.engine()
            ok(ctx, h, ctx.lib.sdv_set_mode(h, mode))
            n, hgt, w = inp["luma"].shape
            return call_frames(ctx, h, "sdv_binarize_frames", dev["luma"], inp["luma"].shape, 1, 1, 48, n * (hgt + 3) + 1, n)
    return S


scenario("binarize_frames_normal", ("line", "stats"), True)(stc_frames(2, 21, 0))
scenario("binarize_frames_insane", ("line", "stats"), True)(stc_frames(3, 22, 5))


def markerless_frames(api, fn, rec_bytes, per_row, gen, mode, seed, **kw):
    """16 frames of 32 / 24 lines that need repair rounds (the tapes of test_emu_stream_in_two_calls)."""
    class S:
        @staticmethod
        def make(tape, orc):
            k = dict(kw, seed=seed if tape == "A" else seed + 1000)
            if tape == "B":
                k.update(x0=11, x1=701)
            luma, _ = gen(16, **k)
            recs, stats = api.run_cpu(orc, "orc_", luma, mode, {}, first_frame_no=first_no(tape))
            return {"luma": luma}, [recs, stats]

        @staticmethod
        def run(ctx, dev, inp):
            h = ctx.engine()
            ok(ctx, h, ctx.lib.sdv_set_mode(h, mode))
            n, hgt, w = inp["luma"].shape
            return call_frames(ctx, h, fn, dev["luma"], inp["luma"].shape, 1, 0, rec_bytes, n * (per_row * hgt + 3), n)
    return S


scenario("pcm1_binarize_frames_jitter", ("bin1", "stats"), True)(
    markerless_frames(p1f, "sdv_pcm1_binarize_frames", 40, 1, lambda n, **k: synth.pcm1_frames(n, height=32, **k), 2, 503, jitter=3, noise_sigma=4.0))
scenario("pcm1_binarize_frames_draft_dropouts", ("bin1", "stats"), True)(
    markerless_frames(p1f, "sdv_pcm1_binarize_frames", 40, 1, lambda n, **k: synth.pcm1_frames(n, height=32, **k), 0, 502, p_dropout=0.1, noise_sigma=5.0))
scenario("pcm16x0_binarize_frames_jitter", ("bin16", "stats"), True)(
    markerless_frames(p16f, "sdv_pcm16x0_binarize_frames", 36, 3, lambda n, **k: synth.pcm16x0_frames(n, height=24, **k), 2, 503, jitter=1, noise_sigma=4.0))
scenario("pcm16x0_binarize_frames_draft_dropouts", ("bin16", "stats"), True)(
    markerless_frames(p16f, "sdv_pcm16x0_binarize_frames", 36, 3, lambda n, **k: synth.pcm16x0_frames(n, height=24, **k), 0, 502, p_dropout=0.1, noise_sigma=5.0))


# ---- the line entries -----------------------------------------------------------------------------------------------------------------
@scenario("binarize_lines", ("line",), True)
class _StcLines:
    @staticmethod
    def make(tape, orc):
        rows = np.ascontiguousarray(synth.stc007_frames(1, height=64, noise_sigma=6.0, blur=1, **tape_kw(tape, 11))[0][0])
        orc.orc_bin_new.restype = VP
        orc.orc_bin_set_mode.argtypes = [VP, I]
        orc.orc_bin_free.argtypes = [VP]
        orc.orc_bin_process.argtypes = [VP, VP, I, U32, U16, I, I, I, VP]
        want = np.zeros(len(rows), dtype=libs.LINE_DTYPE)
        for i in range(len(rows)):          # a fresh Binarizer per line: nothing preset
            hb = VP(orc.orc_bin_new())
            orc.orc_bin_set_mode(hb, 2)
            orc.orc_bin_process(hb, rows[i].ctypes.data, rows.shape[1], first_no(tape), 1 + i, 0, 0, 0, want[i:i + 1].ctypes.data)
            orc.orc_bin_free(hb)
        return {"luma": rows}, [want]

    @staticmethod
    def run(ctx, dev, inp):
        h = ctx.engine()
        ok(ctx, h, ctx.lib.sdv_set_mode(h, 2))
        n, w = inp["luma"].shape
        out = ctx.out(n * 48)
        ok(ctx, h, ctx.lib.sdv_binarize_lines(h, ctx.ptr(dev["luma"]), w, w, n, None, 1, 1, 1, 0, ctx.ptr(out), n, ctx.s))
        return [(out, n * 48)]


def cold_states(n, dtype):
    st = np.zeros(n, dtype=dtype)
    st["start"], st["stop"] = -32768, 32767
    return st


@scenario("pcm1_binarize_lines", ("bin1",), False)
class _Pcm1Lines:
    @staticmethod
    def make(tape, orc):
        luma, _ = synth.pcm1_random_lines(24, seed=3 if tape == "A" else 1003, x0=-9 if tape == "A" else 2, x1=726 if tape == "A" else 715, noise_sigma=3.0)
        cold = cold_states(len(luma), p1l.STATE_DTYPE)
        first = p1l.run_lines_with_states(orc, "orc_bin1_", luma, cold, mode=2, frame=first_no(tape))
        states = p1l.states_from_records(first)      # the lean kernel for lines that read from their presets, the list of the others for the full one
        want = p1l.run_lines_with_states(orc, "orc_bin1_", luma, states, mode=2, frame=first_no(tape))
        return {"luma": luma, "states": states}, [want]

    @staticmethod
    def run(ctx, dev, inp):
        h = ctx.engine()
        ok(ctx, h, ctx.lib.sdv_set_mode(h, 2))
        n, w = inp["luma"].shape
        out = ctx.out(n * 40)
        ok(ctx, h, ctx.lib.sdv_pcm1_binarize_lines(h, ctx.ptr(dev["luma"]), w, w, n, ctx.ptr(dev["states"]), 1, 1, 1, 0, 1, ctx.ptr(out), n, ctx.s))
        return [(out, n * 40)]


@scenario("pcm16x0_binarize_lines", ("bin16",), False)
class _Pcm16Lines:
    @staticmethod
    def make(tape, orc):
        luma, _ = synth.pcm16x0_random_lines(24, seed=5 if tape == "A" else 1005, x0=4 if tape == "A" else 9, x1=716 if tape == "A" else 706, noise_sigma=3.0)
        want = p16l.run_lines_with_states(orc, "orc_bin16_", luma, cold_states(3 * len(luma), p16l.STATE_DTYPE), mode=2, frame=first_no(tape))[0]
        return {"luma": luma}, [want]

    @staticmethod
    def run(ctx, dev, inp):
        h = ctx.engine()
        ok(ctx, h, ctx.lib.sdv_set_mode(h, 2))
        n, w = inp["luma"].shape
        out = ctx.out(3 * n * 36)
        ok(ctx, h, ctx.lib.sdv_pcm16x0_binarize_lines(h, ctx.ptr(dev["luma"]), w, w, n, None, 1, 1, 1, 0, 1, ctx.ptr(out), 3 * n, None, ctx.s))
        return [(out, 3 * n * 36)]


# ---- deinterleave -----------------------------------------------------------------------------------------------------------------------
@scenario("deinterleave_blocks", ("block",), False)
class _Deint:
    N_BLOCKS = 700          # more than two blocks of 256 threads, no multiple of them

    @staticmethod
    def make(tape, orc):
        seed = 31 if tape == "A" else 1031
        rng = np.random.default_rng(seed)
        audio = rng.integers(0, 1 << 14, size=(_Deint.N_BLOCKS + 200, 6), dtype=np.uint32)
        lines = da.make_lines(synth.interleave_stream(audio), frame0=first_no(tape), rng=rng, p_bad=0.08, p_corrupt_valid=0.002, p_cwd=0.01)
        rc, want = da.run_cpu(orc, "orc_", lines, da.settings(), _Deint.N_BLOCKS)
        assert rc == 3          # the oracle's DI_RET_OK
        return {"lines": lines}, [want]

    @staticmethod
    def run(ctx, dev, inp):
        h = ctx.engine()
        st = da.settings()
        out = ctx.out(_Deint.N_BLOCKS * 72)
        ok(ctx, h, ctx.lib.sdv_deinterleave_blocks(h, ctx.ptr(dev["lines"]), len(inp["lines"]), C.byref(st), ctx.ptr(out), _Deint.N_BLOCKS, ctx.s))
        return [(out, _Deint.N_BLOCKS * 72)]


# ---- the stitch entries -----------------------------------------------------------------------------------------------------------------
def call_stitch(ctx, h, fn, recs_buf, n_recs, frasm_bytes, n_frames_est):
    pair_cap, frame_cap = n_frames_est * 2400 + 8192, n_frames_est * 3 + 16
    pairs, frames = ctx.out(pair_cap * 12), ctx.out(frame_cap * frasm_bytes)
    npairs, nframes = C.c_size_t(0), C.c_size_t(0)
    ok(ctx, h, getattr(ctx.lib, fn)(h, ctx.ptr(recs_buf), n_recs, ctx.ptr(pairs), pair_cap, C.byref(npairs), ctx.ptr(frames), frame_cap, C.byref(nframes), ctx.s))
    return [(pairs, npairs.value * 12), (frames, nframes.value * frasm_bytes)]


def stc_tape(tape, n, seed):
    luma = synth.stc007_frames(n, noise_sigma=4.0, **tape_kw(tape, seed))[0].copy()
    luma[:, 77::61] = 16        # lost lines: the error correction has something to do
    return luma


@scenario("stitch_frames", ("pairs", "frasm"), True)
class _StcStitch:
    @staticmethod
    def make(tape, orc):
        recs, _ = oracle_run.oracle_binarize(stc_tape(tape, 4, 12), mode=2, first_frame_no=first_no(tape), new_file=True, end_file=True)
        pairs, frames = sa.run_cpu(orc, "orc_", recs, sa.default_settings())
        return {"recs": recs}, [pairs, frames]

    @staticmethod
    def run(ctx, dev, inp):
        h = ctx.engine()
        st = sa.default_settings()
        ok(ctx, h, ctx.lib.sdv_set_stitch_settings(h, C.byref(st)))
        return call_stitch(ctx, h, "sdv_stitch_frames", dev["recs"], len(inp["recs"]), 64, 6)


def bin_to_line_recs(bin_recs):
    """sdv_pcm1_bin_rec -> sdv_pcm1_line_rec in numpy: what sdv_pcm1_bin_to_line_recs does on the device."""
    out = np.zeros(len(bin_recs), dtype=p1.LINE1_DTYPE)
    for nm in ("frame_number", "line_number", "words", "calc_crc", "ref_level", "picked_bits_left", "picked_bits_right", "service_type"):
        out[nm] = bin_recs[nm]
    out["flags"] = bin_recs["flags"] & (p1.LF_BW_SET | p1.LF_FORCED_BAD)
    return out


def pcm_tape(fmt, tape, n, ei=False):
    if fmt == PCM1:
        k = dict(seed=43, noise_sigma=3.0) if tape == "A" else dict(seed=1043, noise_sigma=3.0, x0=10, x1=700)
        return synth.pcm1_frames(n, height=486, **k)[0]
    k = dict(seed=44) if tape == "A" else dict(seed=1044, x0=10, x1=700)
    return synth.pcm16x0_tape_frames(n, ei=ei, **k)[0]


@scenario("pcm1_bin_to_line_recs+pcm1_stitch_frames", ("pairs", "frasm1"), True)
class _Pcm1Stitch:
    @staticmethod
    def make(tape, orc):
        recs, _ = p1f.run_cpu(orc, "orc_", pcm_tape(PCM1, tape, 3), 2, dict(new_file=True, end_file=True), first_frame_no=first_no(tape))
        pairs, frames = p1.run_cpu(orc, "orc_", bin_to_line_recs(recs), p1.default_settings())
        return {"recs": recs}, [pairs, frames]

    @staticmethod
    def run(ctx, dev, inp):
        h = ctx.engine()
        n = len(inp["recs"])
        lines = ctx.out(n * 32)
        ok(ctx, h, ctx.lib.sdv_pcm1_bin_to_line_recs(h, ctx.ptr(dev["recs"]), n, ctx.ptr(lines), ctx.s))
        return call_stitch(ctx, h, "sdv_pcm1_stitch_frames", lines, n, 52, 5)


def pcm16_stitch(case):
    n, kw, st_kw = p16.CASES[case][:3]

    class S:
        @staticmethod
        def make(tape, orc):
            k = dict(kw) if tape == "A" else dict(kw, seed=kw["seed"] + 1000, first_frame=301)
            recs, _ = p16.make_stream(n, **k)
            pairs, frames = p16.run_cpu(orc, "orc_", recs, p16.default_settings(**st_kw))
            return {"recs": recs}, [pairs, frames]

        @staticmethod
        def run(ctx, dev, inp):
            h = ctx.engine()
            st = p16.default_settings(**st_kw)
            ok(ctx, h, ctx.lib.sdv_set_pcm16x0_stitch_settings(h, C.byref(st)))
            return call_stitch(ctx, h, "sdv_pcm16x0_stitch_frames", dev["recs"], len(inp["recs"]), 56, n + 2)
    return S


# (the analysis batches of the PCM-16x0 stitcher are 1024 frames: no small tape takes more than one, these take its three private streams once)
scenario("pcm16x0_stitch_frames_si", ("pairs", "frasm16"), True)(pcm16_stitch("si_bad10"))
scenario("pcm16x0_stitch_frames_ei", ("pairs", "frasm16"), True)(pcm16_stitch("ei_cut"))


# ---- the fused entry ----------------------------------------------------------------------------------------------------------------------
FRASM_BYTES = {STC007: 64, PCM1: 52, PCM16X0: 56}
FRASM_KIND = {STC007: "frasm", PCM1: "frasm1", PCM16X0: "frasm16"}


def oracle_chain(orc, fmt, luma, first_frame_no):
    """The separate stages of the oracle, one after the other: (pairs, frame descriptors, frame stats)."""
    if fmt == STC007:
        recs, stats = oracle_run.oracle_binarize(luma, mode=2, first_frame_no=first_frame_no, new_file=True, end_file=True)
        pairs, frames = sa.run_cpu(orc, "orc_", recs, sa.default_settings())
    elif fmt == PCM1:
        recs, stats = p1f.run_cpu(orc, "orc_", luma, 2, dict(new_file=True, end_file=True), first_frame_no=first_frame_no)
        pairs, frames = p1.run_cpu(orc, "orc_", bin_to_line_recs(recs), p1.default_settings())
    else:
        recs, stats = p16f.run_cpu(orc, "orc_", luma, 2, dict(new_file=True, end_file=True), first_frame_no=first_frame_no)
        pairs, frames = p16.run_cpu(orc, "orc_", recs, p16.default_settings())
    return pairs, frames, stats


def call_decode(ctx, h, fmt, luma_buf, shape, first_frame_no, flags, with_audio, stop=1, ofs=0):
    n, hgt, w = shape
    cap = (n + 2) * 1800 + 8192
    pairs, frames, stats, pur = ctx.out(cap * 12), ctx.out((n + 16) * FRASM_BYTES[fmt]), ctx.out((n + 1) * 32), ctx.out(8 * 16)
    npairs, nfr, npur, nm = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_uint64(0)
    ok(ctx, h, ctx.lib.sdv_decode_frames(h, fmt, ctx.ptr(luma_buf) + ofs, w, w * hgt, w, hgt, n, first_frame_no, flags, ctx.ptr(pairs), cap, C.byref(npairs),
                                         ctx.ptr(frames), n + 16, C.byref(nfr), ctx.ptr(stats), n + 1, 1 if with_audio else 0, stop, ctx.ptr(pur), 8, C.byref(npur), C.byref(nm), ctx.s))
    n_stats = n + (1 if flags & 4 else 0)
    outs = [(pairs, npairs.value * 12), (frames, nfr.value * FRASM_BYTES[fmt]), (stats, n_stats * 32)]
    if with_audio:
        outs += [(pur, npur.value * 16), np.array([nm.value], dtype=np.uint64)]
    return outs


def decode_frames(fmt, with_audio):
    class S:
        @staticmethod
        def make(tape, orc):
            luma = stc_tape(tape, 3, 12) if fmt == STC007 else pcm_tape(fmt, tape, 3)
            pairs, frames, stats = oracle_chain(orc, fmt, luma, first_no(tape))
            want = [pairs, frames, stats]
            if with_audio:
                out, _, pur, masked, hit = au.run_cpu(orc, "orc_", pairs, au.DROP_INTER_LIN_WORD, np.array([len(pairs)], dtype=np.uint64), 1)
                assert hit == 0
                want = [out, frames, stats, pur, np.array([masked], dtype=np.uint64)]
            return {"luma": luma}, want

        @staticmethod
        def run(ctx, dev, inp):
            h = ctx.engine()
            ok(ctx, h, ctx.lib.sdv_set_pcm_type(h, fmt, 0))
            if with_audio:
                ok(ctx, h, ctx.lib.sdv_set_audio_masking(h, au.DROP_INTER_LIN_WORD))
            return call_decode(ctx, h, fmt, dev["luma"], inp["luma"].shape, 1, 1 | 4, with_audio)
    return S


for _fmt, _nm in ((STC007, "stc007"), (PCM1, "pcm1"), (PCM16X0, "pcm16x0")):
    scenario("decode_frames_%s" % _nm, ("pairs", FRASM_KIND[_fmt], "stats"), True)(decode_frames(_fmt, False))
    scenario("decode_frames_%s_audio" % _nm, ("pairs", FRASM_KIND[_fmt], "stats", "purges", "masked_count"), True)(decode_frames(_fmt, True))


def stitch_info(ctx, h):
    info = ea.StitchInfo()
    ok(ctx, h, ctx.lib.sdv_get_stitch_info(h, C.byref(info)))
    return info


@scenario("decode_frames_stc007_stream_in_calls", ("pairs", "frasm", "stats"), True)
class _FusedStream:
    """One stream through the fused entry three frames per call (NEW_FILE with the first call, END_FILE with the last), frames that play and then
    frames with lost lines: from the third call on the frame kernel writes whole frames into the stitch stage's field buffers and the stitch
    kernels are queued behind its first round, ahead of the host's look at it (pipelined & 4); the call that meets the damage had them queued
    too, needs more rounds and runs the stitch stage again (& 8).  The scenario proves from sdv_get_stitch_info that it got there."""
    N, STEP, BAD_FROM = 15, 3, 9

    @staticmethod
    def make(tape, orc):
        luma = synth.stc007_frames(_FusedStream.N, noise_sigma=4.0, **tape_kw(tape, 12))[0].copy()
        luma[_FusedStream.BAD_FROM:, 77::61] = 16
        pairs, frames, stats = oracle_chain(orc, STC007, luma, first_no(tape))
        return {"luma": luma}, [pairs, frames, stats]

    @staticmethod
    def run(ctx, dev, inp):
        h = ctx.engine()
        ok(ctx, h, ctx.lib.sdv_set_pcm_type(h, STC007, 0))
        n, hgt, w = inp["luma"].shape
        parts, piped, direct = [[], [], []], [], 0
        for k in range(0, n, _FusedStream.STEP):
            flags = (1 if k == 0 else 0) | (4 if k + _FusedStream.STEP == n else 0)
            outs = call_decode(ctx, h, STC007, dev["luma"], (_FusedStream.STEP, hgt, w), 1 + k, flags, False, ofs=k * hgt * w)
            for i in range(3):
                parts[i].append((outs[i][0], 0, outs[i][1]))
            info = stitch_info(ctx, h)         # (direct_frames: one small read-back on stream 0, between two calls on the side stream)
            piped.append(int(info.pipelined))
            direct += int(info.direct_frames)
        assert any(x & 4 for x in piped) and any(x & 8 for x in piped) and direct > 0, (piped, direct)
        return [(ctx.cat(p), sum(hi for _, _, hi in p)) for p in parts]


# ---- the doubler in front of the frame entry ---------------------------------------------------------------------------------------------
@scenario("double_width+binarize_frames_doubled", ("line", "stats"), True)
class _Doubled:
    @staticmethod
    def make(tape, orc):
        k = dict(seed=61, x0=6, x1=354) if tape == "A" else dict(seed=1061, x0=10, x1=349)
        luma = synth.stc007_frames(4, height=60, width=360, noise_sigma=4.0, **k)[0]
        recs, stats = oracle_run.oracle_binarize(np.repeat(luma, 2, axis=2), mode=2, first_frame_no=first_no(tape), new_file=True, doubled=True)
        return {"luma": luma}, [recs, stats]

    @staticmethod
    def run(ctx, dev, inp):
        h = ctx.engine()
        ok(ctx, h, ctx.lib.sdv_set_mode(h, 2))
        n, hgt, w = inp["luma"].shape
        wide = ctx.out(n * hgt * 2 * w)
        ok(ctx, h, ctx.lib.sdv_double_width(h, ctx.ptr(dev["luma"]), w, w, n * hgt, ctx.ptr(wide), 2 * w, ctx.s))
        return call_frames(ctx, h, "sdv_binarize_frames", wide, (n, hgt, 2 * w), 1, 1 | 2, 48, n * (hgt + 3) + 1, n)


# ---- the audio chain ---------------------------------------------------------------------------------------------------------------------
@scenario("audio_process+audio_deemphasis+wav_pack", ("pairs", "purges", "masked_count", "pairs", "pcm"), False)
class _Audio:
    @staticmethod
    def make(tape, orc):
        import test_deemphasis as td
        seed = 71 if tape == "A" else 1071
        pairs = au.tape(["N", au.audio(3000, seed, runs=((400, 30, 2), (1500, 300, 0)), p_bad=0.01, emphasis=1), "E"])
        out, _, pur, masked, hit = au.run_cpu(orc, "orc_", pairs, au.DROP_INTER_LIN_WORD, np.array([len(pairs)], dtype=np.uint64), 1)
        assert hit == 0
        flat, _ = td.walk(out, td.FORCE)
        return {"pairs": pairs}, [out, pur, np.array([masked], dtype=np.uint64), flat, np.ascontiguousarray(flat["audio_word"]).astype("<i2")]

    @staticmethod
    def run(ctx, dev, inp):
        h = ctx.engine()
        n = len(inp["pairs"])
        ok(ctx, h, ctx.lib.sdv_set_audio_masking(h, au.DROP_INTER_LIN_WORD))
        ok(ctx, h, ctx.lib.sdv_set_deemphasis(h, 2))
        cap = n + 1024
        out, pur, flat, pcm = ctx.out(cap * 12), ctx.out(8 * 16), ctx.out(cap * 12), ctx.out(cap * 4)
        n_out, n_pur, nm = C.c_size_t(0), C.c_size_t(0), C.c_uint64(0)
        ok(ctx, h, ctx.lib.sdv_audio_process(h, ctx.ptr(dev["pairs"]), n, 1, ctx.ptr(out), cap, C.byref(n_out), ctx.ptr(pur), 8, C.byref(n_pur), C.byref(nm), ctx.s))
        ok(ctx, h, ctx.lib.sdv_audio_deemphasis(h, ctx.ptr(out), n_out.value, ctx.ptr(flat), ctx.s))
        ok(ctx, h, ctx.lib.sdv_wav_pack(h, ctx.ptr(flat), n_out.value, ctx.ptr(pcm), ctx.s))
        return [(out, n_out.value * 12), (pur, n_pur.value * 16), np.array([nm.value], dtype=np.uint64), (flat, n_out.value * 12), (pcm, n_out.value * 4)]


# ---- the visualiser ----------------------------------------------------------------------------------------------------------------------
def canvas_bytes(kind):
    w, h = ra.SIZE[kind]
    return w * h * 4


@scenario("vis_render_lines", ("canvas",), False)
class _VisLines:
    @staticmethod
    def make(tape, orc):
        recs = ra._stc_records(3, 60, 901 if tape == "A" else 1901, noise_sigma=6.0, p_dropout=0.05, **({} if tape == "A" else dict(x0=19, x1=699)))
        return {"recs": np.ascontiguousarray(recs)}, [ra.run_oracle(ra.STC007, np.ascontiguousarray(recs))[0]]

    @staticmethod
    def run(ctx, dev, inp):
        h = ctx.engine()
        n = ra.n_frames(inp["recs"])
        out = ctx.out(n * canvas_bytes(ra.STC007))
        got = C.c_size_t(0)
        ok(ctx, h, ctx.lib.sdv_vis_render_lines(h, ra.STC007, ctx.ptr(dev["recs"]), len(inp["recs"]), ctx.ptr(out), n, C.byref(got), ctx.s))
        assert got.value == n
        return [(out, n * canvas_bytes(ra.STC007))]


def stitch_feeds(tape, orc):
    """Blocks and assembled lines of a short damaged STC-007 tape, as the oracle's stitcher hands them to the visualiser."""
    luma = synth.stc007_frames(3, noise_sigma=2.0, **tape_kw(tape, 81))[0].copy()
    luma[:, 40::23] = 16
    recs, _ = oracle_run.oracle_binarize(luma, mode=2, first_frame_no=first_no(tape), new_file=True, end_file=True)
    pairs, frames, blocks = sa.run_cpu_blocks(orc, "orc_", recs, sa.default_settings())
    lines, per_turn = sa.last_asm_lines(orc, "orc_")
    per_frame = frames["blocks_total"][frames["service_type"] == 0].astype(np.uint32)
    return np.ascontiguousarray(blocks), np.ascontiguousarray(per_frame), np.ascontiguousarray(lines), np.ascontiguousarray(per_turn)


def vis_rows(fn, kind, which):
    class S:
        @staticmethod
        def make(tape, orc):
            blocks, per_frame, lines, per_turn = stitch_feeds(tape, orc)
            recs, per = (blocks, per_frame) if which == "blocks" else (lines, per_turn)
            want = (ra.run_oracle_blocks if which == "blocks" else ra.run_oracle_asm)(kind, recs, per)[0]
            return {"recs": recs, "_per": per}, [want]

        @staticmethod
        def run(ctx, dev, inp):
            h = ctx.engine()
            per = np.ascontiguousarray(inp["_per"], dtype=np.uint32)
            out = ctx.out(len(per) * canvas_bytes(kind))
            ok(ctx, h, getattr(ctx.lib, fn)(h, kind, ctx.ptr(dev["recs"]), len(inp["recs"]), per.ctypes.data, len(per), ctx.ptr(out), len(per), ctx.s))
            return [(out, len(per) * canvas_bytes(kind))]
    return S


scenario("vis_render_blocks", ("canvas",), False)(vis_rows("sdv_vis_render_blocks", ra.STC007_BLOCKS_NTSC, "blocks"))
scenario("vis_render_asm_lines", ("canvas",), False)(vis_rows("sdv_vis_render_asm_lines", ra.STC007_ASM_NTSC, "lines"))

BY_NAME = {s.name: s for s in SCENARIOS}
