"""sdv_pcm_preemphasis (include/sdvpcm.h): the 15/50 us pre-emphasis network on interleaved int16 PCM, on the SIMT emulator (CPU) and through
the C-ABI on the GPU (-m gpu), against `walk` below - a plain sequential float64 loop written from the definition in the header, never the code
under test.  The end of the file takes both conditioning stages to the encoders and back on the GPU.

Tolerance, derived: the device runs the same recurrence in double, a lane from the 32 pairs in front of its own.  Every output word then comes from
a y that differs from the sequential one by a few roundings of a double at magnitude up to 2^17 - about 1e-11 LSB - plus what a state owes to pairs
more than 32 back (0.139^32 = 3e-28 of full scale).  So a word can differ only where y sits within about 1e-9 of a half, and then by one: every
word within 1 LSB, at most 2 words per case (cases hold at most 200 000 samples - a cap, not a measurement) differing at all, and the clipped count
off the walk's by at most the number of differing words.  An accumulation in float32 differs in 14 of 20 000 samples of +-8000 noise and fails
(test_the_condition_tells_float_from_double)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pcm_condition_api as P
from pcm_condition_api import check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "sdvpcm.h")).read()
T = int(re.search(r"#define SDV_PREEMPH_TILE (\d+)", HDR).group(1))          # pairs per tile of the device's work
W = int(re.search(r"#define SDV_PREEMPH_WARMUP (\d+)", HDR).group(1))        # pairs in front of a lane's own its state comes from
T1, T2 = 50e-6, 15e-6


# ---- the definition ----------------------------------------------------------------------------------------------------------
def de_coeffs(rate):
    fs = 44056.0 if rate == 44056 else 44100.0
    k = 2.0 * fs
    return (1.0 + k * T2) / (1.0 + k * T1), (1.0 - k * T2) / (1.0 + k * T1), (1.0 - k * T1) / (1.0 + k * T1)


def coeffs(rate):
    b0, b1, a1 = de_coeffs(rate)
    return 1.0 / b0, a1 / b0, b1 / b0


def walk(pcm, rate, state=None, ftype=np.float64):
    """-> (out, state, clipped).  state: per channel None (idle) or (fs, x_prev, y_prev)."""
    out = pcm.copy()
    st = [None, None] if state is None else list(state)
    fs = 44056 if rate == 44056 else 44100
    c0, c1, c2 = (ftype(c) for c in coeffs(rate))
    clipped = 0
    for i in range(len(pcm)):
        for ch in range(2):
            x = ftype(pcm[i, ch])
            if st[ch] is None or st[ch][0] != fs:
                y = x
            else:
                y = c0 * x + c1 * st[ch][1] - c2 * st[ch][2]
                r = np.rint(y)
                clipped += int(r < -32768 or r > 32767)
                out[i, ch] = int(min(max(r, -32768), 32767))
            st[ch] = (fs, x, y)
    return out, st, clipped


# ---- signals -------------------------------------------------------------------------------------------------------------------
def signal(kind, n, seed=1, rate=44100):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    a = np.zeros((n, 2), dtype=np.int16)
    if kind == "noise":                                  # full scale, white: it clips
        a[:] = rng.integers(-32768, 32768, (n, 2))
    elif kind == "quiet":                                # sum |g| of the network is 3.657: nothing within +-8900 can clip
        a[:] = rng.integers(-8000, 8001, (n, 2))
    elif kind == "step":
        a[:, 0] = np.where(t >= n // 3, 30000, -20000)
        a[:, 1] = np.where(t >= 2, -32768, 32767)
    else:                                                # 10 kHz, amplitude 9000
        a[:, 0] = np.rint(9000 * np.sin(2 * np.pi * 10000.0 * t / rate))
        a[:, 1] = np.rint(9000 * np.cos(2 * np.pi * 10000.0 * t / rate))
    return a


KINDS = ["noise", "quiet", "step", "tone"]
LENGTHS = [1, 2, W - 1, W, W + 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 1]
_WANT = {}


def wanted(key, pcm, rate):
    """The walk over a case, computed once: (out, clipped)."""
    if key not in _WANT:
        out, _, clipped = walk(pcm, rate)
        _WANT[key] = (out, clipped)
    return _WANT[key][0].copy(), _WANT[key][1]


# ---- the code under test ---------------------------------------------------------------------------------------------------------
def clipped(be):
    n = C.c_uint64(12345)
    assert be.lib.sdv_pcm_preemphasis_clipped(be.h, be.stream(), C.byref(n)) == P.OK
    return int(n.value)


def run(be, pcm, rate, cuts=(), reset=True):
    """The stream through a back end, in calls that end at `cuts` (rate: one value, or one per call) -> the output"""
    n = len(pcm)
    src, dst = be.buffer(pcm), be.buffer(np.full((n, 2), 0x5A5A, dtype=np.int16))
    if reset:
        assert be.lib.sdv_reset_preemphasis(be.h) == P.OK
    ends = sorted(set(c for c in cuts if 0 < c < n)) + [n]
    a = 0
    for k, b in enumerate(ends):
        r = rate[k] if isinstance(rate, (list, tuple)) else rate
        assert be.lib.sdv_pcm_preemphasis(be.h, be.ptr(src, 4 * a), b - a, r, be.ptr(dst, 4 * a), be.stream()) == P.OK, be.lib.sdv_last_error(be.h)
        a = b
    return P.pcm_of(be.read(dst), n)


@pytest.fixture(scope="module")
def emu(emu_lib):
    be = P.Emu(emu_lib)
    yield be
    be.close()


@pytest.fixture(scope="module")
def gpu():
    be = P.Gpu()
    yield be
    be.close()


# ---- the checks, written once for both back ends ------------------------------------------------------------------------------
def _lengths(be, kind, n):
    pcm = signal(kind, 3 * T + 1, seed=3)[:n]
    want, want_clipped = wanted(("len", kind, n), pcm, 44100)
    got = run(be, pcm, 44100)
    differ = check(got, want)
    count = clipped(be)
    print("clipped %d, the walk %d" % (count, want_clipped))
    assert abs(count - want_clipped) <= differ
    if kind == "quiet":
        assert count == 0
    if kind == "noise" and n == 3 * T + 1:
        assert want_clipped > 1000                       # (the case does clip)
    assert np.array_equal(got[0], pcm[0])               # the filter starts: the first word stays


def _rates(be):
    pcm = signal("quiet", T + 300, seed=5)
    lo, hi = wanted("rate_lo", pcm, 44056)[0], wanted("rate_hi", pcm, 44100)[0]
    assert not np.array_equal(lo, hi)
    check(run(be, pcm, 44056), lo)
    for rate in (44100, 48000, 0, 32000):               # anything else reads 44100
        check(run(be, pcm, rate), hi)


def _split(be, cut):
    pcm = signal("noise", 2 * T + 300, seed=31)
    want, want_clipped = wanted("split", pcm, 44056)
    differ = check(run(be, pcm, 44056, cuts=(cut,)), want)
    assert abs(clipped(be) - want_clipped) <= differ


def _split_many(be):
    pcm = signal("tone", 3 * T + 99, seed=32)
    check(run(be, pcm, 44100, cuts=(1, 2, W, W + 1, T - 1, T, T + 100, 2 * T - 7, 2 * T - 6, 3 * T + 98)), wanted("many", pcm, 44100)[0])


def _rate_change_restarts(be):
    """A call at another rate finds the filter running at another fs: it starts again, the first word stays."""
    pcm = signal("quiet", T + 200, seed=33)
    cut = T - 37
    a, st, _ = walk(pcm[:cut], 44056)
    b, _, _ = walk(pcm[cut:], 44100, state=st)
    assert np.array_equal(b[0], pcm[cut]) and not np.array_equal(b[1], pcm[cut + 1])
    got = run(be, pcm, [44056, 44100], cuts=(cut,))
    check(got, np.concatenate([a, b]))
    assert np.array_equal(got[cut], pcm[cut])
    # ... and the same rate goes on from the state: the first word of the second call does not stay
    got = run(be, pcm, [44056, 44056], cuts=(cut,))
    check(got, wanted("rate_same", pcm, 44056)[0])
    assert not np.array_equal(got[cut], pcm[cut])


def _reset(be):
    """sdv_reset_preemphasis: the first word behind it stays, the counter is 0."""
    a, b = signal("noise", T + 50, seed=51), signal("quiet", 300, seed=52)
    run(be, a, 44100)
    assert clipped(be) > 0
    carried = run(be, b, 44100, reset=False)
    check(carried, wanted("reset_ab", np.concatenate([a[-200:], b]), 44100)[0][200:])
    assert not np.array_equal(carried[0], b[0]) and clipped(be) > 0      # (the counter goes on as well)
    got = run(be, b, 44100)                              # (run() resets)
    assert np.array_equal(got[0], b[0]) and clipped(be) == 0
    check(got, wanted("reset_b", b, 44100)[0])
    assert be.lib.sdv_reset_preemphasis(be.h) == P.OK and clipped(be) == 0


def _refusals(be):
    """An overlapping or misaligned call is refused and leaves state and counter alone: the stream in two calls with refused calls in between equals
    the walk over the whole stream."""
    pcm = signal("noise", T + 400, seed=41)
    n, cut = len(pcm), T - 100
    want, want_clipped = wanted("refuse", pcm, 44100)
    lib, h = be.lib, be.h
    buf = be.buffer(np.concatenate([pcm, np.zeros((n + 8, 2), dtype=np.int16)]))          # the input, the output behind it
    out = 4 * n
    assert lib.sdv_reset_preemphasis(h) == P.OK
    assert lib.sdv_pcm_preemphasis(h, be.ptr(buf), cut, 44100, be.ptr(buf, out), be.stream()) == P.OK
    count = clipped(be)
    before = be.read(buf)
    m = n - cut
    for dst in (4 * cut, 4 * (cut + 1), 4 * (cut - 1), 4 * (n - 1), 4 * (cut - m + 1)):              # in place too: any overlap
        assert lib.sdv_pcm_preemphasis(h, be.ptr(buf, 4 * cut), m, 44100, be.ptr(buf, dst), be.stream()) == P.BAD_ARG and b"overlap" in lib.sdv_last_error(h)
    for src_off, dst_off in ((2, 0), (0, 2), (1, 1), (2, 2)):
        assert lib.sdv_pcm_preemphasis(h, be.ptr(buf, 4 * cut + src_off), m - 1, 44100, be.ptr(buf, out + 4 * cut + dst_off), be.stream()) == P.BAD_ARG
        assert b"aligned" in lib.sdv_last_error(h)
    assert lib.sdv_pcm_preemphasis(h, None, 5, 44100, be.ptr(buf, out), be.stream()) == P.NULL_LINES
    assert lib.sdv_pcm_preemphasis(h, be.ptr(buf), 5, 44100, None, be.stream()) == P.NULL_BLOCK
    assert lib.sdv_pcm_preemphasis(h, None, 0, 44100, None, be.stream()) == P.OK           # n_pairs == 0: nothing done
    assert lib.sdv_pcm_preemphasis(h, be.ptr(buf), 0, 44056, be.ptr(buf), be.stream()) == P.OK
    assert be.read(buf).tobytes() == before.tobytes() and clipped(be) == count
    assert lib.sdv_pcm_preemphasis(h, be.ptr(buf, 4 * cut), m, 44100, be.ptr(buf, out + 4 * cut), be.stream()) == P.OK
    differ = check(P.pcm_of(be.read(buf), n, out), want)
    assert abs(clipped(be) - want_clipped) <= differ
    # buffers that are 4-byte but not 16-byte aligned give the same words
    odd = be.buffer(np.concatenate([np.zeros((1, 2), dtype=np.int16), pcm, np.zeros((n + 3, 2), dtype=np.int16)]))
    assert lib.sdv_reset_preemphasis(h) == P.OK
    assert lib.sdv_pcm_preemphasis(h, be.ptr(odd, 4), n, 44100, be.ptr(odd, 4 * (n + 3)), be.stream()) == P.OK
    assert np.array_equal(P.pcm_of(be.read(odd), n, 4 * (n + 3)), P.pcm_of(be.read(buf), n, out))


def _inverse(be, kind):
    """sdv_audio_deemphasis FORCE on the output gives the input back within 1 where nothing clipped: a rounding error <= 0.5 passes through a network
    whose sum |h| is 1.0, then a second rounding follows."""
    from stitch_api import PAIR_DTYPE
    pcm = signal(kind, 2 * T + 77, seed=61, rate=44056)
    got = run(be, pcm, 44056)
    assert clipped(be) == 0
    pairs = be.buffer(P.pairs_of(got, 44056))
    back = be.buffer(np.zeros(len(pcm), dtype=PAIR_DTYPE))
    assert be.lib.sdv_set_deemphasis(be.h, 2) == 0 and be.lib.sdv_reset_deemphasis(be.h) == 0
    assert be.lib.sdv_audio_deemphasis(be.h, be.ptr(pairs), len(pcm), be.ptr(back), be.stream()) == 0
    flat = be.read(back).view(PAIR_DTYPE)["audio_word"]
    assert be.lib.sdv_set_deemphasis(be.h, 0) == 0
    d = np.abs(flat.astype(np.int64) - pcm)
    print("de-emphasis of the pre-emphasis: %d of %d words differ from the input, largest difference %d" % (int((d != 0).sum()), d.size, int(d.max())))
    assert (d <= 1).all()


# ---- CPU: the coefficients of the product library, the definition itself, the emulator ---------------------------------------------
def test_coefficients_of_the_product_library():
    from sdvpcmdecoder_amd import build as b
    lib = P.bind(C.CDLL(b.build_hip()))
    got = {}
    for rate in (44056, 44100, 48000, 0, 32000):
        c = (C.c_double * 3)()
        lib.sdv_preemphasis_coeffs(rate, c)
        got[rate] = tuple(c)
        for g, w in zip(got[rate], coeffs(rate)):
            assert abs(g - w) <= 1e-15 * abs(w)
        c0, c1, c2 = got[rate]
        assert abs((c0 + c1) / (1 + c2) - 1.0) <= 1e-14                 # gain 1 at DC
        assert abs((c0 - c1) / (1 - c2) - 10.0 / 3.0) <= 1e-12          # gain T1 / T2 at fs / 2
    assert got[48000] == got[44100] and got[0] == got[44100] and got[32000] == got[44100] and got[44056] != got[44100]
    assert abs(got[44056][0] - 2.3283) < 1e-4 and abs(-got[44056][2] - 0.1386) < 1e-4         # 1 / b0; the pole at -b1 / b0


def test_the_condition_tells_float_from_double():
    pcm = signal("quiet", 10_000, seed=3)                # 20 000 samples
    want = walk(pcm, 44100)[0]
    f32 = walk(pcm, 44100, ftype=np.float32)[0]
    assert int((f32 != want).sum()) > 2
    with pytest.raises(AssertionError):
        check(f32, want)
    # ... and the walk is the network: a 10 kHz tone comes out at |H(z)|, the inverse of the de-emphasis's; DC passes as it is
    tone = walk(signal("tone", 2000), 44100)[0][1000:, 0].astype(float)
    c0, c1, c2 = coeffs(44100)
    z = np.exp(-2j * np.pi * 10000.0 / 44100)
    gain = abs((c0 + c1 * z) / (1 + c2 * z))
    b0, b1, a1 = de_coeffs(44100)
    assert abs(gain * abs((b0 + b1 * z) / (1 + a1 * z)) - 1.0) < 1e-12
    assert abs(np.sqrt(2 * np.mean(tone ** 2)) / 9000 - gain) < 5e-3
    step = walk(signal("step", 600), 44100)
    assert step[0][-1].tolist() == [30000, -32768] and step[2] > 0


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_emu_lengths(kind, n, emu):
    _lengths(emu, kind, n)


def test_emu_rates(emu):
    _rates(emu)


@pytest.mark.parametrize("cut", [1, T - 1, T, T + 100])
def test_emu_stream_in_two_calls(cut, emu):
    _split(emu, cut)


def test_emu_stream_in_many_calls(emu):
    _split_many(emu)


def test_emu_rate_change_restarts(emu):
    _rate_change_restarts(emu)


def test_emu_reset(emu):
    _reset(emu)


def test_emu_refusals_leave_the_state_alone(emu):
    _refusals(emu)


@pytest.mark.parametrize("kind", ["quiet", "tone"])
def test_emu_deemphasis_is_the_inverse(kind, emu):
    _inverse(emu, kind)


# ---- GPU: the same through the C-ABI of the product library ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_lengths(kind, n, gpu):
    _lengths(gpu, kind, n)


@pytest.mark.gpu
def test_gpu_rates(gpu):
    _rates(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("cut", [1, T - 1, T, T + 100])
def test_gpu_stream_in_two_calls(cut, gpu):
    _split(gpu, cut)


@pytest.mark.gpu
def test_gpu_stream_in_many_calls(gpu):
    _split_many(gpu)


@pytest.mark.gpu
def test_gpu_rate_change_restarts(gpu):
    _rate_change_restarts(gpu)


@pytest.mark.gpu
def test_gpu_reset(gpu):
    _reset(gpu)


@pytest.mark.gpu
def test_gpu_refusals_leave_the_state_alone(gpu):
    _refusals(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["quiet", "tone"])
def test_gpu_deemphasis_is_the_inverse(kind, gpu):
    _inverse(gpu, kind)


@pytest.mark.gpu
def test_gpu_engine_wrappers():
    """sdvpcmdecoder_amd.Engine: preemphasis_coeffs / reset_preemphasis / pcm_preemphasis / preemphasis_clipped."""
    import torch
    from sdvpcmdecoder_amd import Engine
    pcm = signal("noise", 3 * T + 1, seed=3)
    want, want_clipped = wanted(("len", "noise", 3 * T + 1), pcm, 44100)
    eng = Engine(0)
    assert np.allclose(eng.preemphasis_coeffs(44056), coeffs(44056), rtol=1e-15, atol=0) and np.allclose(eng.preemphasis_coeffs(1), coeffs(44100), rtol=1e-15, atol=0)
    d = torch.from_numpy(pcm).cuda()
    assert eng.preemphasis_clipped() == 0
    out = eng.pcm_preemphasis(d, 44100)
    assert out.shape == (len(pcm), 2) and out.dtype == torch.int16
    differ = check(out.cpu().numpy(), want)
    assert abs(eng.preemphasis_clipped() - want_clipped) <= differ
    eng.reset_preemphasis()
    assert eng.preemphasis_clipped() == 0
    mine = torch.empty_like(d)
    assert eng.pcm_preemphasis(d, 44100, out=mine).data_ptr() == mine.data_ptr() and np.array_equal(mine.cpu().numpy(), out.cpu().numpy())
    with pytest.raises(RuntimeError, match="overlap"):
        eng.pcm_preemphasis(d, 44100, out=d)
    assert eng.pcm_preemphasis(d[:0], 44100).shape == (0, 2)
    eng.close()


# ---- end to end on the GPU: 44 100 Hz PCM -> resample -> pre-emphasis -> the encoder -> the decoder ------------------------------------
def _mix_at(t):
    """a 1 kHz + 9 kHz mix of peak 8000 at the instants t (seconds) that starts at 0 in both channels: the filters then start from the state silence
    leaves them in, and the decoder's de-emphasis, which has run over the silence in front of the tape's first pair, is the inverse from the first
    word on"""
    a = np.zeros((len(t), 2))
    a[:, 0] = 5000 * np.sin(2 * np.pi * 1000.0 * t) + 3000 * np.sin(2 * np.pi * 9000.0 * t)
    a[:, 1] = 3000 * np.sin(2 * np.pi * 1000.0 * t) - 5000 * np.sin(2 * np.pi * 9000.0 * t)
    return a


def _mix(n):
    """... as n pairs of a 44 100 Hz WAV"""
    return np.rint(_mix_at(np.arange(n) / 44100.0)).astype(np.int16)


def _conditioned(eng, pcm):
    """-> (what pcm_resample made, what pcm_preemphasis made of it at 44056 Hz, the walks' versions); the device and the walks agree on every word"""
    import torch
    import test_pcm_resample as R
    flat = eng.pcm_resample(torch.from_numpy(pcm).cuda(), flush=True)
    want_flat = R.walk(pcm)
    assert np.array_equal(flat.cpu().numpy(), want_flat)
    emph = eng.pcm_preemphasis(flat, 44056)
    want_emph, _, want_clipped = walk(want_flat, 44056)
    assert np.array_equal(emph.cpu().numpy(), want_emph) and want_clipped == 0 and eng.preemphasis_clipped() == 0
    return flat.cpu().numpy(), emph, want_emph


N_MIX = 4 * 1470 * 1001 // 1000 - 20        # pairs of the WAV: 20 pairs short of 4 frames at 44 056 Hz, so that the tape's last pair is not the decoder's last


def _decoded(frames, pcm_type, deemph, emph, flat):
    """The tape through decode_frames (NEW_FILE | END_FILE, with_audio) under a de-emphasis mode -> its audio words from the tape's first pair on, as
    many as `flat` holds.  Where that pair lies behind the decoder's lead-in is found on the same tape decoded with the stage off, which gives `emph`."""
    import pcm16_api as p16
    from stitch_api import PAIR_DTYPE
    from sdvpcmdecoder_amd import Engine
    got = {}
    for mode in (0, deemph):
        eng = Engine(0)
        eng.setPCMType(pcm_type)
        if pcm_type == 1:
            st = eng.default_pcm16x0_stitch_settings()
            st.format = p16.FORMAT_SI
            eng.set_pcm16x0_stitch_settings(st)
        eng.set_deemphasis(mode)
        p = eng.decode_frames(pcm_type, frames, first_frame_no=1, new_file=True, end_file=True, with_audio=True, audio_stop=True)[0].cpu().numpy().view(PAIR_DTYPE).reshape(-1)
        got[mode] = p[p["service_type"] == 0]
        eng.close()
    raw = got[0]["audio_word"]
    first = next(k for k in range(len(raw) - len(emph) + 1) if np.array_equal(raw[k:k + 8], emph[:8]))
    assert np.array_equal(raw[first:first + len(emph)], emph)
    return got[deemph][first:first + len(flat)], got[0][first:first + len(flat)]


@pytest.mark.gpu
def test_gpu_end_to_end_stc007():
    """4 frames' worth of 44 100 Hz PCM -> pcm_resample -> pcm_preemphasis -> encode_frames (NTSC, 16 bit, control block with the emphasis bit, one
    frame more for the interleave delay) -> decode_frames with DEEMPH_FORCE: the conditioned-but-flat stream within 1 LSB; the frames equal the frames
    the encoder's yardstick makes from the walk's PCM byte for byte."""
    import encode_api as en
    from sdvpcmdecoder_amd import Engine
    eng = Engine(0)
    flat, emph, want_emph = _conditioned(eng, _mix(N_MIX))
    n = (len(flat) + 1469) // 1470 + 1
    assert n == 5
    frames = eng.encode_frames(emph, n, bits=16, ctrl_block=True, ctrl_flags=en.EMPHASIS, height=492)
    want = en.tape_frames(en.tape_words(want_emph, n, res=en.BIT16, ctrl=1, ctrl_flags=en.EMPHASIS), en.desc(res=en.BIT16, ctrl=1, ctrl_flags=en.EMPHASIS, height=492))
    assert np.array_equal(frames.cpu().numpy(), want)
    audio, _ = _decoded(frames, 2, 2, emph.cpu().numpy(), flat)
    d = np.abs(audio["audio_word"].astype(np.int64) - flat)
    print("decoded and de-emphasised against the flat stream: largest difference %d" % int(d.max()))
    assert len(d) == len(flat) and (d <= 1).all()
    eng.close()


@pytest.mark.gpu
def test_gpu_end_to_end_pcm16x0():
    """The same through encode_markerless_frames: pcm16x0_si with emphasis=True -> decode_frames with DEEMPH_AUTO, which goes by the pairs' emphasis
    field that chain sets."""
    import encode_markerless_api as ml
    from sdvpcmdecoder_amd import Engine
    eng = Engine(0)
    flat, emph, want_emph = _conditioned(eng, _mix(N_MIX))
    n = (len(flat) + 1469) // 1470
    assert n == 4
    frames = eng.encode_markerless_frames(emph, n, "pcm16x0_si", emphasis=True)
    assert np.array_equal(frames.cpu().numpy(), ml.tape_frames(want_emph, n, ml.desc(ml.SI, ctrl_flags=ml.EMPHASIS)))
    audio, raw = _decoded(frames, 1, 1, emph.cpu().numpy(), flat)
    assert (raw["emphasis"] == 1).all() and (audio["emphasis"] == 0).all()       # the chain sets the field; the stage has run: the stream is flat
    d = np.abs(audio["audio_word"].astype(np.int64) - flat)
    print("decoded and de-emphasised against the flat stream: largest difference %d" % int(d.max()))
    assert len(d) == len(flat) and (d <= 1).all()
    eng.close()


@pytest.mark.gpu
def test_gpu_decode_tape_from44100_preemph(tmp_path):
    """decode_tape encode in.wav out.luma 16 from44100 preemph, then decode_tape wav out.luma ... force 44100: the WAV comes back within 2 LSB away
    from the ends, with 44 100 in the header.  "Back": the decoder puts a lead-in of n0 pairs of silence in front of the tape's first pair (found here from
    the 44 056 Hz file the same program writes without `44100`), so the file that comes back is the signal n0 * 1.001 pairs late - not a whole number
    of pairs.  The WAV that went in is a sampled sum of two tones, so what has to come back at output m is that sum at (m - n0 * 1.001) / 44100 s; the
    walks of this file and of test_resample.py / test_deemphasis.py in float64 give it within 1.70."""
    import test_pcm_resample as R
    from sdvpcmdecoder_amd import build as b
    exe = b.build_example()
    pcm = _mix(N_MIX)
    hdr = b"RIFF" + (36 + pcm.nbytes).to_bytes(4, "little") + b"WAVEfmt " + (16).to_bytes(4, "little") + (1).to_bytes(2, "little") + (2).to_bytes(2, "little") + \
        (44100).to_bytes(4, "little") + (44100 * 4).to_bytes(4, "little") + (4).to_bytes(2, "little") + (16).to_bytes(2, "little") + b"data" + pcm.nbytes.to_bytes(4, "little")
    (tmp_path / "in.wav").write_bytes(hdr + pcm.tobytes())
    out = subprocess.run([exe, "encode", str(tmp_path / "in.wav"), str(tmp_path / "tape.luma"), "16", "from44100", "preemph"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "clipped" not in out.stderr, out.stderr + out.stdout
    n, width, height = (int(x) for x in out.stdout.split()[:3])
    assert (n, width, height) == (5, 720, 492) and (tmp_path / "tape.luma").stat().st_size == n * width * height
    out = subprocess.run([exe, "wav", str(tmp_path / "tape.luma"), str(width), str(height), str(n), str(tmp_path / "back.wav"), "force", "44100"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    raw = (tmp_path / "back.wav").read_bytes()
    assert raw[24:28] == (44100).to_bytes(4, "little")
    back = np.frombuffer(raw[44:], dtype=np.int16).reshape(-1, 2).astype(np.int64)
    out = subprocess.run([exe, "wav", str(tmp_path / "tape.luma"), str(width), str(height), str(n), str(tmp_path / "slow.wav"), "force"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    slow = (tmp_path / "slow.wav").read_bytes()
    assert slow[24:28] == (44056).to_bytes(4, "little")
    slow = np.frombuffer(slow[44:], dtype=np.int16).reshape(-1, 2).astype(np.int64)
    flat = R.walk(pcm).astype(np.int64)                 # the conditioned-but-flat stream: what the tape holds behind the de-emphasis
    n0 = next(k for k in range(len(slow) - len(flat) + 1) if (np.abs(slow[k + 100:k + 164] - flat[100:164]) <= 1).all())
    assert (np.abs(slow[n0:n0 + len(flat)] - flat) <= 1).all()
    late = n0 * 1.001
    d = np.abs(back - _mix_at((np.arange(len(back)) - late) / 44100.0))[int(late) + 200:int(late) + len(pcm) - 200]
    print("lead-in %d pairs; the WAV that came back against the signal that went in: largest difference %.3f away from the ends" % (n0, d.max()))
    assert len(d) == len(pcm) - 400 and d.max() <= 2
    # usage errors: from44100 on a PAL tape, and together with 44100
    for words in (["pal", "from44100"], ["pcm16si", "44100", "from44100"]):
        bad = subprocess.run([exe, "encode", str(tmp_path / "in.wav"), str(tmp_path / "x.luma")] + words, capture_output=True, text=True, timeout=300)
        assert bad.returncode == 1 and "usage" in bad.stderr
