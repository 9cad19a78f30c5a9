"""The skew stage of sdv_audio_resample (include/sdvpcm.h, SDV_RESAMPLE_DELAY_RIGHT / _LEFT): one channel of the PCMSamplePair stream half a sampling
period later, on the SIMT emulator (CPU) and through the C-ABI on the GPU (-m gpu), against `skew_walk` below - a plain sequential float64 evaluation
written from the definition in the header, with a row of taps of its own (numpy's i0 and sinc), never the code under test.  For the modes with
SDV_RESAMPLE_TO_44100 the expected stream is that walk over `walk` of tests/test_resample.py.

Tolerance, derived as in tests/test_resample.py and tests/test_pcm_resample.py: an output is a sum of 128 products in double.  A product is at most
2^15 |h|, the sum of |h| is 3.1436, so whatever the order of the additions (and with or without fused multiply-adds) y carries an error of at most about
128 * 2^-53 * 2^15 * 3.15 = 1.5e-9 LSB; the rows differ by 1e-14 per tap, 4e-8 LSB in the worst case.  A word can differ only where y lies that close
to a half, and then by one: every word within 1 LSB, at most 2 words per case (cases hold at most 200 000 samples) differing at all - test_resample's
`check`.  A float32 accumulation fails it on full-scale noise (test_the_condition_tells_float_from_double).  Every field but audio_word is compared
bytewise, the untouched channel too, and the output count must be equal."""
import ctypes as C
import math

import numpy as np
import pytest

import audio_api as A
import test_resample as R
from sdvpcmdecoder_amd import abi
from stitch_api import PAIR_DTYPE

T = 1024                # the device's tile (audio_skew_device.h); not in the header: no output depends on it, it only places the cases
HALF, WAIT = abi.RESAMPLE_HALF, abi.RESAMPLE_HALF - 1
OFF, ON, RIGHT, LEFT = abi.RESAMPLE_OFF, abi.RESAMPLE_TO_44100, abi.RESAMPLE_DELAY_RIGHT, abi.RESAMPLE_DELAY_LEFT
assert (OFF, ON, RIGHT, LEFT, abi.RESAMPLE_PHASE_HALF) == (0, 1, 4, 8, -1)
BAD_ARG = abi.ERR_BAD_ARG


# ---- the definition ----------------------------------------------------------------------------------------------------------
def _row():
    d = np.arange(2 * HALF, dtype=np.float64) - 63.5
    g = np.sinc(d) * np.i0(R.BETA * np.sqrt(1.0 - (d / HALF) ** 2)) / np.i0(R.BETA)
    return g / math.fsum(g)


ROW = _row()


def skew_segment(z, ch, ftype=np.float64):
    """A finished segment of n pairs -> its n pairs, channel ch half a sample later."""
    n = len(z)
    out = z.copy()
    x, h = z["audio_word"][:, ch].astype(ftype), ROW.astype(ftype)
    taps = np.arange(2 * HALF, dtype=np.int64)
    for a in range(0, n, 4096):
        m = np.arange(a, min(n, a + 4096), dtype=np.int64)
        prod = h[None, :] * x[np.clip(m[:, None] - HALF + taps[None, :], 0, n - 1)]
        y = np.zeros(len(m), dtype=ftype)
        for k in range(2 * HALF):                       # sequential, in the order of k
            y = y + prod[:, k]
        out["audio_word"][a:a + 4096, ch] = np.clip(np.rint(y.astype(np.float64)), -32768, 32767).astype(np.int16)
    return out


def skew_walk(pairs, ch, ftype=np.float64):
    """The whole stream in one call with flush -> the output stream."""
    srv, rate = pairs["service_type"] != 0, pairs["sample_rate"]
    out, i, n = [], 0, len(pairs)
    while i < n:
        j = i + 1
        if srv[i]:
            out.append(pairs[i:j].copy())
        else:
            while j < n and not srv[j] and rate[j] == rate[i]:
                j += 1
            out.append(skew_segment(pairs[i:j], ch, ftype))
        i = j
    return np.concatenate(out) if out else pairs[:0].copy()


def waiting(pairs):
    """Pairs that wait in the skew stage behind a call without flush that ends a stream of these pairs: the open segment's, at most 63."""
    n = k = len(pairs)
    while k > 0 and pairs["service_type"][k - 1] == 0 and pairs["sample_rate"][k - 1] == pairs["sample_rate"][n - 1]:
        k -= 1
    return min(n - k, WAIT)


def channel_of(mode):
    return 1 if mode & RIGHT else 0


def expected(pairs, mode):
    return skew_walk(R.walk(pairs) if mode & ON else pairs, channel_of(mode))


def check(got, want, source=None, mode=RIGHT):
    """The condition of the module's docstring; source: the stage's input, whose untouched channel and other fields must come out bytewise."""
    R.check(got, want)
    if source is not None:
        a, b = got.copy(), source.copy()
        a["audio_word"][:, channel_of(mode)] = 0; b["audio_word"][:, channel_of(mode)] = 0
        assert a.tobytes() == b.tobytes(), "the stage touched something other than the delayed channel's word"


_WANT = {}


def wanted(key, pairs, mode=RIGHT):
    """The walk over a case, computed once."""
    if (key, mode) not in _WANT:
        _WANT[(key, mode)] = expected(pairs, mode)
    return _WANT[(key, mode)].copy()


# ---- signals -------------------------------------------------------------------------------------------------------------------
def skewed_tones(n, fs=44056.0):
    """What a PCM-F1 records: left = rint(s(nT)), right = rint(s((n + 1/2) T)) for s a sum of tones at 997 Hz, 10 kHz and 18 kHz with peak 30000."""
    t = np.arange(n, dtype=np.float64) / fs

    def s(t):
        return 10000.0 * (np.sin(2 * np.pi * 997.0 * t) + np.sin(2 * np.pi * 10000.0 * t + 1.0) + np.sin(2 * np.pi * 18000.0 * t + 2.0))
    return np.stack([np.rint(s(t)), np.rint(s(t + 0.5 / fs))], axis=1).astype(np.int16)


SKEW_BOUND = 2.7        # 0.5 + 0.5 * 3.1436 + 0.5 for the three roundings (of left, of the row's inputs, of its output), + the passband ripple at 30000 (1.7e-5 dB: 0.06)


def _boundary_cases():
    c = {}
    n = 2 * T + 200
    for k, at in enumerate((0, 1, 62, 63, 64, T - 1)):  # positions of the second tile
        c["service_at_%d" % at] = R._tagged(R.stream("noise", n, 60 + k), [(T + at, 1 + k % 2)])
        a = R.stream("noise", n, 70 + k)
        a["sample_rate"][T + at:] = 44100
        c["rate_change_at_%d" % at] = a
    a = R._tagged(R.stream("noise", n, 80), [(T + 10, 1), (T + 11, 2), (2 * T - 5, 2)])       # closer than 64 to each other, and a rate in between
    a["sample_rate"][T + 40:T + 43] = 44100; a["sample_rate"][T + 43] = 48000
    c["two_fewer_than_64_apart"] = a
    c["service_first_and_last"] = R._tagged(R.stream("noise", n, 81), [(0, 1), (n - 1, 2)])
    return c


BOUNDARY_CASES = _boundary_cases()
LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, T - 1, T, T + 1, 3 * T + 1]
CUTS = [1, 63, 64, 65, T - 1, T, T + 100]


# ---- the two ways to the code under test (test_resample's back ends) -------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(emu_lib):
    be = R.Emu(emu_lib)
    yield be
    be.close()


@pytest.fixture(scope="module")
def gpu():
    be = R.Gpu()
    yield be
    be.close()


def run(be, pairs, mode, cuts=(), flush_last=True, reset=True, pendings=None):
    """The stream through a back end, in calls that end at `cuts` (a cut may repeat: a call of 0 pairs) -> the concatenated output"""
    n = len(pairs)
    src = be.buffer(pairs)
    if reset:
        be.reset()
    if mode is not None:
        assert be.mode(mode) == 0, be.error()
    ends = sorted(c for c in cuts if 0 <= c <= n) + [n]
    out, a = [], 0
    for k, b in enumerate(ends):
        last = k == len(ends) - 1
        cap = be.room(b - a)
        dst = be.buffer(n=cap + 1, fill=0xA5)
        rc, got = be.call(be.addr(src, a) if b > a else None, b - a, 1 if last and flush_last else 0, be.addr(dst), cap)
        assert rc == 0, be.error()
        assert got <= cap
        assert be.read(dst, cap, 1).view(np.uint8).tolist() == [0xA5] * 12          # nothing written behind the room that was asked for
        out.append(be.read(dst, 0, got))
        if pendings is not None:
            pendings.append(be.pending())
        assert be.pending() <= HALF + WAIT and (be.pending() == 0 or not (last and flush_last))
        a = b
    return np.concatenate(out)


def tail(be):
    """A call with no pairs and flush -> what waited"""
    cap = be.room(0)
    dst = be.buffer(n=cap + 1, fill=0xA5)
    rc, got = be.call(None, 0, 1, be.addr(dst), cap)
    assert rc == 0 and be.pending() == 0, be.error()
    assert be.read(dst, cap, 1).view(np.uint8).tolist() == [0xA5] * 12
    return be.read(dst, 0, got)


# ---- the checks, written once for both back ends ------------------------------------------------------------------------------
def _lengths(be, kind, n):
    pairs = R.stream(kind, 3 * T + 1, seed=5)[:n]
    got = run(be, pairs, RIGHT)
    if kind == "dc":                                    # a constant comes out constant, exactly, ends included
        assert got.tobytes() == pairs.tobytes()
    check(got, wanted(("len", kind, n), pairs), pairs)


def _split(be, cut):
    """Two calls, a call of 0 pairs between them, and the tail by a call with no pairs and flush."""
    pairs = R.stream("noise", 2 * T + 300, seed=33)
    n = len(pairs)
    pend = []
    got = run(be, pairs, RIGHT, cuts=(cut, cut), flush_last=False, pendings=pend)
    assert pend == [min(cut, WAIT), min(cut, WAIT), WAIT] and len(got) == n - WAIT
    check(np.concatenate([got, tail(be)]), wanted("split", pairs), pairs)


def _split_many(be):
    pairs = BOUNDARY_CASES["two_fewer_than_64_apart"]
    n = len(pairs)
    cuts = [0, 1, 2, 2, 40, 63, 64, 65, 127, 128, 300, T - 1, T, T, T + 1, T + 12, T + 30, T + 41, T + 50, T + 100, T + 107, 2 * T - 7, 2 * T, n - 63, n - 5, n, n]
    for mode in (RIGHT, LEFT):
        check(run(be, pairs, mode, cuts=cuts), wanted(("bnd", "two_fewer_than_64_apart"), pairs, mode), pairs, mode)
    # the last pair of the stream is a service pair: no flush is needed
    pairs = BOUNDARY_CASES["service_first_and_last"]
    check(run(be, pairs, RIGHT, cuts=(10, 70, T + 1), flush_last=False), wanted(("bnd", "service_first_and_last"), pairs), pairs)
    assert be.pending() == 0


def _boundaries(be, name):
    pairs = BOUNDARY_CASES[name]
    want = wanted(("bnd", name), pairs)
    check(run(be, pairs, RIGHT), want, pairs)
    # ... and with the first boundary as the last pair of a call without flush, and inside the last 63 pairs of one
    at = int(np.nonzero((pairs["service_type"] != 0) | (np.diff(pairs["sample_rate"].astype(np.int64), prepend=pairs["sample_rate"][0]) != 0))[0][0])
    cuts = [c for c in (at + 1, at + 30) if c < len(pairs)]
    pend = []
    check(run(be, pairs, RIGHT, cuts=cuts, pendings=pend), want, pairs)
    assert pend == [waiting(pairs[:c]) for c in cuts] + [0]


def _swapped(be):
    """DELAY_LEFT on the stream with its channels swapped is DELAY_RIGHT, swapped back - bit for bit: the same sums."""
    pairs = BOUNDARY_CASES["two_fewer_than_64_apart"]
    sw = pairs.copy()
    sw["audio_word"] = pairs["audio_word"][:, ::-1]; sw["sample_flags"] = pairs["sample_flags"][:, ::-1]
    right = run(be, pairs, RIGHT)
    left = run(be, sw, LEFT)
    back = left.copy()
    back["audio_word"] = left["audio_word"][:, ::-1]; back["sample_flags"] = left["sample_flags"][:, ::-1]
    assert back.tobytes() == right.tobytes()
    check(left, wanted("swapped", sw, LEFT), sw, LEFT)


def _behind_the_resampler(be, mode):
    """A 44 056 Hz segment with a 44 100 Hz run directly behind it: behind stage A the two are one segment of the skew stage."""
    pairs = R.stream("noise", 2 * T + 500, seed=91)
    pairs["sample_rate"][T + 300:] = 44100
    pairs = R._tagged(pairs, [(2 * T + 100, 2)])
    want = wanted("behind", pairs, mode)
    assert len(want) == len(pairs) + 1 and (want["sample_rate"] == 44100).sum() == len(want) - 1
    check(run(be, pairs, mode), want, R.walk(pairs), mode)
    pend = []
    check(run(be, pairs, mode, cuts=(30, 30, 64, 100, 191, T, T + 300, T + 301, 2 * T + 100), pendings=pend), want, R.walk(pairs), mode)
    assert pend[0] == 30 and max(pend) == HALF + WAIT and pend[-1] == 0
    # the tail of both stages by a call with no pairs
    head = run(be, pairs[:T], mode, flush_last=False)
    assert be.pending() == HALF + WAIT
    check(np.concatenate([head, tail(be)]), expected(pairs[:T], mode))


def _refusals(be):
    """Modes that do not exist, a change of the delay while pairs wait, a small out_cap and an overlap are refused with mode and state untouched:
    the stream in two calls with the refused calls in between."""
    pairs = R.stream("noise", T + 400, seed=43)
    n, cut = len(pairs), T - 100
    want = wanted("refusals", pairs)
    be.reset()
    assert be.mode(OFF) == 0 and be.mode(RIGHT) == 0
    for bad in (2, 3, 6, 7, 10, 12, 16, -1):
        assert be.mode(bad) == BAD_ARG and b"mode" in be.error(), bad
    buf = be.buffer(pairs, n=3 * n + 64)              # input, then room for outputs
    cap1 = be.room(cut)
    assert cap1 == cut
    rc, got1 = be.call(be.addr(buf), cut, 0, be.addr(buf, n), cap1)
    assert rc == 0 and got1 == cut - WAIT and be.pending() == WAIT
    first = be.read(buf, n, got1)
    before = be.read(buf, 0, 3 * n + 64)
    for other in (LEFT, LEFT | ON, OFF, ON):
        assert be.mode(other) == BAD_ARG and b"flush" in be.error() and b"reset" in be.error(), other
    assert be.mode(RIGHT | ON) == 0 and be.mode(RIGHT) == 0         # the same delay: not a change
    room = be.room(n - cut)
    assert room == n - cut + WAIT
    rc, got = be.call(be.addr(buf, cut), n - cut, 1, be.addr(buf, 2 * n), room - 1)
    assert rc == BAD_ARG and got == 0 and b"room" in be.error()
    for dst in (cut + 1, n - 1, cut - room + 1):
        rc, got = be.call(be.addr(buf, cut), n - cut, 1, be.addr(buf, dst), room)
        assert rc == BAD_ARG and b"overlap" in be.error(), dst
    assert be.call(None, 5, 1, be.addr(buf, 2 * n), room)[0] == abi.ERR_NULL_LINES
    assert be.call(be.addr(buf, cut), n - cut, 1, None, room)[0] == abi.ERR_NULL_BLOCK
    assert be.call(None, 0, 1, None, room)[0] == abi.ERR_NULL_BLOCK      # the tail that waits needs a buffer
    assert be.call(None, 0, 0, None, 0) == (0, 0)                       # nothing in, no flush: nothing happens
    assert be.pending() == WAIT and be.room(n - cut) == room
    assert be.read(buf, 0, 3 * n + 64).tobytes() == before.tobytes()
    rc, got2 = be.call(be.addr(buf, cut), n - cut, 1, be.addr(buf, 2 * n), room)
    assert rc == 0 and be.pending() == 0
    check(np.concatenate([first, be.read(buf, 2 * n, got2)]), want, pairs)
    # behind the flush nothing waits, and behind a reset: the delay may change
    assert be.mode(LEFT) == 0
    run(be, pairs[:100], None, reset=False, flush_last=False)
    assert be.pending() == WAIT and be.mode(RIGHT) == BAD_ARG
    be.reset()
    assert be.pending() == 0 and be.mode(RIGHT) == 0 and be.mode(OFF) == 0
    assert run(be, pairs, OFF).tobytes() == pairs.tobytes()


def _purpose(be):
    """What the stage is for: a signal whose right channel was sampled half a period behind the left one comes out with both channels in step."""
    pairs = np.zeros(1500, dtype=PAIR_DTYPE)
    pairs["audio_word"] = skewed_tones(1500)
    pairs["sample_rate"] = 44056
    pairs["sample_flags"] = 3
    pairs = R._tagged(pairs, [(700, 2)])
    got = run(be, pairs, RIGHT)
    inner = np.r_[100:600, 801:1400]                    # away from the 100 pairs at either end of the two segments
    before = np.abs(pairs["audio_word"][inner, 0].astype(np.int64) - pairs["audio_word"][inner, 1])
    after = np.abs(got["audio_word"][inner, 0].astype(np.int64) - got["audio_word"][inner, 1])
    print("largest |L - R|: %d without the stage, %d behind it" % (before.max(), after.max()))
    assert before.max() > 10000
    assert after.max() <= SKEW_BOUND
    check(got, wanted("purpose", pairs), pairs)


# ---- CPU: the row of the product library, the definition itself ------------------------------------------------------------------
def test_half_sample_row_of_the_product_library():
    from sdvpcmdecoder_amd import build as b
    lib = abi.bind(C.CDLL(b.build_hip()))
    c = (C.c_double * 128)()
    lib.sdv_resample_taps(abi.RESAMPLE_PHASE_HALF, c)
    got = np.array(c)
    assert np.abs(got - ROW).max() <= 1e-14
    for row in (got, ROW):
        assert (row == row[::-1]).all()                                             # h[k] = h[127 - k]
        assert abs(math.fsum(row) - 1.0) <= 1e-15 and np.abs(row).sum() <= 3.15
        assert abs(row[63] - 0.63640) < 1e-5 and abs(np.abs(row).sum() - 3.1436) < 1e-4
    # the phases of the resampler are what they were, and any other phase still gives zeros
    lib.sdv_resample_taps(500, c)
    assert np.abs(np.array(c) - R.TABLE[500]).max() <= 1e-14
    for phase in (-2, 1001):
        c = (C.c_double * 128)(*([7.0] * 128))
        lib.sdv_resample_taps(phase, c)
        assert list(c) == [0.0] * 128
    assert lib.sdv_abi_version() >= 13
    # the magnitude at 44.1 kHz: within 2e-5 dB of 1 up to 20 kHz (the definition's row in numpy has 1.70e-5 dB at 19.88 kHz and stays below 1.2e-5 dB
    # up to 19 kHz), -0.02 dB at 21 kHz
    mag = lambda f: abs(np.sum(got * np.exp(-2j * np.pi * f / 44100.0 * np.arange(128))))
    assert max(abs(20 * math.log10(mag(f))) for f in np.linspace(0.0, 20000.0, 501)) <= 2e-5
    assert abs(20 * math.log10(mag(21000.0)) + 0.02) < 0.005


def test_the_condition_tells_float_from_double():
    pairs = R.stream("noise", 3 * T + 1, seed=5)
    want = wanted(("len", "noise", 3 * T + 1), pairs)
    f32 = skew_walk(pairs, 1, ftype=np.float32)
    assert int((f32["audio_word"] != want["audio_word"]).sum()) > 2
    with pytest.raises(AssertionError):
        R.check(f32, want)
    # ... and the walk keeps what it should
    assert len(want) == len(pairs) and (want["audio_word"][:, 0] == pairs["audio_word"][:, 0]).all() and (want["audio_word"][:, 1] != pairs["audio_word"][:, 1]).any()


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("kind", ["noise", "dc"])
def test_emu_lengths(kind, n, emu):
    _lengths(emu, kind, n)


@pytest.mark.parametrize("cut", CUTS)
def test_emu_stream_in_calls(cut, emu):
    _split(emu, cut)


def test_emu_stream_in_many_calls(emu):
    _split_many(emu)


@pytest.mark.parametrize("name", sorted(BOUNDARY_CASES))
def test_emu_boundaries(name, emu):
    _boundaries(emu, name)


def test_emu_delay_left_is_delay_right_swapped(emu):
    _swapped(emu)


@pytest.mark.parametrize("mode", [RIGHT | ON, LEFT | ON])
def test_emu_behind_the_resampler(mode, emu):
    _behind_the_resampler(emu, mode)


def test_emu_refusals(emu):
    _refusals(emu)


def test_emu_purpose(emu):
    _purpose(emu)


# ---- GPU: the same through the C-ABI of the product library ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("kind", ["noise", "dc"])
def test_gpu_lengths(kind, n, gpu):
    _lengths(gpu, kind, n)


@pytest.mark.gpu
@pytest.mark.parametrize("cut", CUTS)
def test_gpu_stream_in_calls(cut, gpu):
    _split(gpu, cut)


@pytest.mark.gpu
def test_gpu_stream_in_many_calls(gpu):
    _split_many(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BOUNDARY_CASES))
def test_gpu_boundaries(name, gpu):
    _boundaries(gpu, name)


@pytest.mark.gpu
def test_gpu_delay_left_is_delay_right_swapped(gpu):
    _swapped(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [RIGHT | ON, LEFT | ON])
def test_gpu_behind_the_resampler(mode, gpu):
    _behind_the_resampler(gpu, mode)


@pytest.mark.gpu
def test_gpu_refusals(gpu):
    _refusals(gpu)


@pytest.mark.gpu
def test_gpu_purpose(gpu):
    _purpose(gpu)


@pytest.mark.gpu
def test_gpu_engine_200000_samples():
    """sdvpcmdecoder_amd.Engine: set_resample with a delay bit, audio_resample in two calls, resample_taps' half-sample row; 100 000 pairs, 98 tiles."""
    import torch
    from sdvpcmdecoder_amd import Engine
    pairs = R._tagged(R.stream("noise", 100_000, seed=7), [(40_000, 2), (40_001, 1)])
    pairs["sample_rate"][70_000:] = 44100
    eng = Engine(0)
    assert np.abs(np.array(eng.resample_taps(abi.RESAMPLE_PHASE_HALF)) - ROW).max() <= 1e-14
    d = torch.from_numpy(pairs.view(np.uint8).reshape(-1, 12).copy()).cuda()
    eng.set_resample(RIGHT)
    a = eng.audio_resample(d[:33_333])
    assert eng.audio_resample_pending() == WAIT and a.shape[0] == 33_333 - WAIT
    b = eng.audio_resample(d[33_333:], flush=True)
    assert eng.audio_resample_pending() == 0
    check(torch.cat([a, b]).cpu().numpy().view(PAIR_DTYPE).reshape(-1), expected(pairs, RIGHT), pairs)
    eng.audio_resample(d[:100])
    with pytest.raises(RuntimeError, match="flush"):
        eng.set_resample(LEFT)
    eng.reset_resample()
    eng.set_resample(LEFT)
    with pytest.raises(RuntimeError):
        eng.set_resample(RIGHT | LEFT)
    eng.close()


@pytest.mark.gpu
def test_gpu_chain_encode_decode_deskew():
    """Through the chain with Engine: the skewed pair signal encoded at 16 bit into NTSC frames, decoded with the audio stage, then the skew stage alone
    (SDV_RESAMPLE_DELAY_RIGHT): the two channels are in step, within the bound of the purpose test, away from the 100 pairs at either end of the signal
    (in front of it lies the decoder's silent lead-in, and where silence turns into three tones the signal is no band-limited one)."""
    import torch
    from sdvpcmdecoder_amd import Engine
    pcm = skewed_tones(2 * 1470)
    eng = Engine(0)
    frames = eng.encode_frames(torch.from_numpy(pcm).cuda(), 3, bits=16, ctrl_block=True, height=492)
    eng.setPCMType(abi.PCM_STC007)
    pairs = eng.decode_frames(abi.PCM_STC007, frames, first_frame_no=1, new_file=True, end_file=True, with_audio=True, audio_stop=True)[0]
    eng.set_resample(RIGHT)
    out = eng.audio_resample(pairs, flush=True)
    src, got = (t.cpu().numpy().view(PAIR_DTYPE).reshape(-1) for t in (pairs, out))
    eng.close()
    assert len(got) == len(src)
    check(got, expected(src, RIGHT), src)
    first = next(k for k in range(len(src) - len(pcm) + 1) if np.array_equal(src["audio_word"][k:k + 8], pcm[:8]))
    assert np.array_equal(src["audio_word"][first:first + len(pcm)], pcm) and (src["service_type"][first:first + len(pcm)] == 0).all()
    assert len(set(src["sample_rate"][first:first + len(pcm)].tolist())) == 1
    inner = slice(first + 100, first + len(pcm) - 100)
    before = np.abs(src["audio_word"][inner, 0].astype(np.int64) - src["audio_word"][inner, 1])
    after = np.abs(got["audio_word"][inner, 0].astype(np.int64) - got["audio_word"][inner, 1])
    print("largest |L - R|: %d as decoded, %d behind the stage" % (before.max(), after.max()))
    assert before.max() > 10000
    assert after.max() <= SKEW_BOUND
