"""sdv_audio_deemphasis (include/sdvpcm.h): the 50/15 us de-emphasis network on the PCMSamplePair stream, on the SIMT emulator (CPU)
and through the C-ABI on the GPU (-m gpu), against `walk` below - a plain sequential float64 loop written from the definition in the
header, never the code under test.

Tolerance, derived: the device evaluates the recurrence tile by tile as a scan of affine maps, in double.  Every output word then comes from
a y that differs from the sequential one by a few roundings of a double at magnitude 2^15 - about 1e-11 LSB - plus what a tile's state owes
to pairs more than 128 back (0.63^128 = 2e-26 of full scale).  So a word can differ only where y sits within 1e-11 of a half, and then by
one: every sample within 1 LSB, at most 2 samples per case (cases hold at most 200 000 samples) differing at all.  An accumulation in
float differs in about one sample per thousand - hundreds at that size, several in the smallest noise case here - and fails
(test_the_condition_tells_float_from_double).  Every field but audio_word is compared bytewise."""
import ctypes as C

import numpy as np
import pytest

import audio_api as A
from sdvpcmdecoder_amd import abi
from stitch_api import PAIR_DTYPE

T = abi.DEEMPH_TILE          # pairs per tile of the device's work
WARM = abi.DEEMPH_WARMUP     # pairs in front of a tile its state comes from
OFF, AUTO, FORCE = abi.DEEMPH_OFF, abi.DEEMPH_AUTO, abi.DEEMPH_FORCE
BAD_ARG, NULL_LINES, NULL_BLOCK = abi.ERR_BAD_ARG, abi.ERR_NULL_LINES, abi.ERR_NULL_BLOCK
T1, T2 = 50e-6, 15e-6


# ---- the definition ----------------------------------------------------------------------------------------------------------
def coeffs(rate):
    fs = 44056.0 if rate == 44056 else 44100.0
    k = 2.0 * fs
    return (1.0 + k * T2) / (1.0 + k * T1), (1.0 - k * T2) / (1.0 + k * T1), (1.0 - k * T1) / (1.0 + k * T1)


def walk(pairs, mode, state=None, ftype=np.float64):
    """-> (out, state).  state: per channel None (idle) or (fs, x_prev, y_prev)."""
    out = pairs.copy()
    st = [None, None] if state is None else list(state)
    if mode == OFF:
        return out, [None, None]
    co = {r: tuple(ftype(c) for c in coeffs(r)) for r in (44056, 44100)}
    words, rates, emph, srv = pairs["audio_word"], pairs["sample_rate"], pairs["emphasis"], pairs["service_type"]
    for i in range(len(pairs)):
        if srv[i] != 0 or not (mode == FORCE or emph[i] != 0):
            st = [None, None]
            continue
        fs = 44056 if rates[i] == 44056 else 44100
        b0, b1, a1 = co[fs]
        for ch in range(2):
            x = ftype(words[i, ch])
            if st[ch] is None or st[ch][0] != fs:
                y = x
            else:
                y = b0 * x + b1 * st[ch][1] - a1 * st[ch][2]
                out["audio_word"][i, ch] = int(min(max(np.rint(y), -32768), 32767))
            st[ch] = (fs, x, y)
        out["emphasis"][i] = 0
    return out, st


def check(got, want):
    """The condition of the module's docstring."""
    assert len(got) == len(want)
    a, b = got.copy(), want.copy()
    a["audio_word"] = 0; b["audio_word"] = 0
    assert a.tobytes() == b.tobytes(), "a field other than audio_word differs at pair %d" % int(np.nonzero(a.view(np.uint8).reshape(-1, 12) != b.view(np.uint8).reshape(-1, 12))[0][0])
    d = np.abs(got["audio_word"].astype(np.int64) - want["audio_word"].astype(np.int64))
    print("samples that differ: %d of %d, largest difference %d" % (int((d != 0).sum()), d.size, int(d.max()) if d.size else 0))
    assert d.size <= 200_000
    assert (d <= 1).all() and int((d != 0).sum()) <= 2, (int((d != 0).sum()), int(d.max()))


# ---- signals -------------------------------------------------------------------------------------------------------------------
def stream(kind, n, seed=1, rate=44056, emphasis=0):
    a = np.zeros(n, dtype=PAIR_DTYPE)
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    if kind == "noise":                                  # full scale, white
        a["audio_word"] = rng.integers(-32768, 32768, (n, 2))
    elif kind == "step":
        a["audio_word"][:, 0] = np.where(t >= n // 3, 30000, -20000)
        a["audio_word"][:, 1] = np.where(t >= 2, -32768, 32767)
    else:                                                # 10 kHz
        a["audio_word"][:, 0] = np.rint(32767 * np.sin(2 * np.pi * 10000.0 * t / rate))
        a["audio_word"][:, 1] = np.rint(20000 * np.cos(2 * np.pi * 10000.0 * t / rate))
    a["sample_flags"] = rng.integers(0, 16, (n, 2))      # (the stage neither reads nor alters them)
    a["sample_rate"] = rate
    a["emphasis"] = emphasis
    a["_pad"] = rng.integers(0, 65536, n)
    return a


def _runs(a, runs):
    for s, ln in runs:
        a["emphasis"][s:s + ln] = 1
    return a


def _auto_cases():
    n = 4 * T + 37
    c = {}
    c["start_on_last_pair_of_tile"] = _runs(stream("noise", n, 11), [(T - 1, 700), (3 * T - 1, T)])
    c["start_on_first_pair_of_tile"] = _runs(stream("noise", n, 12), [(T, 900), (3 * T, T + 37)])
    # runs shorter than the warm-up: in front of a tile edge, across it, ending on it, one pair long
    c["short_runs"] = _runs(stream("noise", n, 13), [(5, 1), (T - 40, 30), (T - 10, 20), (2 * T - WARM + 3, WARM - 3), (3 * T - 60, 61), (3 * T + 2, 7), (4 * T - 1, 1), (4 * T + 30, 7)])
    a = _runs(stream("noise", n, 14), [(0, n)])         # tags inside a run: at a tile edge and inside a warm-up window
    for i, kind in ((T - 1, 1), (T, 2), (2 * T - 50, 1), (2 * T - 1, 2), (3 * T, 1), (3 * T - WARM, 2), (3 * T - WARM - 1, 1), (4 * T + 36, 2)):
        a[i] = A.tag(kind)[0]
        a["emphasis"][i] = 1                             # (a service pair is never selected, whatever it carries)
    c["tags"] = a
    a = _runs(stream("noise", n, 15), [(0, n)])         # 44056 <-> 44100 in the middle of a run
    a["sample_rate"][700:T + 5] = 44100; a["sample_rate"][2 * T - 30:2 * T] = 44100; a["sample_rate"][3 * T:] = 44100; a["sample_rate"][3 * T + 500] = 48000
    c["rate_change"] = a
    a = _runs(stream("tone", n, 16), [(3, T - 3), (T + 1, 2 * T - 1), (3 * T + 100, 900)])
    a["sample_rate"][2 * T + 100:] = 44100
    a[2 * T - 7] = A.tag(2)[0]
    c["tone_mixed"] = a
    return c


AUTO_CASES = _auto_cases()
LENGTHS = [1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 1]
_WANT = {}


def wanted(key, pairs, mode):
    """The walk over a case, computed once."""
    if key not in _WANT:
        _WANT[key] = walk(pairs, mode)[0]
    return _WANT[key].copy()


# ---- the two ways to the code under test ---------------------------------------------------------------------------------------
class Emu:
    """The emulator build: host memory."""
    def __init__(self, lib):
        self.lib = lib
        self.h = C.c_void_p(self.lib.sdv_engine_create(0))

    def close(self):
        self.lib.sdv_engine_destroy(self.h)

    def mode(self, m):
        return self.lib.sdv_set_deemphasis(self.h, m)

    def reset(self):
        assert self.lib.sdv_reset_deemphasis(self.h) == 0

    def buffer(self, pairs, room=0):
        b = np.zeros(len(pairs) + room, dtype=PAIR_DTYPE)
        b[:len(pairs)] = pairs
        return b

    def call(self, buf, src, n, dst):
        """n pairs from pair `src` of the buffer to pair `dst` of it -> rc"""
        return self.lib.sdv_audio_deemphasis(self.h, buf.ctypes.data + 12 * src, n, buf.ctypes.data + 12 * dst, None)

    def read(self, buf, at, n):
        return buf[at:at + n].copy()


class Gpu:
    """The product library: device memory, the engine's C-ABI handle."""
    def __init__(self):
        from sdvpcmdecoder_amd import Engine
        self.eng = Engine(0)
        self.lib, self.h = self.eng.lib, self.eng._h

    def close(self):
        self.eng.close()

    def mode(self, m):
        return self.lib.sdv_set_deemphasis(self.h, m)

    def reset(self):
        assert self.lib.sdv_reset_deemphasis(self.h) == 0

    def buffer(self, pairs, room=0):
        import torch
        b = np.zeros(len(pairs) + room, dtype=PAIR_DTYPE)
        b[:len(pairs)] = pairs
        return torch.from_numpy(b.view(np.uint8).reshape(-1, 12).copy()).to("cuda:0")

    def call(self, buf, src, n, dst):
        import torch
        return self.lib.sdv_audio_deemphasis(self.h, buf.data_ptr() + 12 * src, n, buf.data_ptr() + 12 * dst, C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def read(self, buf, at, n):
        return buf[at:at + n].cpu().numpy().view(PAIR_DTYPE).reshape(-1).copy()


def run(be, pairs, mode, cuts=(), in_place=False, reset=True):
    """The stream through a back end, in calls that end at `cuts` -> the output"""
    n = len(pairs)
    buf = be.buffer(pairs, 0 if in_place else n)
    assert be.mode(mode) == 0
    if reset:
        be.reset()
    ends = sorted(set(c for c in cuts if 0 < c < n)) + [n]
    a = 0
    for b in ends:
        assert be.call(buf, a, b - a, a if in_place else n + a) == 0, be.lib.sdv_last_error(be.h)
        a = b
    return be.read(buf, 0 if in_place else n, n)


@pytest.fixture(scope="module")
def emu(emu_lib):
    be = Emu(emu_lib)
    yield be
    be.close()


@pytest.fixture(scope="module")
def gpu():
    be = Gpu()
    yield be
    be.close()


# ---- the checks, written once for both back ends ------------------------------------------------------------------------------
def _lengths(be, kind, n):
    pairs = stream(kind, 3 * T + 1, seed=3)[:n]
    check(run(be, pairs, FORCE), wanted(("len", kind, n), pairs, FORCE))       # FORCE on pairs without the flag


def _auto(be, name):
    pairs = AUTO_CASES[name]
    want = wanted(("auto", name), pairs, AUTO)
    got = run(be, pairs, AUTO)
    check(got, want)
    keep = (pairs["service_type"] != 0) | (pairs["emphasis"] == 0)
    assert got[keep].tobytes() == pairs[keep].tobytes()         # pairs and tags that are not selected: byte-identical
    assert (got["emphasis"][~keep] == 0).all() and (got["audio_word"][~keep] != pairs["audio_word"][~keep]).any()
    assert run(be, got, AUTO).tobytes() == got.tobytes()                        # a second AUTO pass is the identity
    assert run(be, got, AUTO, in_place=True).tobytes() == got.tobytes()
    assert run(be, pairs, OFF).tobytes() == pairs.tobytes()                     # OFF is a byte copy
    assert run(be, pairs, AUTO, in_place=True).tobytes() == got.tobytes()       # in place = out of place


def _force_all_signals(be):
    pairs = np.concatenate([stream("noise", T + 300, 21), stream("step", 700, 22), stream("tone", T + 77, 23), stream("noise", 500, 24, rate=44100)])
    want = wanted("force_mix", pairs, FORCE)
    got = run(be, pairs, FORCE)
    check(got, want)
    assert run(be, pairs, FORCE, in_place=True).tobytes() == got.tobytes()
    assert run(be, pairs, OFF, in_place=True).tobytes() == pairs.tobytes()


def _split(be, cut):
    pairs = stream("noise", 2 * T + 300, seed=31)
    want = wanted("split", pairs, FORCE)
    got = run(be, pairs, FORCE, cuts=(cut,))
    check(got, want)
    assert run(be, pairs, FORCE, cuts=(cut,), in_place=True).tobytes() == got.tobytes()


def _split_many(be):
    pairs = AUTO_CASES["tone_mixed"]
    check(run(be, pairs, AUTO, cuts=(1, 2, T - 1, T, T + 100, 2 * T - 7, 2 * T - 6, 3 * T + 99)), wanted(("auto", "tone_mixed"), pairs, AUTO))


def _overlap_refused(be):
    """A partial overlap is refused and leaves the state alone: the stream in two calls, with refused calls in between."""
    pairs = stream("noise", T + 400, seed=41)
    n, cut = len(pairs), T - 100
    buf = be.buffer(pairs, n + 8)
    assert be.mode(FORCE) == 0
    be.reset()
    assert be.call(buf, 0, cut, n + 8) == 0
    before = be.read(buf, 0, 2 * n + 8)
    for dst in (cut + 1, cut - 1, n - 1, cut - (n - cut) + 1):
        assert be.call(buf, cut, n - cut, dst) == BAD_ARG and b"overlap" in be.lib.sdv_last_error(be.h)
    assert be.lib.sdv_audio_deemphasis(be.h, None, 5, None, None) == NULL_LINES
    assert be.call(buf, 0, 0, 0) == 0                                           # n == 0
    assert be.lib.sdv_audio_deemphasis(be.h, None, 0, None, None) == 0
    assert be.mode(3) == BAD_ARG and be.mode(-1) == BAD_ARG                     # (the mode stays FORCE)
    assert be.read(buf, 0, 2 * n + 8).tobytes() == before.tobytes()
    assert be.call(buf, cut, n - cut, n + 8 + cut) == 0
    check(be.read(buf, n + 8, n), wanted("overlap", pairs, FORCE))
    assert be.read(buf, n + 8, n).tobytes() == run(be, pairs, FORCE, cuts=(cut,)).tobytes()


def _reset(be):
    """sdv_reset_deemphasis restarts click-free: the first pair behind it leaves as it came, what follows is a stream of its own."""
    a, b = stream("noise", T + 50, seed=51), stream("noise", 300, seed=52)
    run(be, a, FORCE)
    # without the reset the second burst goes on from the first
    carried = run(be, b, FORCE, reset=False)
    check(carried, wanted("reset_ab", np.concatenate([a[-200:], b]), FORCE)[200:])
    assert carried["audio_word"][0].tolist() != b["audio_word"][0].tolist()
    got = run(be, b, FORCE)                  # (run() resets)
    assert got["audio_word"][0].tolist() == b["audio_word"][0].tolist()
    check(got, wanted("reset_b", b, FORCE))
    # OFF leaves the state idle as well
    assert run(be, a, OFF, reset=False).tobytes() == a.tobytes()
    check(run(be, b, FORCE, reset=False), wanted("reset_b", b, FORCE))


# ---- CPU: the coefficients of the product library, the definition itself, the emulator ---------------------------------------------
def test_coefficients_of_the_product_library():
    from sdvpcmdecoder_amd import build as b
    lib = abi.bind(C.CDLL(b.build_hip()))
    got = {}
    for rate in (44056, 44100, 48000, 0, 32000):
        c = (C.c_double * 3)()
        lib.sdv_deemphasis_coeffs(rate, c)
        got[rate] = tuple(c)
        want = coeffs(rate)
        for g, w in zip(got[rate], want):
            assert abs(g - w) <= 1e-15 * abs(w)
        b0, b1, a1 = got[rate]
        assert abs((b0 + b1) - (1 + a1)) <= 1e-15                   # gain 1 at DC
        assert abs((b0 - b1) / (1 - a1) - 0.3) <= 1e-12             # gain T2 / T1 at fs / 2
    assert got[48000] == got[44100] and got[0] == got[44100] and got[32000] == got[44100] and got[44056] != got[44100]


def test_the_condition_tells_float_from_double():
    pairs = stream("noise", 3 * T + 1, seed=3)
    want = wanted(("len", "noise", 3 * T + 1), pairs, FORCE)
    f32 = walk(pairs, FORCE, ftype=np.float32)[0]
    assert int((f32["audio_word"] != want["audio_word"]).sum()) > 2
    with pytest.raises(AssertionError):
        check(f32, want)
    # ... and the walk is the network: a 10 kHz tone comes out at |H(z)|, which is the analog network's gain at the frequency the bilinear
    # transform maps 10 kHz to; DC passes as it is
    tone = walk(stream("tone", 2000, rate=44100), FORCE)[0]["audio_word"][1000:, 0].astype(float)
    b0, b1, a1 = coeffs(44100)
    z = np.exp(-2j * np.pi * 10000.0 / 44100)
    gain = abs((b0 + b1 * z) / (1 + a1 * z))
    w = 2 * 44100.0 * np.tan(np.pi * 10000.0 / 44100)
    assert abs(gain - abs((1 + 1j * w * T2) / (1 + 1j * w * T1))) < 1e-12
    assert abs(np.sqrt(2 * np.mean(tone ** 2)) / 32767 - gain) < 5e-3
    step = walk(stream("step", 600), FORCE)[0]["audio_word"]
    assert step[-1].tolist() == [30000, -32768]


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("kind", ["noise", "step", "tone"])
def test_emu_lengths_force(kind, n, emu):
    _lengths(emu, kind, n)


@pytest.mark.parametrize("name", sorted(AUTO_CASES))
def test_emu_auto(name, emu):
    _auto(emu, name)


def test_emu_force_all_signals(emu):
    _force_all_signals(emu)


@pytest.mark.parametrize("cut", [1, T - 1, T, T + 100])
def test_emu_stream_in_two_calls(cut, emu):
    _split(emu, cut)


def test_emu_stream_in_many_calls(emu):
    _split_many(emu)


def test_emu_partial_overlap_is_refused(emu):
    _overlap_refused(emu)


def test_emu_reset_restarts_click_free(emu):
    _reset(emu)


# ---- GPU: the same through the C-ABI of the product library ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("kind", ["noise", "step", "tone"])
def test_gpu_lengths_force(kind, n, gpu):
    _lengths(gpu, kind, n)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(AUTO_CASES))
def test_gpu_auto(name, gpu):
    _auto(gpu, name)


@pytest.mark.gpu
def test_gpu_force_all_signals(gpu):
    _force_all_signals(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("cut", [1, T - 1, T, T + 100])
def test_gpu_stream_in_two_calls(cut, gpu):
    _split(gpu, cut)


@pytest.mark.gpu
def test_gpu_stream_in_many_calls(gpu):
    _split_many(gpu)


@pytest.mark.gpu
def test_gpu_partial_overlap_is_refused(gpu):
    _overlap_refused(gpu)


@pytest.mark.gpu
def test_gpu_reset_restarts_click_free(gpu):
    _reset(gpu)


@pytest.mark.gpu
def test_gpu_engine_wrappers():
    """sdvpcmdecoder_amd.Engine: set_deemphasis / reset_deemphasis / audio_deemphasis / deemphasis_coeffs."""
    import torch
    from sdvpcmdecoder_amd import Engine
    pairs = AUTO_CASES["rate_change"]
    want = wanted(("auto", "rate_change"), pairs, AUTO)
    eng = Engine(0)
    assert np.allclose(eng.deemphasis_coeffs(44056), coeffs(44056), rtol=1e-15, atol=0) and np.allclose(eng.deemphasis_coeffs(1), coeffs(44100), rtol=1e-15, atol=0)
    d = torch.from_numpy(pairs.view(np.uint8).reshape(-1, 12).copy()).cuda()
    assert eng.audio_deemphasis(d).cpu().numpy().tobytes() == pairs.tobytes()           # the mode of a new engine is OFF
    eng.set_deemphasis(AUTO)
    out = eng.audio_deemphasis(d)
    got = out.cpu().numpy().view(PAIR_DTYPE).reshape(-1)
    check(got, want)
    eng.reset_deemphasis()
    assert eng.audio_deemphasis(d, out=d) is not None and d.cpu().numpy().tobytes() == got.tobytes()
    with pytest.raises(RuntimeError):
        eng.set_deemphasis(7)
    assert eng.audio_deemphasis(d[:0]).shape[0] == 0
    eng.close()


def _tape(fmt, n):
    import dist_worker
    from sdvpcmdecoder_amd import synth
    if fmt == 2:
        return synth.stc007_frames(n, seed=12, noise_sigma=4.0)[0].copy()
    return dist_worker.pcm_tape("pcm1" if fmt == 0 else "pcm16x0", n)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [2, 0, 1], ids=["stc007", "pcm1", "pcm16x0"])
def test_gpu_decode_frames_with_deemphasis_equals_separate_calls(fmt):
    """sdv_decode_frames(with_audio = 1) under FORCE = the separate entry points, sdv_audio_process, then sdv_audio_deemphasis: byte for byte
    (the same kernels on the same input in the same launch shape)."""
    import torch
    from sdvpcmdecoder_amd import Engine
    d = torch.from_numpy(np.ascontiguousarray(_tape(fmt, 3))).cuda()
    eng = Engine(0)
    eng.setPCMType(fmt)
    eng.set_audio_masking(A.DROP_INTER_LIN_WORD)
    if fmt == 2:
        lines, _ = eng.binarize_frames(d, first_frame_no=1, new_file=True, end_file=True)
        p, _ = eng.stitch_frames(lines)
    elif fmt == 0:
        lines, _ = eng.pcm1_binarize_frames(d, first_frame_no=1, new_file=True, end_file=True)
        p, _ = eng.pcm1_stitch_frames(eng.pcm1_bin_to_line_recs(lines))
    else:
        lines, _ = eng.pcm16x0_binarize_frames(d, first_frame_no=1, new_file=True, end_file=True)
        p, _ = eng.pcm16x0_stitch_frames(lines)
    masked, pur, _ = eng.audio_process(p, stop=True)
    flat_in = masked.cpu().numpy().view(PAIR_DTYPE).reshape(-1).copy()
    eng.set_deemphasis(FORCE)
    want = eng.audio_deemphasis(masked).cpu().numpy().view(PAIR_DTYPE).reshape(-1).copy()
    assert len(want) > 3 * 1400 and (want["audio_word"] != flat_in["audio_word"]).any()
    check(want, walk(flat_in, FORCE)[0])
    eng.close()
    for mode in (FORCE, OFF):
        fused = Engine(0)
        fused.setPCMType(fmt)
        fused.set_audio_masking(A.DROP_INTER_LIN_WORD)
        fused.set_deemphasis(mode)
        got, _, _, got_pur, _ = fused.decode_frames(fmt, d, first_frame_no=1, new_file=True, end_file=True, with_audio=True, audio_stop=True)
        assert got.cpu().numpy().tobytes() == (want if mode == FORCE else flat_in).tobytes() and got_pur.cpu().numpy().tobytes() == pur.cpu().numpy().tobytes()
        fused.close()
