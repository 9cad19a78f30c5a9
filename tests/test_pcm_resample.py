"""sdv_pcm_resample (include/sdvpcm.h): 44 100 Hz interleaved int16 PCM to 44 056 Hz by the 1000 / 1001 polyphase filter, on the SIMT emulator (CPU)
and through the C-ABI on the GPU (-m gpu), against `walk` below - a plain float64 evaluation of the definition in the header, summed in the order of k,
never the code under test.

Tolerance, derived: the device adds the same 128 products of at most 2^15 |h| in double, in the same order (it may fuse a product with its add);
its table is the library's, which differs from the one here by at most 1e-14 per tap (test_table).  A sum then differs from the walk's by about
1e-9 LSB at most, so a word can differ only where y lies within that of a half, and then by one: every word within 1 LSB, at most 2 words per case
(cases hold at most 200 000 samples - a cap, not a measurement) differing at all.  An accumulation in float32 differs in 7 of 3 070 outputs of
full-scale noise and fails (test_the_condition_tells_float_from_double)."""
import ctypes as C
import math

import numpy as np
import pytest

import pcm_condition_api as P
from pcm_condition_api import check

L, M, HALF, BETA = P.abi.PCM_RESAMPLE_L, P.abi.PCM_RESAMPLE_M, 64, 12.0         # 1000 outputs for 1001 pairs; 64 taps on each side
T = 4000                                        # outputs per tile of the device's work (not in the header: no output depends on it; it places the cases)


# ---- the definition ----------------------------------------------------------------------------------------------------------
def _table():
    k = np.arange(2 * HALF, dtype=np.float64)[None, :]
    p = np.arange(L, dtype=np.float64)[:, None]
    d = (k - (HALF - 1)) - p / L
    w = np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - (d / HALF) ** 2))) / np.i0(BETA)
    g = np.sinc(d) * w
    return g / np.array([math.fsum(row) for row in g])[:, None]


TABLE = _table()


def n_out_of(n):
    return (L * n - 1) // M + 1 if n >= 1 else 0


def walk(x, ftype=np.float64):
    """One stream of n pairs, (n, 2) int16 -> its n_out pairs."""
    n = len(x)
    m = np.arange(n_out_of(n), dtype=np.int64)
    i0, p = m * M // L, (m * M) % L
    out = np.zeros((len(m), 2), dtype=np.int16)
    h = TABLE.astype(ftype)
    taps = np.arange(2 * HALF, dtype=np.int64)
    for a in range(0, len(m), 4096):
        idx = np.clip(i0[a:a + 4096, None] - (HALF - 1) + taps[None, :], 0, n - 1)
        rows = h[p[a:a + 4096]]
        for ch in range(2):
            prod = rows * x[:, ch].astype(ftype)[idx]
            y = np.zeros(len(prod), dtype=ftype)
            for k in range(2 * HALF):                   # sequential, in the order of k
                y = y + prod[:, k]
            out[a:a + 4096, ch] = np.clip(np.rint(y.astype(np.float64)), -32768, 32767)
    return out


# ---- signals -------------------------------------------------------------------------------------------------------------------
def signal(kind, n, seed=1):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    a = np.zeros((n, 2), dtype=np.int16)
    if kind == "noise":                                  # full scale, white: sum |h| = 3.144, it clamps
        a[:] = rng.integers(-32768, 32768, (n, 2))
    elif kind == "dc":
        a[:, 0] = 12345; a[:, 1] = -32768
    else:                                                # a tone of `kind` Hz, amplitude 30000
        a[:, 0] = np.rint(30000 * np.sin(2 * np.pi * float(kind) * t / 44100.0))
        a[:, 1] = np.rint(30000 * np.cos(2 * np.pi * float(kind) * t / 44100.0))
    return a


LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 999, 1000, 1001, 1002, 2002, 2003, 3 * T + 1]
CUTS = [1, 63, 64, 65, 999, 1000, 1001, T - 1, T, T + 100]
_WANT = {}


def wanted(key, pcm):
    if key not in _WANT:
        _WANT[key] = walk(pcm)
    return _WANT[key].copy()


# ---- the code under test ---------------------------------------------------------------------------------------------------------
def run(be, pcm, cuts=(), flush_last=True, tail_call=False, reset=True):
    """The stream through a back end in calls that end at `cuts`; the last call flushes (tail_call: a call of its own with no pairs does) -> the
    output.  Checks pending and room on the way."""
    lib, h = be.lib, be.h
    n = len(pcm)
    src = be.buffer(pcm) if n else None
    if reset:
        assert lib.sdv_reset_pcm_resample(h) == P.OK
    ends = sorted(set(c for c in cuts if 0 < c < n)) + [n]
    calls = [(a, b, flush_last and not tail_call and b == n) for a, b in zip([0] + ends[:-1], ends)]
    if tail_call:
        calls.append((n, n, True))
    out, seen = [], 0
    for a, b, flush in calls:
        room = lib.sdv_pcm_resample_room(h, b - a)
        dst = be.buffer(np.full((room + 1, 2), 0x5A5A, dtype=np.int16))
        got = C.c_size_t(99)
        rc = lib.sdv_pcm_resample(h, be.ptr(src, 4 * a) if b > a else None, b - a, 1 if flush else 0, be.ptr(dst), room, C.byref(got), be.stream())
        assert rc == P.OK, lib.sdv_last_error(h)
        assert got.value <= room
        raw = P.pcm_of(be.read(dst), room + 1)
        assert (raw[got.value:] == 0x5A5A).all()        # nothing written behind the count
        out.append(raw[:got.value])
        seen = 0 if flush else seen + (b - a)
        assert lib.sdv_pcm_resample_pending(h) == min(seen, 64)
    return np.concatenate(out) if out else np.zeros((0, 2), dtype=np.int16)


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
def _lengths(be, n):
    pcm = signal("noise", 3 * T + 1, seed=3)[:n]
    got = run(be, pcm)
    assert len(got) == n_out_of(n) == (1000 * n - 1) // 1001 + 1
    check(got, wanted(("len", n), pcm))
    dc = signal("dc", n)
    assert np.array_equal(run(be, dc), dc[:n_out_of(n)])                # DC comes out exactly


def _tones(be, hz):
    """Every output within 2.1 of the ideal tone sampled at m 1.001 / 44100 s, away from the 100 outputs at either end: 0.5 sum |h| for the input's
    rounding, plus 0.5 for the output's, plus ripple.  Then the round trip: sdv_audio_resample (44056 -> 44100, flush) gives the input's length and
    the input within 2 away from the ends."""
    from stitch_api import PAIR_DTYPE
    pcm = signal(hz, 6000)
    got = run(be, pcm)
    check(got, wanted(("tone", hz), pcm))
    t = np.arange(len(got)) * 1.001 / 44100.0
    ideal = np.stack([30000 * np.sin(2 * np.pi * hz * t), 30000 * np.cos(2 * np.pi * hz * t)], axis=1)
    err = np.abs(got - ideal)[100:-100]
    print("%d Hz: largest distance from the ideal tone %.3f" % (hz, err.max()))
    assert err.max() <= 2.1
    lib, h = be.lib, be.h
    assert lib.sdv_set_resample(h, 1) == 0 and lib.sdv_reset_resample(h) == 0
    room = lib.sdv_audio_resample_room(h, len(got))
    src, dst = be.buffer(P.pairs_of(got, 44056)), be.buffer(np.zeros(room, dtype=PAIR_DTYPE))
    n_back = C.c_size_t(0)
    assert lib.sdv_audio_resample(h, be.ptr(src), len(got), 1, be.ptr(dst), room, C.byref(n_back), be.stream()) == 0, lib.sdv_last_error(h)
    assert lib.sdv_set_resample(h, 0) == 0
    assert n_back.value == len(pcm)
    back = be.read(dst).view(PAIR_DTYPE)[:n_back.value]
    assert (back["sample_rate"] == 44100).all()
    d = np.abs(back["audio_word"].astype(np.int64) - pcm)[100:-100]
    print("%d Hz: there and back, largest difference %d" % (hz, int(d.max())))
    assert d.max() <= 2


def _split(be, cut):
    pcm = signal("noise", T + 1200, seed=31)
    want = wanted("split", pcm)
    got = run(be, pcm, cuts=(cut,))
    check(got, want)
    assert np.array_equal(got, run(be, pcm, cuts=(cut,), tail_call=True))        # unflushed output plus the flushed tail equals one call


def _split_many(be):
    pcm = signal("noise", 2 * T + 777, seed=32)
    check(run(be, pcm, cuts=(1, 2, 63, 64, 65, 128, 999, 1000, 1001, 1002, 2002, T - 1, T, T + 100, 2 * T, 2 * T + 776), tail_call=True), wanted("many", pcm))


def _two_streams(be):
    """Two flushed streams back to back each start at phase 0; a stream left open is cut off by sdv_reset_pcm_resample."""
    a, b = signal("noise", 1500, seed=41), signal("noise", 700, seed=42)
    check(run(be, a), wanted("two_a", a))
    check(run(be, b, reset=False), wanted("two_b", b))
    run(be, a, flush_last=False)
    assert be.lib.sdv_pcm_resample_pending(be.h) == 64
    check(run(be, b), wanted("two_b", b))               # (run() resets)
    got = C.c_size_t(99)
    assert be.lib.sdv_pcm_resample(be.h, None, 0, 1, None, 0, C.byref(got), be.stream()) == P.OK and got.value == 0       # nothing open: nothing to flush
    assert be.lib.sdv_pcm_resample(be.h, None, 0, 0, None, 0, C.byref(got), be.stream()) == P.OK and got.value == 0


def _refusals(be):
    """Refusals come before any launch and leave the state untouched: the stream in two calls with refused calls in between equals one call."""
    pcm = signal("noise", 2500, seed=51)
    n, cut = len(pcm), 1100
    lib, h = be.lib, be.h
    buf = be.buffer(np.concatenate([pcm, np.full((n + 16, 2), 0x5A5A, dtype=np.int16)]))
    out = 4 * n
    got = C.c_size_t(0)
    assert lib.sdv_reset_pcm_resample(h) == P.OK
    assert lib.sdv_pcm_resample(h, be.ptr(buf), cut, 0, be.ptr(buf, out), n + 16, C.byref(got), be.stream()) == P.OK
    first = got.value
    assert first == n_out_of(cut - 64)
    before = be.read(buf)
    m = n - cut
    room = lib.sdv_pcm_resample_room(h, m)
    assert room == n_out_of(n) - first
    tail = out + 4 * first
    assert lib.sdv_pcm_resample(h, be.ptr(buf, 4 * cut), m, 1, be.ptr(buf, tail), room - 1, C.byref(got), be.stream()) == P.BAD_ARG and b"room" in lib.sdv_last_error(h)
    for dst, cap in ((4 * cut, room), (4 * (n - 1), room), (4 * (cut - 1), room), (0, n + 1)):
        assert lib.sdv_pcm_resample(h, be.ptr(buf, 4 * cut), m, 1, be.ptr(buf, dst), cap, C.byref(got), be.stream()) == P.BAD_ARG and b"overlap" in lib.sdv_last_error(h)
    for src_off, dst_off in ((2, 0), (0, 2), (1, 1)):
        assert lib.sdv_pcm_resample(h, be.ptr(buf, 4 * cut + src_off), m - 1, 1, be.ptr(buf, tail + dst_off), room, C.byref(got), be.stream()) == P.BAD_ARG
        assert b"aligned" in lib.sdv_last_error(h)
    assert lib.sdv_pcm_resample(h, None, 5, 0, be.ptr(buf, tail), room, C.byref(got), be.stream()) == P.NULL_LINES
    assert lib.sdv_pcm_resample(h, be.ptr(buf, 4 * cut), m, 1, None, room, C.byref(got), be.stream()) == P.NULL_BLOCK
    assert be.read(buf).tobytes() == before.tobytes() and lib.sdv_pcm_resample_pending(h) == 64 and lib.sdv_pcm_resample_room(h, m) == room
    assert lib.sdv_pcm_resample(h, be.ptr(buf, 4 * cut), m, 1, be.ptr(buf, tail), room, C.byref(got), be.stream()) == P.OK
    assert first + got.value == n_out_of(n)
    check(P.pcm_of(be.read(buf), n_out_of(n), out), wanted("refuse", pcm))


# ---- CPU: the table, the definition itself, the emulator -----------------------------------------------------------------------------
def test_table():
    from sdvpcmdecoder_amd import build as b
    lib = P.bind(C.CDLL(b.build_hip()))
    got = np.zeros((L, 2 * HALF))
    row = (C.c_double * 128)()
    for p in range(L):
        lib.sdv_pcm_resample_taps(p, row)
        got[p] = row
    assert np.abs(got - TABLE).max() <= 1e-14
    assert max(abs(math.fsum(r) - 1.0) for r in got) <= 1e-15                 # every phase: gain 1 at DC
    assert np.abs(got[1:] - got[:0:-1, ::-1]).max() <= 1e-14             # h[p][k] = h[1000 - p][127 - k]
    assert got[0, HALF - 1] == 1.0 and np.abs(np.delete(got[0], HALF - 1)).max() < 1e-15      # phase 0 is the pair itself
    assert 3.14 < np.abs(got).sum(axis=1).max() < 3.15                   # outputs clamp
    for p in (-1, L, L + 1, 5000):
        lib.sdv_pcm_resample_taps(p, row)
        assert not any(row)
    assert [n_out_of(n) for n in (1, 1000, 1001, 1002, 2003)] == [1, 1000, 1000, 1001, 2001]


def test_the_condition_tells_float_from_double():
    pcm = signal("noise", 3073, seed=3)                  # 3 070 outputs
    want = walk(pcm)
    assert len(want) == 3070
    f32 = walk(pcm, ftype=np.float32)
    assert int((f32 != want).sum()) > 2
    with pytest.raises(AssertionError):
        check(f32, want)


@pytest.mark.parametrize("n", LENGTHS)
def test_emu_lengths(n, emu):
    _lengths(emu, n)


@pytest.mark.parametrize("hz", [1000, 10000, 19000])
def test_emu_tones_and_round_trip(hz, emu):
    _tones(emu, hz)


@pytest.mark.parametrize("cut", CUTS)
def test_emu_stream_in_two_calls(cut, emu):
    _split(emu, cut)


def test_emu_stream_in_many_calls(emu):
    _split_many(emu)


def test_emu_two_streams(emu):
    _two_streams(emu)


def test_emu_refusals_leave_the_state_alone(emu):
    _refusals(emu)


# ---- GPU: the same through the C-ABI of the product library ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_gpu_lengths(n, gpu):
    _lengths(gpu, n)


@pytest.mark.gpu
@pytest.mark.parametrize("hz", [1000, 10000, 19000])
def test_gpu_tones_and_round_trip(hz, gpu):
    _tones(gpu, hz)


@pytest.mark.gpu
@pytest.mark.parametrize("cut", CUTS)
def test_gpu_stream_in_two_calls(cut, gpu):
    _split(gpu, cut)


@pytest.mark.gpu
def test_gpu_stream_in_many_calls(gpu):
    _split_many(gpu)


@pytest.mark.gpu
def test_gpu_two_streams(gpu):
    _two_streams(gpu)


@pytest.mark.gpu
def test_gpu_refusals_leave_the_state_alone(gpu):
    _refusals(gpu)


@pytest.mark.gpu
def test_gpu_engine_wrappers():
    """sdvpcmdecoder_amd.Engine: pcm_resample_taps / reset_pcm_resample / pcm_resample_pending / pcm_resample."""
    import torch
    from sdvpcmdecoder_amd import Engine
    pcm = signal("noise", T + 1200, seed=31)
    want = wanted("split", pcm)
    eng = Engine(0)
    assert np.abs(np.array(eng.pcm_resample_taps(137)) - TABLE[137]).max() <= 1e-14 and not any(eng.pcm_resample_taps(1000))
    d = torch.from_numpy(pcm).cuda()
    a = eng.pcm_resample(d[:1500])
    assert a.dtype == torch.int16 and a.shape == (n_out_of(1500 - 64), 2) and eng.pcm_resample_pending() == 64
    b = eng.pcm_resample(d[1500:], flush=True)
    assert eng.pcm_resample_pending() == 0
    check(torch.cat([a, b]).cpu().numpy(), want)
    mine = torch.empty((len(want) + 5, 2), dtype=torch.int16, device="cuda")
    got = eng.pcm_resample(d, flush=True, out=mine)
    assert got.data_ptr() == mine.data_ptr() and got.shape == (len(want), 2) and np.array_equal(got.cpu().numpy(), torch.cat([a, b]).cpu().numpy())
    eng.pcm_resample(d[:200])
    eng.reset_pcm_resample()
    assert eng.pcm_resample_pending() == 0
    with pytest.raises(RuntimeError, match="room"):
        eng.pcm_resample(d, flush=True, out=mine[:100])
    assert eng.pcm_resample(d[:0], flush=True).shape == (0, 2)
    eng.close()
