"""sdv_audio_resample (include/sdvpcm.h): 44 056 Hz segments of the PCMSamplePair stream to 44 100 Hz by the 1001 / 1000 polyphase filter, on
the SIMT emulator (CPU) and through the C-ABI on the GPU (-m gpu), against `walk` below - a plain sequential float64 evaluation written
from the definition in the header, with a tap table of its own (numpy's i0 and sinc), never the code under test.

Tolerance, derived: an output is a sum of 128 products in double.  A product is at most 2^15 |h|, the sum of |h| over a phase is at most 3.15,
so whatever the order of the additions (and with or without fused multiply-adds) y carries an error of at most about 128 * 2^-53 * 2^15 * 3.15
= 1.5e-9 LSB; the tables differ by 1e-14 per tap, 4e-8 LSB in the worst case.  A word can therefore differ only where y lies that close
to a half, and then by one: every word within 1 LSB, at most 2 words per case (cases hold at most 200 000 samples) differing at all - a cap,
not a measurement.  On full-scale noise the float64 walk has no differing word against its own taps summed in reverse order, a float32
accumulation differs in about one word of 430 and fails (test_the_condition_tells_float_from_double).
Every field but audio_word is compared bytewise, and the output count must be equal."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import audio_api as A
from sdvpcmdecoder_amd import abi
from stitch_api import PAIR_DTYPE

L, M, HALF = abi.RESAMPLE_L, abi.RESAMPLE_M, abi.RESAMPLE_HALF
assert (L, M, HALF) == (1001, 1000, 64)
T = 1024                # the device's tile (audio_resample_device.h); not in the header: no output depends on it, it only places the cases
OFF, ON = abi.RESAMPLE_OFF, abi.RESAMPLE_TO_44100
BAD_ARG, NULL_LINES, NULL_BLOCK = abi.ERR_BAD_ARG, abi.ERR_NULL_LINES, abi.ERR_NULL_BLOCK
BETA = 12.0


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
    return (n - 1) * L // M + 1


def resample_segment(x, ftype=np.float64, reverse=False):
    """A finished segment of n pairs -> its n_out pairs."""
    n = len(x)
    m = np.arange(n_out_of(n), dtype=np.int64)
    i0, p = m * M // L, (m * M) % L
    out = x[i0].copy()
    out["sample_rate"] = 44100
    h = TABLE.astype(ftype)
    taps = np.arange(2 * HALF, dtype=np.int64)
    for a in range(0, len(m), 4096):
        idx = np.clip(i0[a:a + 4096, None] - (HALF - 1) + taps[None, :], 0, n - 1)
        rows = h[p[a:a + 4096]]
        for ch in range(2):
            prod = rows * x["audio_word"][:, ch].astype(ftype)[idx]
            if reverse:
                prod = np.ascontiguousarray(prod[:, ::-1])
            y = np.zeros(len(prod), dtype=ftype)
            for k in range(2 * HALF):                   # sequential, in the order of k
                y = y + prod[:, k]
            out["audio_word"][a:a + 4096, ch] = np.clip(np.rint(y.astype(np.float64)), -32768, 32767).astype(np.int16)
    return out


def walk(pairs, ftype=np.float64, reverse=False):
    """The whole stream in one call with flush -> the output stream."""
    seg = (pairs["service_type"] == 0) & (pairs["sample_rate"] == 44056)
    out, i, n = [], 0, len(pairs)
    while i < n:
        j = i
        while j < n and seg[j] == seg[i]:
            j += 1
        out.append(resample_segment(pairs[i:j], ftype, reverse) if seg[i] else pairs[i:j].copy())
        i = j
    return np.concatenate(out) if out else pairs[:0].copy()


def check(got, want):
    """The condition of the module's docstring."""
    assert len(got) == len(want), (len(got), len(want))
    a, b = got.copy(), want.copy()
    a["audio_word"] = 0; b["audio_word"] = 0
    assert a.tobytes() == b.tobytes(), "a field other than audio_word differs at pair %d" % int(np.nonzero(a.view(np.uint8).reshape(-1, 12) != b.view(np.uint8).reshape(-1, 12))[0][0])
    d = np.abs(got["audio_word"].astype(np.int64) - want["audio_word"].astype(np.int64))
    print("samples that differ: %d of %d, largest difference %d" % (int((d != 0).sum()), d.size, int(d.max()) if d.size else 0))
    assert d.size <= 200_000
    assert (d <= 1).all() and int((d != 0).sum()) <= 2, (int((d != 0).sum()), int(d.max()))


# ---- signals -------------------------------------------------------------------------------------------------------------------
def stream(kind, n, seed=1, rate=44056):
    a = np.zeros(n, dtype=PAIR_DTYPE)
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    if kind == "noise":                                  # full scale, white
        a["audio_word"] = rng.integers(-32768, 32768, (n, 2))
    elif kind == "step":
        a["audio_word"][:, 0] = np.where(t >= n // 3, 30000, -20000)
        a["audio_word"][:, 1] = np.where(t >= 2, -32768, 32767)
    elif kind == "dc":
        a["audio_word"][:, 0] = 32767
        a["audio_word"][:, 1] = -12345
    else:                                                # 1 kHz, amplitude 20 000, sampled at 44 100 / 1.001 Hz
        a["audio_word"][:, 0] = np.rint(20000 * np.sin(2 * np.pi * 1000.0 * t * 1.001 / 44100.0))
        a["audio_word"][:, 1] = np.rint(20000 * np.cos(2 * np.pi * 1000.0 * t * 1.001 / 44100.0))
    a["sample_flags"] = rng.integers(0, 16, (n, 2))      # (the stage carries them along)
    a["sample_rate"] = rate
    a["emphasis"] = rng.integers(0, 2, n)
    a["_pad"] = rng.integers(0, 65536, n)
    return a


def _tagged(a, tags):
    for i, kind in tags:
        a[i] = A.tag(kind)[0]
    return a


def _boundary_cases():
    n = 4 * T + 37
    c = {}
    # tags at a tile edge and one pair either side of it, inside the last 64 pairs of the call, and as its last pair
    c["tags_at_tile_edges"] = _tagged(stream("noise", n, 11), [(T - 1, 1), (2 * T, 2), (3 * T + 1, 1), (n - 30, 2)])
    c["tag_is_last_pair"] = _tagged(stream("noise", n, 12), [(T, 1), (T + 1, 2), (n - 1, 2)])
    c["tag_is_first_pair"] = _tagged(stream("noise", 2 * T + 5, 13), [(0, 1), (2 * T + 4 - 64, 2)])
    a = stream("noise", n, 14)                          # runs of 44100 pairs and one pair of another rate inside a 44056 stream
    a["sample_rate"][700:T + 5] = 44100; a["sample_rate"][2 * T - 30:2 * T] = 44100; a["sample_rate"][3 * T + 500] = 48000; a["sample_rate"][n - 3:] = 44100
    c["rate_changes"] = a
    # segments of one pair (and of two) between two tags, in the middle of a tile and across a tile edge
    c["one_pair_segments"] = _tagged(stream("noise", 3 * T, 15), [(5, 1), (7, 2), (9, 1), (12, 2), (T - 2, 1), (T, 2), (2 * T - 1, 1), (2 * T + 1, 2), (2 * T + 70, 1)])
    c["tone_with_tags"] = _tagged(stream("tone", 2 * T + 900, 16), [(1500, 2), (1501, 1)])
    return c


BOUNDARY_CASES = _boundary_cases()
LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 999, 1000, 1001, 1002, 2002, T - 1, T, T + 1, 3 * T + 1]
CUTS = [1, 63, 64, 65, T - 1, T, T + 100, 1000, 1001]     # (pair 1000 of a segment is the one that owns two outputs: cut in front of it and behind it)
_WANT = {}


def wanted(key, pairs):
    """The walk over a case, computed once."""
    if key not in _WANT:
        _WANT[key] = walk(pairs)
    return _WANT[key].copy()


# ---- the two ways to the code under test ---------------------------------------------------------------------------------------
class Backend:
    def mode(self, m):
        return self.lib.sdv_set_resample(self.h, m)

    def reset(self):
        assert self.lib.sdv_reset_resample(self.h) == 0

    def pending(self):
        return int(self.lib.sdv_audio_resample_pending(self.h))

    def room(self, n):
        return int(self.lib.sdv_audio_resample_room(self.h, n))

    def call(self, src, n, flush, dst, cap, stream=None):
        """n pairs at address src -> (rc, n_out); addresses may be None"""
        n_out = C.c_size_t(12345)
        rc = self.lib.sdv_audio_resample(self.h, src, n, flush, dst, cap, C.byref(n_out), self.stream() if stream is None else stream)
        return rc, int(n_out.value)

    def error(self):
        return self.lib.sdv_last_error(self.h)


class Emu(Backend):
    """The emulator build: host memory."""
    def __init__(self, lib):
        self.lib = lib
        self.h = C.c_void_p(self.lib.sdv_engine_create(0))

    def close(self):
        self.lib.sdv_engine_destroy(self.h)

    def stream(self):
        return None

    def buffer(self, pairs=None, n=0, fill=0):
        b = np.full(max(n, 1 if pairs is None else len(pairs)) * 12, fill, dtype=np.uint8).view(PAIR_DTYPE)
        if pairs is not None:
            b[:len(pairs)] = pairs
        return b

    def addr(self, buf, at=0):
        return buf.ctypes.data + 12 * at

    def read(self, buf, at, n):
        return buf[at:at + n].copy()


class Gpu(Backend):
    """The product library: device memory, the engine's C-ABI handle."""
    def __init__(self):
        from sdvpcmdecoder_amd import Engine
        self.eng = Engine(0)
        self.lib, self.h = self.eng.lib, self.eng._h

    def close(self):
        self.eng.close()

    def stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def buffer(self, pairs=None, n=0, fill=0):
        import torch
        b = np.full(max(n, 1 if pairs is None else len(pairs)) * 12, fill, dtype=np.uint8).view(PAIR_DTYPE)
        if pairs is not None:
            b[:len(pairs)] = pairs
        return torch.from_numpy(b.view(np.uint8).reshape(-1, 12).copy()).to("cuda:0")

    def addr(self, buf, at=0):
        return buf.data_ptr() + 12 * at

    def read(self, buf, at, n):
        return buf[at:at + n].cpu().numpy().view(PAIR_DTYPE).reshape(-1).copy()


def run(be, pairs, cuts=(), flush_last=True, reset=True, mode=ON, pendings=None):
    """The stream through a back end, in calls that end at `cuts` (a cut may repeat: a call of 0 pairs) -> the concatenated output"""
    n = len(pairs)
    src = be.buffer(pairs)
    assert be.mode(mode) == 0
    if reset:
        be.reset()
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
        assert be.pending() <= HALF and (be.pending() == 0 or not (last and flush_last))
        a = b
    return np.concatenate(out)


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
    got = run(be, pairs)
    assert len(got) == n_out_of(n)
    check(got, wanted(("len", kind, n), pairs))


def _dc(be):
    """A constant comes out constant, exactly, ends included."""
    for n in (1, 70, T + 5, 2 * T + 300):
        got = run(be, stream("dc", n))
        assert len(got) == n_out_of(n) and (got["audio_word"][:, 0] == 32767).all() and (got["audio_word"][:, 1] == -12345).all() and (got["sample_rate"] == 44100).all()


def _tone(be):
    """1 kHz at 44 100 / 1.001 Hz in, the same tone sampled at 44 100 Hz out: within 2 LSB away from the ends (the float64 definition is within
    1.08; the margin is the rounding of the input and of the output)."""
    n = 3 * T
    got = run(be, stream("tone", n))
    t = np.arange(len(got))
    ideal = np.stack([20000 * np.sin(2 * np.pi * 1000.0 * t / 44100.0), 20000 * np.cos(2 * np.pi * 1000.0 * t / 44100.0)], axis=1)
    err = np.abs(got["audio_word"].astype(np.float64) - ideal)[2 * HALF:-2 * HALF]
    print("tone: largest deviation %.3f LSB" % err.max())
    assert err.max() <= 2.0


def _boundaries(be, name):
    pairs = BOUNDARY_CASES[name]
    want = wanted(("bnd", name), pairs)
    got = run(be, pairs)
    check(got, want)
    keep = (pairs["service_type"] != 0) | (pairs["sample_rate"] != 44056)
    assert got[_through_positions(pairs)].tobytes() == pairs[keep].tobytes()       # what is not in a segment: byte-identical, at its place
    assert run(be, pairs, mode=OFF).tobytes() == pairs.tobytes()        # OFF is a byte copy


def _through_positions(pairs):
    """Output positions of the pairs that go through (the walk's bookkeeping, for 44100 pairs that cannot be told from outputs by their fields)."""
    seg = (pairs["service_type"] == 0) & (pairs["sample_rate"] == 44056)
    pos, out, i, n = [], 0, 0, len(pairs)
    while i < n:
        j = i
        while j < n and seg[j] == seg[i]:
            j += 1
        if seg[i]:
            out += n_out_of(j - i)
        else:
            pos.extend(range(out, out + j - i)); out += j - i
        i = j
    return np.array(pos, dtype=np.int64)


def _identity(be):
    a = stream("noise", T + 70, 17, rate=44100)
    a = _tagged(a, [(0, 1), (T, 2), (T + 69, 2)])
    a["sample_rate"][5] = 48000
    assert run(be, a).tobytes() == a.tobytes()
    assert run(be, a, cuts=(3, T, T + 1), flush_last=False).tobytes() == a.tobytes() and be.pending() == 0


def _split(be, cut):
    pairs = stream("noise", 2 * T + 300, seed=31)
    want = wanted("split", pairs)
    pend = []
    check(run(be, pairs, cuts=(cut,), pendings=pend), want)
    assert pend == [min(cut, HALF), 0]


def _split_many(be):
    pairs = BOUNDARY_CASES["tags_at_tile_edges"]
    want = wanted(("bnd", "tags_at_tile_edges"), pairs)
    n = len(pairs)
    cuts = [0, 1, 2, 2, 40, 70, 100, 163, 164, 300, T - 1, T, T, T + 1, T + 50, 2 * T - 7, 2 * T + 1001, 3 * T + 2, n - 31, n - 30, n - 29, n - 5, n, n]
    check(run(be, pairs, cuts=cuts), want)
    # the last pair of the stream ends the segment: no flush is needed
    pairs = BOUNDARY_CASES["tag_is_last_pair"]
    check(run(be, pairs, cuts=(10, 50, T + 1, 3 * T), flush_last=False), wanted(("bnd", "tag_is_last_pair"), pairs))
    assert be.pending() == 0


def _refusals(be):
    """Small out_cap, an overlap and null pointers are refused with the state untouched: the stream in two calls with refused calls in between."""
    pairs = stream("noise", T + 400, seed=41)
    n, cut = len(pairs), T - 100
    want = wanted("refusals", pairs)
    assert be.mode(ON) == 0
    be.reset()
    buf = be.buffer(pairs, n=3 * n + 64)              # input, then room for outputs
    cap1 = be.room(cut)
    rc, got1 = be.call(be.addr(buf), cut, 0, be.addr(buf, n), cap1)
    assert rc == 0 and be.pending() == HALF
    first = be.read(buf, n, got1)
    before = be.read(buf, 0, 3 * n + 64)
    room = be.room(n - cut)
    assert room >= n_out_of(n) - got1
    rc, got = be.call(be.addr(buf, cut), n - cut, 1, be.addr(buf, 2 * n), room - 1)
    assert rc == BAD_ARG and got == 0 and b"room" in be.error()
    for dst in (cut + 1, n - 1, cut - room + 1):
        rc, got = be.call(be.addr(buf, cut), n - cut, 1, be.addr(buf, dst), room)
        assert rc == BAD_ARG and b"overlap" in be.error(), dst
    assert be.call(None, 5, 1, be.addr(buf, 2 * n), room)[0] == NULL_LINES
    assert be.call(be.addr(buf, cut), n - cut, 1, None, room)[0] == NULL_BLOCK
    assert be.call(None, 0, 1, None, room)[0] == NULL_BLOCK             # the tail that waits needs a buffer
    assert be.lib.sdv_audio_resample(be.h, be.addr(buf, cut), n - cut, 1, be.addr(buf, 2 * n), room, None, be.stream()) == BAD_ARG
    assert be.mode(2) == BAD_ARG and be.mode(-1) == BAD_ARG             # (the mode stays as it is)
    assert be.call(None, 0, 0, None, 0) == (0, 0)                       # nothing in, no flush: nothing happens
    assert be.pending() == HALF and be.room(n - cut) == room
    assert be.read(buf, 0, 3 * n + 64).tobytes() == before.tobytes()
    rc, got2 = be.call(be.addr(buf, cut), n - cut, 1, be.addr(buf, 2 * n), room)
    assert rc == 0 and be.pending() == 0
    check(np.concatenate([first, be.read(buf, 2 * n, got2)]), want)


def _reset_and_off(be):
    """sdv_reset_resample drops what waits; OFF copies and leaves the state empty."""
    a, b = stream("noise", 300, seed=51), stream("noise", 200, seed=52)
    head = run(be, a, flush_last=False)
    assert be.pending() == HALF and 0 < len(head) < n_out_of(300)
    got = run(be, b)                                    # (run() resets)
    check(got, wanted("reset_b", b))
    run(be, a, flush_last=False)
    carried = run(be, b, reset=False)                   # without the reset the second burst goes on from the first
    check(np.concatenate([head, carried]), wanted("reset_ab", np.concatenate([a, b])))
    run(be, a, flush_last=False)
    assert run(be, a, mode=OFF, reset=False, flush_last=False).tobytes() == a.tobytes() and be.pending() == 0
    check(run(be, b, reset=False), wanted("reset_b", b))
    # a flush with nothing in puts out the tail
    head = run(be, a, flush_last=False)
    dst = be.buffer(n=be.room(0))
    rc, got = be.call(None, 0, 1, be.addr(dst), be.room(0))
    assert rc == 0 and got == n_out_of(300) - len(head) and be.pending() == 0
    check(np.concatenate([head, be.read(dst, 0, got)]), wanted("reset_a", a))


# ---- CPU: the taps of the product library, the definition itself, the emulator ---------------------------------------------------
def test_symbols_and_taps_of_the_product_library():
    from sdvpcmdecoder_amd import build as b
    lib = abi.bind(C.CDLL(b.build_hip()))
    got = np.zeros((L, 2 * HALF))
    for p in range(L):
        c = (C.c_double * 128)()
        lib.sdv_resample_taps(p, c)
        got[p] = c
    assert np.abs(got - TABLE).max() <= 1e-14
    for tab in (got, TABLE):
        assert max(abs(math.fsum(row) - 1.0) for row in tab) <= 1e-15                           # gain 1 at DC, every phase
        assert np.abs(tab[1:] - tab[:0:-1, ::-1]).max() <= 1e-14                                 # h[p][k] = h[1001 - p][127 - k]
        assert np.abs(tab).sum(axis=1).max() <= 3.15
    assert got[0, HALF - 1] == got[0].max() and abs(got[0, HALF - 1] - 1.0) < 1e-12             # phase 0 is the identity
    c = (C.c_double * 128)(*([7.0] * 128))
    lib.sdv_resample_taps(L, c)
    assert list(c) == [0.0] * 128
    assert lib.sdv_abi_version() >= 7


def test_the_condition_tells_float_from_double():
    pairs = stream("noise", 3 * T + 1, seed=3)
    want = wanted(("len", "noise", 3 * T + 1), pairs)
    check(walk(pairs, reverse=True), want)                                                      # another order of the sum: within the cap
    f32 = walk(pairs, ftype=np.float32)
    assert int((f32["audio_word"] != want["audio_word"]).sum()) > 2
    with pytest.raises(AssertionError):
        check(f32, want)
    assert len(want) == n_out_of(3 * T + 1) and (want["sample_rate"] == 44100).all()
    # ... and the walk keeps what it should: an output carries the fields of x[i0]
    m = np.arange(len(want))
    assert (want["sample_flags"] == pairs["sample_flags"][m * M // L]).all() and (want["_pad"] == pairs["_pad"][m * M // L]).all()


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("kind", ["noise", "step", "tone"])
def test_emu_lengths(kind, n, emu):
    _lengths(emu, kind, n)


def test_emu_dc(emu):
    _dc(emu)


def test_emu_tone(emu):
    _tone(emu)


@pytest.mark.parametrize("name", sorted(BOUNDARY_CASES))
def test_emu_boundaries(name, emu):
    _boundaries(emu, name)


def test_emu_pass_through_only_is_the_identity(emu):
    _identity(emu)


@pytest.mark.parametrize("cut", CUTS)
def test_emu_stream_in_two_calls(cut, emu):
    _split(emu, cut)


def test_emu_stream_in_many_calls(emu):
    _split_many(emu)


def test_emu_refusals(emu):
    _refusals(emu)


def test_emu_reset_and_off(emu):
    _reset_and_off(emu)


# ---- GPU: the same through the C-ABI of the product library ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("kind", ["noise", "step", "tone"])
def test_gpu_lengths(kind, n, gpu):
    _lengths(gpu, kind, n)


@pytest.mark.gpu
def test_gpu_dc(gpu):
    _dc(gpu)


@pytest.mark.gpu
def test_gpu_tone(gpu):
    _tone(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BOUNDARY_CASES))
def test_gpu_boundaries(name, gpu):
    _boundaries(gpu, name)


@pytest.mark.gpu
def test_gpu_pass_through_only_is_the_identity(gpu):
    _identity(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("cut", CUTS)
def test_gpu_stream_in_two_calls(cut, gpu):
    _split(gpu, cut)


@pytest.mark.gpu
def test_gpu_stream_in_many_calls(gpu):
    _split_many(gpu)


@pytest.mark.gpu
def test_gpu_refusals(gpu):
    _refusals(gpu)


@pytest.mark.gpu
def test_gpu_reset_and_off(gpu):
    _reset_and_off(gpu)


@pytest.mark.gpu
def test_gpu_busy_side_stream(gpu):
    """All device work goes on `stream` and the call returns when the outputs are complete: a non-blocking side stream that is busy writing
    the input, the output buffer pre-filled, nothing synchronised by the caller between the call and the read-back on another stream."""
    import torch
    pairs = BOUNDARY_CASES["tags_at_tile_edges"]
    want = wanted(("bnd", "tags_at_tile_edges"), pairs)
    n = len(pairs)
    assert gpu.mode(ON) == 0
    gpu.reset()
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    raw = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(raw), 1) == 0          # hipStreamNonBlocking
    try:
        final = gpu.buffer(pairs)
        junk = gpu.buffer(n=n, fill=0x11)
        src = gpu.buffer(n=n, fill=0x22)
        cap = gpu.room(n)
        dst = gpu.buffer(n=cap, fill=0xA5)
        big = torch.empty(256 << 20, dtype=torch.uint8, device="cuda:0")
        big2 = torch.empty_like(big)
        torch.cuda.synchronize()
        # the side stream is kept busy, and the input is only there once that stream has got to its last copy
        for _ in range(4):
            assert hip.hipMemcpyAsync(big2.data_ptr(), big.data_ptr(), big.numel(), 3, raw) == 0
        assert hip.hipMemcpyAsync(src.data_ptr(), junk.data_ptr(), n * 12, 3, raw) == 0
        assert hip.hipMemcpyAsync(src.data_ptr(), final.data_ptr(), n * 12, 3, raw) == 0
        rc, got = gpu.call(gpu.addr(src), n, 1, gpu.addr(dst), cap, stream=raw)
        assert rc == 0, gpu.error()
        check(gpu.read(dst, 0, got), want)                              # (read on the default stream of torch, without a wait for `raw`)
        if cap > got:
            assert gpu.read(dst, got, cap - got).view(np.uint8).min() == 0xA5
    finally:
        torch.cuda.synchronize()
        hip.hipStreamDestroy(raw)


@pytest.mark.gpu
def test_gpu_engine_wrappers():
    """sdvpcmdecoder_amd.Engine: set_resample / reset_resample / audio_resample / resample_taps."""
    import torch
    from sdvpcmdecoder_amd import Engine
    pairs = BOUNDARY_CASES["rate_changes"]
    want = wanted(("bnd", "rate_changes"), pairs)
    eng = Engine(0)
    assert np.abs(np.array(eng.resample_taps(500)) - TABLE[500]).max() <= 1e-14
    d = torch.from_numpy(pairs.view(np.uint8).reshape(-1, 12).copy()).cuda()
    assert eng.audio_resample(d).cpu().numpy().tobytes() == pairs.tobytes()                     # the mode of a new engine is OFF
    eng.set_resample(ON)
    a = eng.audio_resample(d[:T + 100])
    assert eng.audio_resample_pending() == HALF
    b = eng.audio_resample(d[T + 100:], flush=True)
    assert eng.audio_resample_pending() == 0
    check(torch.cat([a, b]).cpu().numpy().view(PAIR_DTYPE).reshape(-1), want)
    out = torch.empty((len(want) + 100, 12), dtype=torch.uint8, device="cuda")
    got = eng.audio_resample(d, flush=True, out=out)
    assert got.data_ptr() == out.data_ptr()
    check(got.cpu().numpy().view(PAIR_DTYPE).reshape(-1), want)
    eng.audio_resample(d[:100])
    eng.reset_resample()
    assert eng.audio_resample_pending() == 0
    with pytest.raises(RuntimeError):
        eng.set_resample(7)
    with pytest.raises(RuntimeError):
        eng.audio_resample(d, out=d)
    assert eng.audio_resample(d[:0]).shape[0] == 0
    eng.close()


@pytest.mark.gpu
def test_gpu_decode_tape_wav_44100(tmp_path):
    """decode_tape wav ... [auto|force] 44100 on a three-frame synthetic STC-007 tape: the file equals `walk` over the pairs of the file the same
    program writes without the word, the header says 44 100 Hz; the forms without the word write what the engine's chain gives.
    "Equals" is the condition of this file, `check`: the count and the header bytewise, every PCM word within 1 LSB of the float64 walk and at most 2
    of them different.  The program's words are the device's sums, which add the same 128 products in double as the walk does but need not round the
    same way where y lies within about 1e-9 LSB of a half (the derivation in this module's docstring); a bytewise comparison would ask more than the definition fixes."""
    import torch
    from sdvpcmdecoder_amd import Engine, build as b, synth
    exe = b.build_example()
    luma = synth.stc007_frames(3, seed=12, noise_sigma=4.0)[0].copy()
    n, h, w = luma.shape
    (tmp_path / "luma.raw").write_bytes(np.ascontiguousarray(luma).tobytes())

    def tape(*words):
        out = subprocess.run([exe, "wav", str(tmp_path / "luma.raw"), str(w), str(h), str(n), str(tmp_path / "out.wav")] + list(words), capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr + out.stdout
        return (tmp_path / "out.wav").read_bytes()

    # the forms that worked before: the engine's own chain, stage by stage
    eng = Engine(0)
    eng.set_audio_masking(A.DROP_INTER_LIN_WORD)
    lines, _ = eng.binarize_frames(torch.from_numpy(luma).cuda(), first_frame_no=1, new_file=True, end_file=True)
    p, _ = eng.stitch_frames(lines)
    masked, pur, _ = eng.audio_process(p, stop=True)
    plain = eng.wav_files(masked, pur)[0]
    assert tape() == plain and tape("6") == plain
    pv = pur.cpu().numpy().view(A.PURGE_DTYPE).reshape(-1)
    k = int(np.nonzero(pv["kind"] == 1)[0][0])
    a0, a1 = int(pv["first_pair"][k]), int(pv["first_pair"][k + 1]) if k + 1 < len(pv) else masked.shape[0]
    eng.set_deemphasis(2)
    flat = eng.audio_deemphasis(masked[a0:a1])
    forced = eng.wav_header(a1 - a0, 44056) + eng.wav_pack(flat).cpu().numpy().tobytes()
    assert tape("force") == forced and tape("6", "force") == forced and forced != plain
    eng.close()
    assert plain[24:28] == (44056).to_bytes(4, "little") and len(plain) > 44 + 4 * 3 * 1400
    for words, base in ((("44100",), plain), (("6", "44100"), plain), (("force", "44100"), forced), (("6", "force", "44100"), forced)):
        got = tape(*words)
        src = np.zeros((len(base) - 44) // 4, dtype=PAIR_DTYPE)
        src["audio_word"] = np.frombuffer(base[44:], dtype="<i2").reshape(-1, 2)
        src["sample_rate"] = 44056
        want = wanted(("tape", base is plain), src)
        assert len(got) == 44 + 4 * len(want)
        hdr = C.create_string_buffer(44)
        lib = abi.bind(C.CDLL(b.build_hip()))
        lib.sdv_wav_header(hdr, len(want), 44100)
        assert got[:44] == hdr.raw and got[24:28] == (44100).to_bytes(4, "little")
        res = want.copy()
        res["audio_word"] = np.frombuffer(got[44:], dtype="<i2").reshape(-1, 2)
        check(res, want)
