"""sdv_encode_frames / sdv_encode_geometry / sdv_reset_encoder: interleaved 16-bit PCM -> STC-007 / PCM-F1 video frames on the device.

The expected bytes are encode_api.tape_words / tape_frames, numpy written from the header's text on top of the synth functions the real reference
decodes in the other suites; the comparison is bytewise and covers the whole destination buffer: the rows, the padding of every row, the bytes in
front of and behind the stated span (on the GPU also device_calls' guard).  Every body is written once against a memory of device_calls.py and
called by a test_emu_* / test_gpu_* pair (tests/test_twins.py)."""
import binascii
import ctypes as C

import numpy as np
import pytest

import device_calls as dc
import encode_api as en
import stitch_api as sa

STC007 = 2


def _engine(lib):
    eng = C.c_void_p(lib.sdv_engine_create(0))
    assert eng, lib.sdv_last_error(None)
    return eng


def _audio(rng, n_pairs, res=en.BIT16):
    pcm = rng.integers(-32768, 32768, size=(n_pairs, 2), dtype=np.int16)
    return pcm & ~3 if res == en.BIT14 else pcm         # (14 bit: what the truncation keeps)


# ---- 1. layout and edges ----------------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 15, 16, 17, 33, 137, 720)
N_COMBINATIONS = 224


def _window(kind, w):
    """inside the picture, touching its edges, reaching past both"""
    if kind == 0:
        return w // 4, max(w // 4 + 1, w - w // 4)
    if kind == 1:
        return 0, w
    return -(1 + w // 3), w + 2 + w // 5


def _layout_and_edges(lib, via):
    """A seeded sample of the cross product: width and (standard x resolution x control block x field order) cycle, so every pair of them occurs
    twice; the rest is drawn: window inside / on the edges / past both, top_line 0 / 3 / beyond the field (an all-black frame), heights 1, 2, 7,
    486, 2 (lpf + 1), 2 (lpf + 1) + 4, 1 or 2 frames, destination offset 0 / 3, row stride + 0 / 6, frame stride + 0 / 10, pcm offset 0 / 2
    bytes, n_pairs full / short / 0, levels, control bits and time code.  Every case is a tape of its own.  Then windows on either side of the width at which
    the raster changes its way."""
    rng = np.random.default_rng(2024)
    eng = _engine(lib)
    try:
        for i in range(N_COMBINATIONS):
            width = WIDTHS[i % 7]
            std, res, ctrl, order = (i // 7) & 1, (i // 14) & 1, (i // 28) & 1, (i // 56) & 1
            lpft = en.LPF[std] + ctrl
            height = int(rng.choice((1, 2, 7, 486, 2 * (en.LPF[std] + 1), 2 * (en.LPF[std] + 1) + 4)))
            start, stop = _window(int(rng.integers(0, 3)), width)
            top = int(rng.choice((0, 3, lpft + 5)))
            n = int(rng.choice((1, 2)))
            black = int(rng.integers(0, 255))
            flags = int(rng.integers(0, 4))
            tc = (int(rng.integers(0, 64)), int(rng.integers(0, 16)), int(rng.integers(0, 60)), int(rng.integers(0, 60)), int(rng.integers(0, en.FPS[std])))
            d = en.desc(std, res, ctrl, flags, order, black, int(rng.integers(black + 1, 256)), tc, width, height, start, stop, top)
            full = n * en.pairs_per_frame(std)
            assert en.geometry(lib, d) == (en.OK, en.pairs_per_frame(std), lpft, width)
            n_pairs = (full, int(rng.integers(1, full)), 0)[int(rng.integers(0, 3))]
            pcm = _audio(rng, full)
            want = en.tape_frames(en.tape_words(pcm[:n_pairs], n, std, res, ctrl, flags, tc), d)
            if top > lpft:
                assert (want == black).all()
            assert lib.sdv_reset_encoder(eng) == en.OK
            en.run_call(via, lib, eng, d, pcm, n_pairs, n, want, dst_off=int(rng.choice((0, 3))), dst_pad=int(rng.choice((0, 6))),
                        frame_pad=int(rng.choice((0, 10))), pcm_off=int(rng.choice((0, 2))))
        # windows of 66 .. 72 pixels, on either side of the width below which 16 pixels can show cells more than 31 apart and the raster reads its
        # pixels one by one (encode_engine.inc, `narrow`), inside the picture and across either edge of it
        pcm = _audio(rng, en.pairs_per_frame(en.NTSC))
        words = en.tape_words(pcm, 1)
        for span in range(66, 73):
            for start in (-3, 30, 137 - span + 5):
                d = en.desc(width=137, height=7, data_start=start, data_stop=start + span, top_line=120)
                assert lib.sdv_reset_encoder(eng) == en.OK
                en.run_call(via, lib, eng, d, pcm, len(pcm), 1, en.tape_frames(words, d), dst_off=int(rng.choice((0, 3))))
    finally:
        lib.sdv_engine_destroy(eng)


def test_emu_layout_and_edges(emu_lib):
    _layout_and_edges(en.emu(emu_lib), dc.HOST)


@pytest.mark.gpu
def test_gpu_layout_and_edges():
    _layout_and_edges(en.product(), dc.DEVICE)


# ---- 2. words ---------------------------------------------------------------------------------------------------------------------------------
def _poly_mod(v):
    """a polynomial over GF(2) modulo x^14 + x^8 + 1"""
    for bit in range(v.bit_length() - 1, 13, -1):
        if v >> bit & 1:
            v ^= (1 << 14 | 1 << 8 | 1) << (bit - 14)
    return v


def _poly_mul(a, b):
    r = 0
    for bit in range(b.bit_length()):
        if b >> bit & 1:
            r ^= a << bit
    return r


def _q(words):
    """x^6 L0 + x^5 R0 + ... + x R2 modulo x^14 + x^8 + 1, by polynomial arithmetic"""
    q = 0
    for k, w in enumerate(words):
        q ^= _poly_mod(_poly_mul(w, 1 << (6 - k)))
    return q


def _crc_of_words(words8):
    """CRC-16/CCITT-FALSE over the 112 bits of eight 14-bit words as 14 bytes, by binascii"""
    v = 0
    for w in words8:
        v = v << 14 | int(w)
    return binascii.crc_hqx(v.to_bytes(14, "big"), 0xFFFF)


def _words(lib, via):
    """Independent of the raster: width 137 x 4 with the window the whole row, so every cell is four pixels; the cells are read back from the bytes
    and checked against known answers - the CRC of every line by binascii (check value 0x29B1 for "123456789"), 0xA96A on silent lines, P and Q on the
    all-ones and the one-bit blocks by polynomial arithmetic, the 16-bit P and S words, the control words and a time code that crosses a second
    and a minute (1:07:59 and 58 / 48 fields, three frames)."""
    assert binascii.crc_hqx(b"123456789", 0xFFFF) == 0x29B1
    assert (_q([0x3FFF] * 6), _q([1, 0, 0, 0, 0, 0]), _q([0, 0, 0, 0, 0, 1]), _q([0x2000, 0, 0, 0, 0, 0]), _q([0, 0, 0, 0x2000, 0, 0])) == (0x2A00, 0x40, 0x02, 0x2020, 0x0404)
    eng = _engine(lib)
    rng = np.random.default_rng(5)
    try:
        for std in (en.NTSC, en.PAL):
            lpf, fps = en.LPF[std], en.FPS[std]
            tc = (9, 1, 7, 59, fps - 2)
            d = en.desc(std, en.BIT14, 1, en.COPY_PROHIBITED, en.TFF, 20, 220, tc, 137 * 4, 2 * (lpf + 1), 0, 137 * 4, 0)
            # blocks with known answers in random audio; frames 1 and 2 are silent
            blocks = (_audio(rng, lpf * 6, en.BIT14).reshape(-1, 6).view(np.uint16) >> 2).astype(np.uint32)
            known = {200: [0x3FFF] * 6, 230: [1, 0, 0, 0, 0, 0], 231: [0, 0, 0, 0, 0, 1], 232: [0x2000, 0, 0, 0, 0, 0], 233: [0, 0, 0, 0x2000, 0, 0]}
            for b, w in known.items():
                blocks[b] = w
            pcm = (blocks << 2).astype(np.uint16).view(np.int16).reshape(-1, 2)
            buf = en.run_call(via, lib, eng, d, pcm, len(pcm), 3, en.tape_frames(en.tape_words(pcm, 3, std, en.BIT14, 1, en.COPY_PROHIBITED, tc), d))
            frames = en.frames_of(buf, d, 3)
            words, ok = en.words_of(en.cells_of(frames, 220))           # [frame][row][9]
            assert ok.all()
            fields = np.stack([words[:, 0::2], words[:, 1::2]], axis=1).reshape(6, lpf + 1, 9)         # [field][line of the field][9]
            for line in fields.reshape(-1, 9):
                assert _crc_of_words(line[:8]) == line[8]
            # the control lines: 1:07:59.58, .59, 1:08:00.00, .01, .02, .03 (PAL: .48, .49, ...)
            times = [(1, 7, 59, fps - 2), (1, 7, 59, fps - 1), (1, 8, 0, 0), (1, 8, 0, 1), (1, 8, 0, 2), (1, 8, 0, 3)]
            for f, (hour, minute, second, field) in enumerate(times):
                assert fields[f, 0, :8].tolist() == [0x3333, 0x0CCC, 0x3333, 0x0CCC, 0, 9 << 8 | hour << 4 | minute >> 2, (minute & 3) << 12 | second << 6 | field, 8 | 1]
            data = fields[:, 1:].reshape(6 * lpf, 9)                    # data line M of the tape
            for b, w in known.items():
                full = list(w) + [w[0] ^ w[1] ^ w[2] ^ w[3] ^ w[4] ^ w[5], _q(w)]
                assert [int(data[b + 16 * k, k]) for k in range(8)] == full, b
            assert data[200 + 96, 6] == 0 and data[200 + 112, 7] == 0x2A00 and data[230 + 112, 7] == 0x40 and data[232 + 96, 6] == 0x2000
            silent = data[2 * lpf + 112:]                               # behind the delay of the last block with audio
            assert len(silent) > lpf and (silent[:, :8] == 0).all() and (silent[:, 8] == 0xA96A).all()
            assert (data[:16, 1:8] == 0).all() and (data[:112, 7] == 0).all()        # in front of the tape
            # 16 bit: slot k carries the upper 14 bits, slot 7 the low two of the seven words of its line at shift 12 - 2 k; P16 is the XOR
            assert lib.sdv_reset_encoder(eng) == en.OK
            d16 = en.desc(std, en.BIT16, 0, 0, en.TFF, 20, 220, tc, 137 * 4, 2 * lpf, 0, 137 * 4, 0)
            pcm16 = np.zeros((lpf * 6, 2), dtype=np.int16)
            pcm16.reshape(-1, 6)[100] = [0x0003, 0x0002, 0x0001, 0x0000, 0x0003, 0x7FFC]
            buf = en.run_call(via, lib, eng, d16, pcm16, len(pcm16), 1, en.tape_frames(en.tape_words(pcm16, 1, std, en.BIT16), d16))
            words, ok = en.words_of(en.cells_of(en.frames_of(buf, d16, 1), 220))
            data = np.concatenate([words[0, 0::2], words[0, 1::2]])
            assert ok.all() and [int(data[100 + 16 * k, 7]) for k in range(7)] == [3 << 12, 2 << 10, 1 << 8, 0, 3 << 4, 0, 3]      # P16 = 0x7FFF
            assert [int(data[100 + 16 * k, k]) for k in range(7)] == [0, 0, 0, 0, 0, 0x1FFF, 0x1FFF]
            assert lib.sdv_reset_encoder(eng) == en.OK
    finally:
        lib.sdv_engine_destroy(eng)


def test_emu_words(emu_lib):
    _words(en.emu(emu_lib), dc.HOST)


@pytest.mark.gpu
def test_gpu_words():
    _words(en.product(), dc.DEVICE)


# ---- 3. streaming -----------------------------------------------------------------------------------------------------------------------------
def _streaming(lib, via):
    """5 frames in one call equal calls of 1, 2, 0 and 2 frames, whose geometry, levels and control bits differ from call to call; the last call has
    fewer pairs than it consumes.  sdv_reset_encoder between two tapes gives the first tape's bytes again.  A changed standard, resolution or
    control block without a reset is refused, writes nothing and leaves the tape where it was."""
    rng = np.random.default_rng(9)
    eng = _engine(lib)
    std, res, tc = en.NTSC, en.BIT14, (3, 15, 59, 59, 47)
    ppf = en.pairs_per_frame(std)
    pcm = _audio(rng, 5 * ppf - 700)
    one = en.desc(std, res, 1, en.EMPHASIS, en.TFF, 30, 200, tc, 97, 30, 3, 95, 0)
    calls = [(1, one, en.EMPHASIS), (2, en.desc(std, res, 1, 0, en.BFF, 10, 90, (4, 0, 0, 0, 0), 137, 12, -4, 140, 240), 0), (0, one, en.EMPHASIS),
             (2, en.desc(std, res, 1, en.COPY_PROHIBITED, en.TFF, 30, 200, tc, 33, 2 * 246, 0, 33, 0), en.COPY_PROHIBITED)]
    try:
        for tape in range(2):
            w_one = en.tape_words(pcm, 5, std, res, 1, en.EMPHASIS, tc)
            en.run_call(via, lib, eng, one, pcm, len(pcm), 5, en.tape_frames(w_one, one), dst_off=1)
            assert lib.sdv_reset_encoder(eng) == en.OK
        # the same tape in calls: the control bits are each call's own, the time code runs on (tc_index comes with every call: the second call's is 4)
        for tape in range(2):
            done = 0
            for n, d, flags in calls:
                w = en.tape_words(pcm, 5, std, res, 1, flags, (d.tc_index,) + tc[1:])
                left = pcm[done * ppf:]
                en.run_call(via, lib, eng, d, left, len(left), n, en.tape_frames(w, d, range(done, done + n)), dst_pad=6)
                done += n
            assert done == 5
            if tape == 0:
                assert lib.sdv_reset_encoder(eng) == en.OK
        # a tape stays what it is: refused, nothing written, and the sixth frame follows the fifth
        for other in (en.desc(en.PAL, res, 1, 0, en.TFF, 30, 200, tc, 97, 30, 3, 95, 0), en.desc(std, en.BIT16, 1, 0, en.TFF, 30, 200, tc, 97, 30, 3, 95, 0),
                      en.desc(std, res, 0, 0, en.TFF, 30, 200, tc, 97, 30, 3, 95, 0)):
            en.run_call(via, lib, eng, other, pcm, len(pcm), 1, None, expect_rc=en.BAD_ARG)
            assert b"sdv_reset_encoder" in lib.sdv_last_error(eng)
        tail = _audio(rng, 100)
        whole = np.concatenate([pcm, np.zeros((700, 2), dtype=np.int16), tail])
        en.run_call(via, lib, eng, one, tail, len(tail), 1, en.tape_frames(en.tape_words(whole, 6, std, res, 1, en.EMPHASIS, tc), one, range(5, 6)))
    finally:
        lib.sdv_engine_destroy(eng)


def test_emu_streaming(emu_lib):
    _streaming(en.emu(emu_lib), dc.HOST)


@pytest.mark.gpu
def test_gpu_streaming():
    _streaming(en.product(), dc.DEVICE)


# ---- 4. round trip ----------------------------------------------------------------------------------------------------------------------------
ROUND_TRIPS = {"ntsc_14bit_ctrl": (en.NTSC, en.BIT14, 1, 492, 0), "pal_16bit_ctrl": (en.PAL, en.BIT16, 1, 590, 0), "ntsc_16bit_top2": (en.NTSC, en.BIT16, 0, 486, 2)}


def _round_trip(lib, via, oracle_lib, case):
    """2 frames of seeded random audio (14 bit: the two low bits cleared) and one frame with no pairs, encoded into a buffer that goes to
    sdv_decode_frames(NEW_FILE | END_FILE) as it lies in the memory of the call - on the GPU nothing comes back in between: every source pair comes
    back in order behind the lead-in with SDV_SF_BLOCK_OK | SDV_SF_WORD_VALID on both channels, no frame drops a block, the resolution of the full
    frames is the encoded one, and the frame descriptors equal bytewise, ctrl_* included, what the oracle's two workers make of the frames."""
    from oracle_run import oracle_binarize
    std, res, ctrl, height, top = ROUND_TRIPS[case]
    rng = np.random.default_rng(77)
    tc = (2, 1, 2, 59, en.FPS[std] - 2)
    d = en.desc(std, res, ctrl, 0, en.TFF, 30, 200, tc, 720, height, 12, 708, top)
    n = 3
    pcm = _audio(rng, 2 * en.pairs_per_frame(std), res)
    want = en.tape_frames(en.tape_words(pcm, n, std, res, ctrl, 0, tc), d)
    eng = _engine(lib)
    try:
        dbuf = via.array(np.full(want.size, en.FILL, dtype=np.uint8))
        sbuf = via.array(pcm)
        assert lib.sdv_encode_frames(eng, C.byref(d), via.ptr(sbuf), len(pcm), n, via.ptr(dbuf), 720, 720 * height, via.stream()) == en.OK, lib.sdv_last_error(eng)
        lib.sdv_set_pcm_type(eng, STC007, 0)
        cap = (n + 2) * 2100 + 8192
        pairs, frames = via.zeros(cap, sa.PAIR_DTYPE), via.zeros(n + 16, sa.FRASM_DTYPE)
        n_pairs, n_frames = C.c_size_t(0), C.c_size_t(0)
        rc = lib.sdv_decode_frames(eng, STC007, via.ptr(dbuf), 720, 720 * height, 720, height, n, 1, 1 | 4, via.ptr(pairs), cap, C.byref(n_pairs),
                                   via.ptr(frames), len(frames), C.byref(n_frames), None, 0, 0, 0, None, 0, None, None, via.stream())
        assert rc == 0, lib.sdv_last_error(eng)
        got_p, got_f = via.get(pairs, n_pairs.value), via.get(frames, n_frames.value)
        assert np.array_equal(via.get(dbuf), want.reshape(-1))
    finally:
        lib.sdv_engine_destroy(eng)
    audio = got_p[got_p["service_type"] == 0]
    first = next((k for k in range(len(audio) - len(pcm) + 1) if np.array_equal(audio["audio_word"][k:k + 8], pcm[:8])), None)
    assert first is not None and first < 2 * 112 * 3
    assert np.array_equal(audio["audio_word"][first:first + len(pcm)], pcm)
    assert ((audio["sample_flags"][first:first + len(pcm)] & 3) == 3).all()           # SDV_SF_BLOCK_OK | SDV_SF_WORD_VALID
    assert (got_f["blocks_drop"] == 0).all()
    full = got_f[np.isin(got_f["frame_number"], (1, 2)) & (got_f["service_type"] == 0)]
    res_mode = 3 if res == en.BIT16 else 0                                                # SDV_RES_MODE_16BIT / _14BIT
    assert len(full) == 2 and (full["odd_resolution"] == res_mode).all() and (full["even_resolution"] == res_mode).all()
    recs, _ = oracle_binarize(want, mode=2, first_frame_no=1, new_file=True, end_file=True)
    _, want_f = sa.run_cpu(oracle_lib, "orc_", recs, sa.default_settings())
    assert got_f.tobytes() == want_f.tobytes()
    if ctrl:
        assert (int(full["ctrl_index"][1]), int(full["ctrl_hour"][1]), int(full["ctrl_minute"][1]), int(full["ctrl_second"][1])) == (2, 1, 3, 0)


@pytest.mark.parametrize("case", sorted(ROUND_TRIPS))
def test_emu_round_trip(case, emu_lib, oracle_lib):
    _round_trip(en.emu(emu_lib), dc.HOST, oracle_lib, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(ROUND_TRIPS))
def test_gpu_round_trip(case, oracle_lib):
    _round_trip(en.product(), dc.DEVICE, oracle_lib, case)


# ---- 5. more than one trip --------------------------------------------------------------------------------------------------------------------
def _more_than_one_trip(lib, via):
    """1000 frames of 137 x 54 at a destination 3 bytes off: 1000 x 54 x 10 chunk slots, more than the 2048 x 256 threads of the product's launch, so
    its threads take a second trip with the stride split into frames, rows and slots for that launch size (the emulator build walks every case
    with a few threads)."""
    rng = np.random.default_rng(13)
    n, d = 1000, en.desc(en.NTSC, en.BIT14, 0, 0, en.TFF, 16, 235, (0, 0, 0, 0, 0), 137, 54, 0, 137, 100)
    assert n * 54 * ((137 + 30) // 16) > 2048 * 256
    pcm = _audio(rng, n * en.pairs_per_frame(en.NTSC))
    eng = _engine(lib)
    try:
        en.run_call(via, lib, eng, d, pcm, len(pcm), n, en.tape_frames(en.tape_words(pcm, n), d), dst_off=3)
    finally:
        lib.sdv_engine_destroy(eng)


def test_emu_more_than_one_trip(emu_lib):
    _more_than_one_trip(en.emu(emu_lib), dc.HOST)


@pytest.mark.gpu
def test_gpu_more_than_one_trip():
    _more_than_one_trip(en.product(), dc.DEVICE)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
def _refusals(lib, via):
    """Host checks ahead of any launch: the code, a reason in sdv_last_error, the destination untouched, the tape where it was - the good call
    behind every refusal writes the next frame of one tape.  sdv_encode_geometry gives the same code for the same descriptor."""
    rng = np.random.default_rng(17)
    eng = _engine(lib)
    w, h, n = 40, 6, 2
    ppf = en.pairs_per_frame(en.NTSC)
    pcm = _audio(rng, 40 * ppf)
    base = dict(std=en.NTSC, res=en.BIT14, ctrl=1, ctrl_flags=0, order=en.TFF, black=30, white=200, tc=(1, 2, 3, 4, 5), width=w, height=h, data_start=2, data_stop=38, top_line=0)
    good = en.desc(**base)
    tape = en.tape_frames(en.tape_words(pcm, 40, en.NTSC, en.BIT14, 1, 0, base["tc"]), good)
    src = via.array(pcm)
    dst = via.array(np.full(4096, en.FILL, dtype=np.uint8))
    sp, dp = via.ptr(src), via.ptr(dst)
    d_span = n * h * w
    NULL = object()
    done = [0]

    def call(d=None, s=sp, pairs=n * ppf, frames=n, t=dp, drs=w, dfs=h * w, **kw):
        d = en.desc(**dict(base, **kw)) if d is None else d
        return lib.sdv_encode_frames(eng, None if d is NULL else C.byref(d), s, pairs, frames, t, drs, dfs, via.stream())

    def refused(code, geo=False, **kw):
        assert call(**kw) == code, kw
        assert lib.sdv_last_error(eng), kw
        assert (via.get(dst) == en.FILL).all(), kw
        if kw.get("d") is not NULL:         # the descriptor alone: refused for the same reason, or nothing wrong with it
            d = en.desc(**dict(base, **{k: v for k, v in kw.items() if k in base}))
            assert lib.sdv_encode_geometry(C.byref(d), None, None, None) == (code if geo else en.OK), kw
        out = via.array(np.full(h * w + en.TAIL, en.FILL, dtype=np.uint8))            # ... and the engine takes the next call, on the same tape
        assert lib.sdv_encode_frames(eng, C.byref(good), via.ptr(src, 2 * ppf * done[0]), ppf, 1, via.ptr(out), w, h * w, via.stream()) == en.OK
        got = via.get(out)
        assert np.array_equal(got[:h * w], tape[done[0]].reshape(-1)) and (got[h * w:] == en.FILL).all(), kw
        done[0] += 1
    try:
        # null pointers
        refused(en.BAD_ARG, d=NULL)
        assert lib.sdv_encode_geometry(None, None, None, None) == en.BAD_ARG
        refused(en.NULL_PCM, s=None)
        refused(en.NULL_VIDEO, t=None)
        # unknown enum values and control bits (the P word cannot be left out)
        refused(en.BAD_ARG, geo=True, std=2)
        refused(en.BAD_ARG, geo=True, res=2)
        refused(en.BAD_ARG, geo=True, ctrl=2)
        refused(en.BAD_ARG, geo=True, order=2)
        refused(en.BAD_ARG, geo=True, ctrl_flags=4)
        # sizes, window, levels
        refused(en.BAD_ARG, frames=-1)
        for bad in (0, -3, 32769):
            refused(en.BAD_ARG, geo=True, width=bad)
            refused(en.BAD_ARG, geo=True, height=bad)
        refused(en.BAD_ARG, geo=True, data_stop=2)
        refused(en.BAD_ARG, geo=True, data_start=20, data_stop=10)
        refused(en.BAD_ARG, geo=True, white=30)
        refused(en.BAD_ARG, geo=True, black=100, white=99)
        # time code
        for tc in ((64, 0, 0, 0, 0), (0, 16, 0, 0, 0), (0, 0, 60, 0, 0), (0, 0, 0, 60, 0), (0, 0, 0, 0, 60)):
            refused(en.BAD_ARG, geo=True, tc=tc)
        refused(en.BAD_ARG, geo=True, std=en.PAL, tc=(0, 0, 0, 0, 50))
        # strides
        refused(en.BAD_ARG, drs=w - 1)
        refused(en.BAD_ARG, dfs=h * w - 1)
        refused(en.BAD_ARG, drs=(1 << 32) + 1)
        refused(en.BAD_ARG, dfs=(1 << 32) + 1)
        # overlap: the destination's first byte on the last byte of the pairs the call reads, and its last byte on their first one
        refused(en.BAD_ARG, s=dp + 1024, t=dp + 1024 + 4 * n * ppf - 1)
        refused(en.BAD_ARG, s=dp + 1024, t=dp + 1024 - d_span + 1)
        refused(en.BAD_ARG, s=dp, t=dp)
        assert done[0] > 30
        # no frames ask nothing at all; no pairs ask no pcm; one frame asks nothing of the frame stride; pairs the call does not read may lie anywhere
        assert call(frames=0, s=None, t=None, d=NULL) == en.OK and (via.get(dst) == en.FILL).all()
        assert lib.sdv_reset_encoder(eng) == en.OK and lib.sdv_reset_encoder(None) == en.BAD_ARG
        assert call(frames=1, s=None, pairs=0, dfs=0, t=dp + 2048) == en.OK
        got = via.get(dst)
        silent = en.tape_frames(en.tape_words(pcm[:0], 1, en.NTSC, en.BIT14, 1, 0, base["tc"]), good)
        assert np.array_equal(got[2048:2048 + h * w], silent.reshape(-1)) and (got[:2048] == en.FILL).all() and (got[2048 + h * w:] == en.FILL).all()
    finally:
        lib.sdv_engine_destroy(eng)


def test_emu_refusals(emu_lib):
    _refusals(en.emu(emu_lib), dc.HOST)


@pytest.mark.gpu
def test_gpu_refusals():
    _refusals(en.product(), dc.DEVICE)


# ---- 7. the library ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_of_the_product_library():
    from sdvpcmdecoder_amd import build as b
    lib = en.bind(C.CDLL(b.build_hip()))
    assert hasattr(lib, "sdv_encode_geometry") and hasattr(lib, "sdv_encode_frames") and hasattr(lib, "sdv_reset_encoder")
    assert lib.sdv_abi_version() >= 9
    # the geometry needs neither an engine nor a device
    assert en.geometry(lib, en.desc(en.NTSC, ctrl=1)) == (0, 1470, 246, 720)
    assert en.geometry(lib, en.desc(en.PAL, en.BIT16, width=640)) == (0, 1764, 294, 640)


@pytest.mark.gpu
def test_gpu_engine_wrapper_round_trip():
    """Engine.encode_frames: torch tensors in, an (n, height, width) uint8 tensor out on torch's current stream, which Engine.decode_frames takes
    as it is; a tape in two calls and Engine.reset_encoder."""
    import torch
    from sdvpcmdecoder_amd import Engine
    rng = np.random.default_rng(31)
    pcm = _audio(rng, 2 * 1470, en.BIT14)
    want = en.tape_frames(en.tape_words(pcm, 3, ctrl=1), en.desc(ctrl=1, height=492))
    eng = Engine(0)
    t = torch.from_numpy(pcm).cuda()
    a = eng.encode_frames(t[:1470], 1, ctrl_block=True, height=492)
    b = eng.encode_frames(t[1470:], 2, ctrl_block=True, height=492)
    got = torch.cat([a, b])
    assert got.shape == (3, 492, 720) and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    eng.reset_encoder()
    assert np.array_equal(eng.encode_frames(t, 3, ctrl_block=True, height=492).cpu().numpy(), want)
    eng.setPCMType(STC007)
    pairs, frames, _ = eng.decode_frames(STC007, got, first_frame_no=1, new_file=True, end_file=True)
    p = pairs.cpu().numpy().view(sa.PAIR_DTYPE).reshape(-1)
    audio = p[p["service_type"] == 0]["audio_word"]
    first = next(k for k in range(len(audio)) if np.array_equal(audio[k:k + 8], pcm[:8]))
    assert np.array_equal(audio[first:first + len(pcm)], pcm)
    with pytest.raises(RuntimeError, match="sdv_reset_encoder"):
        eng.encode_frames(t, 1, standard="pal")


@pytest.mark.gpu
def test_gpu_cpp_host_program_encodes_and_decodes(tmp_path):
    """decode_tape encode in.wav out.luma, then decode_tape wav out.luma: the WAV that comes back holds the samples of the WAV that went in,
    behind the decoder's lead-in."""
    import subprocess
    from sdvpcmdecoder_amd import build as b
    exe = b.build_example()
    rng = np.random.default_rng(29)
    pcm = _audio(rng, 2 * 1470 + 321, en.BIT14)
    hdr = b"RIFF" + (36 + pcm.nbytes).to_bytes(4, "little") + b"WAVEfmt " + (16).to_bytes(4, "little") + (1).to_bytes(2, "little") + (2).to_bytes(2, "little") + \
        (44056).to_bytes(4, "little") + (44056 * 4).to_bytes(4, "little") + (4).to_bytes(2, "little") + (16).to_bytes(2, "little") + b"data" + pcm.nbytes.to_bytes(4, "little")
    (tmp_path / "in.wav").write_bytes(hdr + pcm.tobytes())
    out = subprocess.run([exe, "encode", str(tmp_path / "in.wav"), str(tmp_path / "tape.luma")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    n, width, height = (int(x) for x in out.stdout.split()[:3])
    assert (n, width, height) == (4, 720, 492) and (tmp_path / "tape.luma").stat().st_size == n * width * height
    want = en.tape_frames(en.tape_words(pcm, n, ctrl=1), en.desc(ctrl=1, height=492))
    assert (tmp_path / "tape.luma").read_bytes() == want.tobytes()
    out = subprocess.run([exe, "wav", str(tmp_path / "tape.luma"), str(width), str(height), str(n), str(tmp_path / "back.wav")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    back = np.frombuffer((tmp_path / "back.wav").read_bytes()[44:], dtype=np.int16).reshape(-1, 2)
    first = next(k for k in range(len(back)) if np.array_equal(back[k:k + 8], pcm[:8]))
    assert np.array_equal(back[first:first + len(pcm)], pcm)
