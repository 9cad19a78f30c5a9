"""sdv_encode_markerless_frames / sdv_encode_markerless_geometry: interleaved 16-bit PCM -> Sony PCM-1 and PCM-16x0 (SI, EI) video frames on the device.

The expected bytes are encode_markerless_api.tape_bits / tape_frames, numpy written from the header's text on top of the synth functions the real
reference decodes in the other suites; the comparison is bytewise and covers the whole destination buffer: the rows, the padding of every row, the
bytes in front of and behind the stated span (on the GPU also device_calls' guard).  Every body is written once against a memory of device_calls.py
and called by a test_emu_* / test_gpu_* pair (tests/test_twins.py)."""
import binascii
import ctypes as C

import numpy as np
import pytest

import device_calls as dc
import encode_api as en
import encode_markerless_api as ml
import pcm1_api as p1
import pcm16_api as p16
from stitch_api import PAIR_DTYPE
from sdvpcmdecoder_amd.abi import PCM_PCM1 as PCM1_TYPE, PCM_PCM16X0 as PCM16X0_TYPE

FORMATS = (ml.PCM1, ml.SI, ml.EI)
EDGES = (-32768, -8193, -8192, -1, 0, 8191, 8192, 32767)        # either side of the PCM-1 companding ranges, and the ends


def _engine(lib):
    eng = C.c_void_p(lib.sdv_engine_create(0))
    assert eng, lib.sdv_last_error(None)
    return eng


def _audio(rng, n_pairs):
    pcm = rng.integers(-32768, 32768, size=(n_pairs, 2), dtype=np.int16)
    pcm[::3] >>= 3              # a third of the pairs inside the fine range of PCM-1
    return pcm


# ---- 1. layout and edges ----------------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 15, 16, 17, 33, 94, 193, 720)
N_COMBINATIONS = 192


def _window(kind, w):
    """inside the picture, touching its edges, reaching past both"""
    if kind == 0:
        return w // 4, max(w // 4 + 1, w - w // 4)
    if kind == 1:
        return 0, w
    return -(1 + w // 3), w + 2 + w // 5


def _narrow_spans(cells):
    """the spans on either side of the one at which the host's rule, (15 * CELLS) / span + 2 > 31, changes: three below, three from it on"""
    first_wide = next(s for s in range(1, 1000) if (15 * cells) // s + 2 <= 31)
    return range(first_wide - 3, first_wide + 3)


assert list(_narrow_spans(193)) == list(range(94, 100)) and list(_narrow_spans(94)) == list(range(45, 51))


def _layout_and_edges(lib, via):
    """A seeded sample of the cross product: width and (format x field order) cycle, so every pair of them occurs four times; the rest is drawn: window
    inside / on the edges / past both, top_line 0 / 3 / -2 / beyond the field (an all-black frame), heights 1, 2, 7, 490, 2 (245 + header) + 4, 0 / 1 / 8
    header lines (PCM-1), 1 or 2 frames, destination offset 0 / 3, row stride + 0 / 6, frame stride + 0 / 10, pcm offset 0 / 2 bytes, n_pairs full /
    short / 0, levels and control flags.  Then windows on either side of the span at which the raster changes its way."""
    rng = np.random.default_rng(2025)
    eng = _engine(lib)
    try:
        for i in range(N_COMBINATIONS):
            width = WIDTHS[i % 8]
            fmt, order = FORMATS[(i // 8) % 3], (i // 24) & 1
            header = int(rng.choice((0, 1, 8))) if fmt == ml.PCM1 else 0
            lpft = ml.LINES + header
            height = int(rng.choice((1, 2, 7, 490, 2 * lpft + 4)))
            start, stop = _window(int(rng.integers(0, 3)), width)
            top = int(rng.choice((0, 3, -2, lpft + 5)))
            n = int(rng.choice((1, 2)))
            black = int(rng.integers(0, 255))
            flags = int(rng.integers(0, 8)) if fmt != ml.PCM1 else 0
            d = ml.desc(fmt, order, black, int(rng.integers(black + 1, 256)), header, flags, width, height, start, stop, top)
            full = n * ml.PAIRS_PER_FRAME
            assert ml.geometry(lib, d) == (ml.OK, ml.PAIRS_PER_FRAME, lpft, width)
            n_pairs = (full, int(rng.integers(1, full)), 0)[int(rng.integers(0, 3))]
            pcm = _audio(rng, full)
            want = ml.tape_frames(pcm[:n_pairs], n, d)
            if top > lpft:
                assert (want == black).all()
            ml.run_call(via, lib, eng, d, pcm, n_pairs, n, want, dst_off=int(rng.choice((0, 3))), dst_pad=int(rng.choice((0, 6))),
                        frame_pad=int(rng.choice((0, 10))), pcm_off=int(rng.choice((0, 2))))
        # windows on either side of the span below which 16 pixels can show cells more than 31 apart and the raster reads its pixels one by one
        # (encode_engine.inc, `narrow`), inside the picture and across either edge of it
        pcm = _audio(rng, ml.PAIRS_PER_FRAME)
        for fmt in FORMATS:
            cells = ml.CELLS[fmt]
            bits = ml.tape_bits(pcm, 1, fmt)
            for span in _narrow_spans(cells):
                for start in (-3, 30, cells - span + 5):
                    d = ml.desc(fmt, width=cells, height=7, data_start=start, data_stop=start + span, top_line=120)
                    ml.run_call(via, lib, eng, d, pcm, len(pcm), 1, ml.frames_of_bits(bits, d), dst_off=int(rng.choice((0, 3))))
    finally:
        lib.sdv_engine_destroy(eng)


def test_emu_layout_and_edges(emu_lib):
    _layout_and_edges(ml.emu(emu_lib), dc.HOST)


@pytest.mark.gpu
def test_gpu_layout_and_edges():
    _layout_and_edges(ml.product(), dc.DEVICE)


# ---- 2. words ---------------------------------------------------------------------------------------------------------------------------------
def _crc_ccitt(value, n_bits):
    """CRC-16/CCITT-FALSE over n_bits bits (a multiple of 8 after padding is not needed: bit by bit)"""
    crc = 0xFFFF
    for bit in range(n_bits - 1, -1, -1):
        top = ((crc >> 15) ^ (value >> bit)) & 1
        crc = ((crc << 1) & 0xFFFF) ^ (0x1021 if top else 0)
    return crc


def _pcm1_pair_of(u):
    """the direction of oracle/pcm1.c: the pair of a field on its sub-line u (the formula of the header solved for the pair, by search)"""
    for n in range(735):
        itl, p = divmod(n, 92)
        if 92 * itl + (0 if (itl % 2 == 0) == ((p & 1) == 1) else 46) + (p >> 1) == u:
            return n
    raise AssertionError(u)


def _words_pcm1(lib, via):
    """Independent of the raster: width 94 x 4 with the window the whole row, so every cell is four pixels; the cells are read back from the bytes.
    Every word is the companded sample at the place the interleave says - the read-back words are deinterleaved with the formula and compared with
    s & ~3 / s & ~15 -, every line's CRC is CRC-16/CCITT-FALSE over the inverted words, inverted (bit by bit here; check value 0x29B1 by binascii),
    the Header lines are the constant, and behind n_pairs the words are 0x1000 and the CRC 0xECBF."""
    assert binascii.crc_hqx(b"123456789", 0xFFFF) == 0x29B1 and _crc_ccitt(int.from_bytes(b"123456789", "big"), 72) == 0x29B1
    rng = np.random.default_rng(6)
    eng = _engine(lib)
    header, n = 2, 2
    pcm = _audio(rng, ml.PAIRS_PER_FRAME + 400)           # frame 1 runs out of pairs
    pcm[5:5 + len(EDGES), 0] = EDGES
    pcm[900:900 + len(EDGES), 1] = EDGES[::-1]
    d = ml.desc(ml.PCM1, ml.TFF, 20, 220, header, 0, 94 * 4, 2 * (ml.LINES + header), 0, 94 * 4, 0)
    try:
        buf = ml.run_call(via, lib, eng, d, pcm, len(pcm), n, ml.tape_frames(pcm, n, d))
    finally:
        lib.sdv_engine_destroy(eng)
    cells = ml.fields_of(ml.cells_of(ml.frames_of(buf, d, n), 220, 94))         # [field][line][94]
    words = ml.bits_value(cells[..., :78].reshape(cells.shape[:-1] + (6, 13)))
    crc = ml.bits_value(cells[..., 78:])
    assert (words[:, :header] == ml.HEADER_WORDS[:6]).all() and (crc[:, :header] == 0xCCCC).all()
    words, crc = words[:, header:], crc[:, header:]
    for f in range(2 * n):
        for j in range(ml.LINES):
            v = 0
            for w in words[f, j]:
                v = v << 13 | (~int(w) & 0x1FFF)
            assert (~_crc_ccitt(v, 78)) & 0xFFFF == crc[f, j], (f, j)
    sub = words.reshape(2 * n, 735, 2)                                          # [field][sub-line][L R]
    pair_of = np.array([_pcm1_pair_of(u) for u in range(735)])
    back = np.zeros_like(sub)
    back[:, pair_of] = sub                                                      # [field][pair of the field]
    back = back.reshape(-1, 2).astype(np.int64)
    # a word back to a sample: the range bit says which 12 bits it holds
    fine = (back & 0x1000) != 0
    val = np.where(fine, ((back & 0xFFF) ^ 0x800) - 0x800 << 2, ((back & 0xFFF) ^ 0x800) - 0x800 << 4)
    src = np.zeros((n * ml.PAIRS_PER_FRAME, 2), dtype=np.int16)
    src[:len(pcm)] = pcm
    want = np.where((src >= -8192) & (src < 8192), src & ~3, src & ~15)
    assert np.array_equal(val, want)
    assert np.array_equal(want, ml.pcm1_kept(src))
    assert (back[len(pcm):] == 0x1000).all()
    # a line all of whose pairs lie behind n_pairs: sub-lines 3 j .. 3 j + 2 of the last field
    silent = [j for j in range(ml.LINES) if all(3 * ml.FIELD_PAIRS + pair_of[3 * j + q] >= len(pcm) for q in range(3))]
    assert len(silent) > 100 and (crc[3, silent] == 0xECBF).all() and (words[3, silent] == 0x1000).all()


def test_emu_words_pcm1(emu_lib):
    _words_pcm1(ml.emu(emu_lib), dc.HOST)


@pytest.mark.gpu
def test_gpu_words_pcm1():
    _words_pcm1(ml.product(), dc.DEVICE)


def _words_pcm16(lib, via):
    """Width 193 x 4 with the window the whole row: the words read back from the pixels equal synth.pcm16x0_encode_fields for SI and EI, the middle
    role carries L ^ R of the pair its neighbours carry, the three CRCs of every line are right, and the Control Bit column is the header's for all 16
    combinations of the three flags and the interleave."""
    from sdvpcmdecoder_amd import synth
    rng = np.random.default_rng(8)
    eng = _engine(lib)
    n = 2
    pcm = _audio(rng, n * ml.PAIRS_PER_FRAME)
    pcm[7:7 + len(EDGES), 1] = EDGES
    try:
        for fmt in (ml.SI, ml.EI):
            for flags in range(8):
                frames = n if flags == 5 else 1
                d = ml.desc(fmt, ml.TFF, 20, 220, 0, flags, 193 * 4, 2 * ml.LINES, 0, 193 * 4, 0)
                buf = ml.run_call(via, lib, eng, d, pcm, len(pcm), frames, ml.tape_frames(pcm, frames, d))
                cells = ml.fields_of(ml.cells_of(ml.frames_of(buf, d, frames), 220, 193))          # [field][line][193]
                want_ctrl = np.ones(ml.LINES, dtype=np.uint32)
                for i in range(7):
                    want_ctrl[35 * i:35 * i + 4] = [0 if flags & 1 else 1, 0 if flags & 2 else 1, 0 if fmt == ml.EI else 1, 0 if flags & 4 else 1]
                assert (cells[..., 128] == want_ctrl).all(), (fmt, flags)
                if frames != n:
                    continue
                subs = np.stack([cells[..., 0:64], cells[..., 64:128], cells[..., 129:193]], axis=2)         # [field][line][sub-line of the line][64]
                w4 = ml.bits_value(subs.reshape(subs.shape[:-1] + (4, 16))).reshape(n, 2, 735, 4)           # [frame][field][sub-line][3 words, CRC]
                want = synth.pcm16x0_encode_fields(pcm, ei=(fmt == ml.EI))
                assert np.array_equal(w4[..., :3], want)
                for s4 in w4.reshape(-1, 4):
                    v = int(s4[0]) << 32 | int(s4[1]) << 16 | int(s4[2])
                    assert binascii.crc_hqx(v.to_bytes(6, "big"), 0xFFFF) == s4[3]
                # block 0 of frame 0: pairs 0 .. 2 on the sub-lines 0, 35, 70 (SI) or 0, 490, 980 (EI) of the frame; the block is even, so L is first on word 1
                fr = w4[0].reshape(1470, 4)
                a, b, c = (0, 35, 70) if fmt == ml.SI else (0, 490, 980)
                src = pcm[:3].view(np.uint16).astype(np.uint32)
                assert fr[a, :3].tolist() == [src[0, 1], src[1, 0], src[2, 1]] and fr[c, :3].tolist() == [src[0, 0], src[1, 1], src[2, 0]]
                assert fr[b, :3].tolist() == (src[:, 0] ^ src[:, 1]).tolist()
    finally:
        lib.sdv_engine_destroy(eng)


def test_emu_words_pcm16(emu_lib):
    _words_pcm16(ml.emu(emu_lib), dc.HOST)


@pytest.mark.gpu
def test_gpu_words_pcm16():
    _words_pcm16(ml.product(), dc.DEVICE)


# ---- 3. calls equal one call ------------------------------------------------------------------------------------------------------------------
def _calls_equal_one_call(lib, via):
    """4 frames in one call = 1 + 3 = 2 + 2 with the pcm advanced by 1470 pairs a frame, a call of another format in between; and an STC-007 tape made
    by sdv_encode_frames in two calls with marker-less calls around and between them is the tape made without them."""
    rng = np.random.default_rng(10)
    eng = _engine(lib)
    pcm = _audio(rng, 4 * ml.PAIRS_PER_FRAME - 333)
    other = {ml.PCM1: ml.desc(ml.EI, width=40, height=9), ml.SI: ml.desc(ml.PCM1, header=3, width=40, height=9), ml.EI: ml.desc(ml.SI, ctrl_flags=7, width=40, height=9)}
    try:
        for fmt in FORMATS:
            d = ml.desc(fmt, ml.BFF if fmt == ml.SI else ml.TFF, 30, 200, 1 if fmt == ml.PCM1 else 0, ml.RATE_44100 if fmt != ml.PCM1 else 0, 97, 30, 3, 95, 110)
            want = ml.tape_frames(pcm, 4, d)
            ml.run_call(via, lib, eng, d, pcm, len(pcm), 4, want, dst_off=1)
            for split in ((1, 3), (2, 2)):
                done = 0
                for k in split:
                    left = pcm[done * ml.PAIRS_PER_FRAME:]
                    ml.run_call(via, lib, eng, d, left, len(left), k, want[done:done + k], dst_pad=6)
                    ml.run_call(via, lib, eng, other[fmt], pcm, len(pcm), 1, ml.tape_frames(pcm, 1, other[fmt]))
                    done += k
        # the STC-007 tape
        sd = en.desc(en.NTSC, en.BIT14, 1, 0, en.TFF, 30, 200, (1, 2, 3, 4, 5), 97, 30, 3, 95, 0)
        spcm = (pcm & ~3)[:3 * en.pairs_per_frame(en.NTSC)]
        tape = en.tape_frames(en.tape_words(spcm, 3, en.NTSC, en.BIT14, 1, 0, (1, 2, 3, 4, 5)), sd)
        d = ml.desc(ml.PCM1, header=1, width=50, height=20)
        assert lib.sdv_reset_encoder(eng) == en.OK
        ml.run_call(via, lib, eng, d, pcm, len(pcm), 1, ml.tape_frames(pcm, 1, d))
        en.run_call(via, lib, eng, sd, spcm, len(spcm), 1, tape[:1])
        ml.run_call(via, lib, eng, d, pcm, len(pcm), 2, ml.tape_frames(pcm, 2, d))
        ml.run_call(via, lib, eng, other[ml.EI], pcm, len(pcm), 1, ml.tape_frames(pcm, 1, other[ml.EI]))
        left = spcm[en.pairs_per_frame(en.NTSC):]
        en.run_call(via, lib, eng, sd, left, len(left), 2, tape[1:])
    finally:
        lib.sdv_engine_destroy(eng)


def test_emu_calls_equal_one_call(emu_lib):
    _calls_equal_one_call(ml.emu(emu_lib), dc.HOST)


@pytest.mark.gpu
def test_gpu_calls_equal_one_call():
    _calls_equal_one_call(ml.product(), dc.DEVICE)


# ---- 4. round trip ----------------------------------------------------------------------------------------------------------------------------
# name: (format, field order, header lines, control flags, top_line, height, all of it checked)
ROUND_TRIPS = {
    "pcm1_tff": (ml.PCM1, ml.TFF, 1, 0, 0, 492, True),
    "pcm1_bff": (ml.PCM1, ml.BFF, 1, 0, 0, 492, True),
    "pcm16_si": (ml.SI, ml.TFF, 0, ml.RATE_44100, 0, 490, True),
    "pcm16_ei_emphasis_blank_rows": (ml.EI, ml.TFF, 0, ml.EMPHASIS, -2, 496, True),
    "pcm16_si_bff": (ml.SI, ml.BFF, 0, ml.RATE_44100, 0, 490, True),
    "pcm1_no_header": (ml.PCM1, ml.TFF, 0, 0, 0, 490, False),
}


def _oracle_chain(oracle_lib, frames, fmt, order):
    """the oracle's two halves over the frames, NEW_FILE and END_FILE -> (pairs, frame descriptors)"""
    import pcm1_frames_api as p1f
    import pcm16_frames_api as p16f
    from stream_scenarios import bin_to_line_recs
    if fmt == ml.PCM1:
        recs, _ = p1f.run_cpu(oracle_lib, "orc_", frames, 2, dict(new_file=True, end_file=True))
        return p1.run_cpu(oracle_lib, "orc_", bin_to_line_recs(recs), p1.default_settings(field_order=2 if order == ml.BFF else 1))
    recs, _ = p16f.run_cpu(oracle_lib, "orc_", frames, 2, dict(new_file=True, end_file=True))
    return p16.run_cpu(oracle_lib, "orc_", recs, p16.default_settings(format=p16.FORMAT_EI if fmt == ml.EI else p16.FORMAT_SI, field_order=2 if order == ml.BFF else 1))


def _round_trip(lib, via, oracle_lib, case):
    """3 frames of seeded audio, 720 wide, window 4 .. 716, levels 30 / 200, full fields in the picture, encoded into a buffer that goes to
    sdv_decode_frames(NEW_FILE | END_FILE) as it lies in the memory of the call: every source pair comes back in order (PCM-1: what its companding
    keeps) with SDV_SF_BLOCK_OK | SDV_SF_WORD_VALID on both channels, PCM-1 frames show 245 valid lines a field, PCM-16x0 pairs carry the sample rate
    and the emphasis the Control Bits say; pairs and descriptors equal bytewise what the oracle's two halves make of the frames.  pcm1_no_header: the
    first line of a field is forced bad by the reference's first-line-duplicate rule, so only the audio and the oracle's bytes are asserted."""
    fmt, order, header, flags, top, height, strict = ROUND_TRIPS[case]
    rng = np.random.default_rng(78)
    n = 3
    pcm = _audio(rng, n * ml.PAIRS_PER_FRAME)
    pcm[11:11 + len(EDGES), 0] = EDGES
    d = ml.desc(fmt, order, 30, 200, header, flags, 720, height, 4, 716, top)
    want = ml.tape_frames(pcm, n, d)
    pcm_type = PCM1_TYPE if fmt == ml.PCM1 else PCM16X0_TYPE
    frasm = p1.FRASM1_DTYPE if fmt == ml.PCM1 else p16.FRASM16_DTYPE
    eng = _engine(lib)
    try:
        dbuf = via.array(np.full(want.size, ml.FILL, dtype=np.uint8))
        sbuf = via.array(pcm)
        assert lib.sdv_encode_markerless_frames(eng, C.byref(d), via.ptr(sbuf), len(pcm), n, via.ptr(dbuf), 720, 720 * height, via.stream()) == ml.OK, lib.sdv_last_error(eng)
        lib.sdv_set_pcm_type(eng, pcm_type, 0)
        if fmt == ml.PCM1:
            st = p1.default_settings(field_order=2 if order == ml.BFF else 1)
            assert lib.sdv_set_pcm1_stitch_settings(eng, C.byref(st)) == 0
        else:
            st = p16.default_settings(format=p16.FORMAT_EI if fmt == ml.EI else p16.FORMAT_SI, field_order=2 if order == ml.BFF else 1)
            assert lib.sdv_set_pcm16x0_stitch_settings(eng, C.byref(st)) == 0
        cap = (n + 2) * 1800 + 8192
        pairs, frames = via.zeros(cap, PAIR_DTYPE), via.zeros(n + 16, frasm)
        n_pairs, n_frames = C.c_size_t(0), C.c_size_t(0)
        rc = lib.sdv_decode_frames(eng, pcm_type, via.ptr(dbuf), 720, 720 * height, 720, height, n, 1, 1 | 4, via.ptr(pairs), cap, C.byref(n_pairs),
                                   via.ptr(frames), len(frames), C.byref(n_frames), None, 0, 0, 0, None, 0, None, None, via.stream())
        assert rc == 0, lib.sdv_last_error(eng)
        got_p, got_f = via.get(pairs, n_pairs.value), via.get(frames, n_frames.value)
        assert np.array_equal(via.get(dbuf), want.reshape(-1))
    finally:
        lib.sdv_engine_destroy(eng)
    audio = got_p[got_p["service_type"] == 0]
    src = ml.pcm1_kept(pcm) if fmt == ml.PCM1 else pcm
    assert len(audio) == len(src) and np.array_equal(audio["audio_word"], src)
    want_p, want_f = _oracle_chain(oracle_lib, want, fmt, order)
    assert got_p.tobytes() == want_p.tobytes() and got_f.tobytes() == want_f.tobytes()
    if not strict:
        return
    assert ((audio["sample_flags"] & 3) == 3).all()           # SDV_SF_BLOCK_OK | SDV_SF_WORD_VALID
    full = got_f[got_f["service_type"] == 0]
    assert len(full) == n
    if fmt == ml.PCM1:
        assert (full["odd_valid_lines"] == 245).all() and (full["even_valid_lines"] == 245).all()
    else:
        assert (audio["sample_rate"] == (44100 if flags & ml.RATE_44100 else 44056)).all()
        assert (audio["emphasis"] == (1 if flags & ml.EMPHASIS else 0)).all()


@pytest.mark.parametrize("case", sorted(ROUND_TRIPS))
def test_emu_round_trip(case, emu_lib, oracle_lib):
    _round_trip(ml.emu(emu_lib), dc.HOST, oracle_lib, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(ROUND_TRIPS))
def test_gpu_round_trip(case, oracle_lib):
    _round_trip(ml.product(), dc.DEVICE, oracle_lib, case)


# ---- 5. more than one trip --------------------------------------------------------------------------------------------------------------------
def _more_than_one_trip(lib, via):
    """1400 frames of 97 x 54 (top_line = 100: every row shows a line) at a destination 3 bytes off.  A row of 97 bytes has (97 + 30) / 16 = 7 chunk
    slots, so the 1000 frames first thought of make 378 000 slots, fewer than the 2048 x 256 threads of the product's raster launch; 1400 frames make
    529 200, so its threads take a second trip with the stride split into frames, rows and slots for that launch size (the emulator build walks
    every case with a few threads)."""
    rng = np.random.default_rng(14)
    n, d = 1400, ml.desc(ml.SI, ml.TFF, 16, 235, 0, ml.RATE_44100, 97, 54, 0, 97, 100)
    assert n * 54 * ((97 + 30) // 16) > 2048 * 256
    pcm = _audio(rng, n * ml.PAIRS_PER_FRAME)
    eng = _engine(lib)
    try:
        ml.run_call(via, lib, eng, d, pcm, len(pcm), n, ml.tape_frames(pcm, n, d), dst_off=3)
    finally:
        lib.sdv_engine_destroy(eng)


def test_emu_more_than_one_trip(emu_lib):
    _more_than_one_trip(ml.emu(emu_lib), dc.HOST)


@pytest.mark.gpu
def test_gpu_more_than_one_trip():
    _more_than_one_trip(ml.product(), dc.DEVICE)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
def _refusals(lib, via):
    """Host checks ahead of any launch: the code, a reason in sdv_last_error, the destination untouched, and a good call afterwards unaffected.
    sdv_encode_markerless_geometry gives the same code for the same descriptor, without an engine."""
    rng = np.random.default_rng(18)
    eng = _engine(lib)
    w, h, n = 40, 6, 2
    ppf = ml.PAIRS_PER_FRAME
    pcm = _audio(rng, n * ppf)
    base = dict(fmt=ml.SI, order=ml.TFF, black=30, white=200, header=0, ctrl_flags=ml.EMPHASIS, width=w, height=h, data_start=2, data_stop=38, top_line=50)
    good = ml.desc(**base)
    tape = ml.tape_frames(pcm, n, good)
    src = via.array(pcm)
    dst = via.array(np.full(4096, ml.FILL, dtype=np.uint8))
    sp, dp = via.ptr(src), via.ptr(dst)
    d_span = n * h * w
    NULL = object()
    done = [0]

    def call(d=None, s=sp, pairs=n * ppf, frames=n, t=dp, drs=w, dfs=h * w, **kw):
        d = ml.desc(**dict(base, **kw)) if d is None else d
        return lib.sdv_encode_markerless_frames(eng, None if d is NULL else C.byref(d), s, pairs, frames, t, drs, dfs, via.stream())

    def refused(code, geo=False, **kw):
        assert call(**kw) == code, kw
        assert lib.sdv_last_error(eng), kw
        assert (via.get(dst) == ml.FILL).all(), kw
        if kw.get("d") is not NULL:         # the descriptor alone: refused for the same reason, or nothing wrong with it
            d = ml.desc(**dict(base, **{k: v for k, v in kw.items() if k in base}))
            assert lib.sdv_encode_markerless_geometry(C.byref(d), None, None, None) == (code if geo else ml.OK), kw
            if geo:
                assert lib.sdv_last_error(None), kw
        out = via.array(np.full(n * h * w + ml.TAIL, ml.FILL, dtype=np.uint8))            # ... and the engine takes the next call
        assert lib.sdv_encode_markerless_frames(eng, C.byref(good), sp, n * ppf, n, via.ptr(out), w, h * w, via.stream()) == ml.OK
        got = via.get(out)
        assert np.array_equal(got[:n * h * w], tape.reshape(-1)) and (got[n * h * w:] == ml.FILL).all(), kw
        done[0] += 1
    try:
        # null pointers
        refused(ml.BAD_ARG, d=NULL)
        assert lib.sdv_encode_markerless_geometry(None, None, None, None) == ml.BAD_ARG
        refused(ml.NULL_PCM, s=None)
        refused(ml.NULL_VIDEO, t=None)
        # unknown enum values and control bits
        refused(ml.BAD_ARG, geo=True, fmt=3)
        refused(ml.BAD_ARG, geo=True, order=2)
        refused(ml.BAD_ARG, geo=True, ctrl_flags=8)
        # header lines: more than 8, or with a format that has none; control bits with a format that has none
        refused(ml.BAD_ARG, geo=True, fmt=ml.PCM1, ctrl_flags=0, header=9)
        refused(ml.BAD_ARG, geo=True, header=1)
        refused(ml.BAD_ARG, geo=True, fmt=ml.EI, header=8)
        refused(ml.BAD_ARG, geo=True, fmt=ml.PCM1, ctrl_flags=ml.EMPHASIS)
        refused(ml.BAD_ARG, geo=True, fmt=ml.PCM1, ctrl_flags=ml.CODE, header=1)
        # sizes, window, levels
        refused(ml.BAD_ARG, frames=-1)
        refused(ml.BAD_ARG, frames=(1 << 24) + 1)
        for bad in (0, -3, 32769):
            refused(ml.BAD_ARG, geo=True, width=bad)
            refused(ml.BAD_ARG, geo=True, height=bad)
        refused(ml.BAD_ARG, geo=True, data_stop=2)
        refused(ml.BAD_ARG, geo=True, data_start=20, data_stop=10)
        refused(ml.BAD_ARG, geo=True, white=30)
        refused(ml.BAD_ARG, geo=True, black=100, white=99)
        # strides
        refused(ml.BAD_ARG, drs=w - 1)
        refused(ml.BAD_ARG, dfs=h * w - 1)
        refused(ml.BAD_ARG, drs=(1 << 32) + 1)
        refused(ml.BAD_ARG, dfs=(1 << 32) + 1)
        # overlap: the destination's first byte on the last byte of the pairs the call reads, and its last byte on their first one
        refused(ml.BAD_ARG, s=dp + 1024, t=dp + 1024 + 4 * n * ppf - 1)
        refused(ml.BAD_ARG, s=dp + 1024, t=dp + 1024 - d_span + 1)
        refused(ml.BAD_ARG, s=dp, t=dp)
        assert done[0] >= 30
        # no frames ask nothing at all; no pairs ask no pcm; one frame asks nothing of the frame stride; pairs the call does not read may lie anywhere
        assert call(frames=0, s=None, t=None, d=NULL) == ml.OK and (via.get(dst) == ml.FILL).all()
        assert call(frames=1, s=None, pairs=0, dfs=0, t=dp + 2048) == ml.OK
        got = via.get(dst)
        silent = ml.tape_frames(pcm[:0], 1, good)
        assert np.array_equal(got[2048:2048 + h * w], silent.reshape(-1)) and (got[:2048] == ml.FILL).all() and (got[2048 + h * w:] == ml.FILL).all()
        assert call(frames=1, s=dp + 2048 - 4 * ppf, pairs=10 * ppf, dfs=0, t=dp + 2048) == ml.OK          # the pairs behind the frame's 1470 reach into the destination: not read
    finally:
        lib.sdv_engine_destroy(eng)


def test_emu_refusals(emu_lib):
    _refusals(ml.emu(emu_lib), dc.HOST)


@pytest.mark.gpu
def test_gpu_refusals():
    _refusals(ml.product(), dc.DEVICE)


# ---- 7. the library ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_of_the_product_library():
    from sdvpcmdecoder_amd import build as b
    lib = ml.bind(C.CDLL(b.build_hip()))
    assert hasattr(lib, "sdv_encode_markerless_geometry") and hasattr(lib, "sdv_encode_markerless_frames")
    assert lib.sdv_abi_version() >= 10
    # the geometry needs neither an engine nor a device
    assert ml.geometry(lib, ml.desc(ml.PCM1, header=1, height=492)) == (0, 1470, 246, 720)
    assert ml.geometry(lib, ml.desc(ml.EI, ctrl_flags=7, width=640)) == (0, 1470, 245, 640)


# ---- 8. the wrappers (GPU only) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["pcm1", "pcm16x0_ei"])
def test_gpu_engine_wrapper_round_trip(fmt):
    """Engine.encode_markerless_frames: torch tensors in, an (n, height, width) uint8 tensor out on torch's current stream, which Engine.decode_frames
    takes as it is; a tape in two calls."""
    import torch
    from sdvpcmdecoder_amd import Engine
    rng = np.random.default_rng(32)
    pcm = _audio(rng, 3 * 1470 - 200)
    eng = Engine(0)
    t = torch.from_numpy(pcm).cuda()
    if fmt == "pcm1":
        kw, d, pcm_type, src = dict(header_lines=1, height=492), ml.desc(ml.PCM1, header=1, height=492), PCM1_TYPE, ml.pcm1_kept(pcm)
    else:
        kw, d, pcm_type, src = dict(emphasis=True, rate_44100=True), ml.desc(ml.EI, ctrl_flags=ml.EMPHASIS | ml.RATE_44100), PCM16X0_TYPE, pcm
    want = ml.tape_frames(pcm, 3, d)
    assert eng.encode_markerless_geometry(eng.encode_markerless_desc(fmt, **kw)) == (1470, d.header_lines + 245, 720)
    a = eng.encode_markerless_frames(t[:1470], 1, fmt, **kw)
    b = eng.encode_markerless_frames(t[1470:], 2, fmt, **kw)
    got = torch.cat([a, b])
    assert got.shape == (3, d.height, 720) and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    eng.setPCMType(pcm_type)
    if fmt != "pcm1":
        st = eng.default_pcm16x0_stitch_settings()
        st.format = p16.FORMAT_EI
        eng.set_pcm16x0_stitch_settings(st)
    pairs, frames, _ = eng.decode_frames(pcm_type, got, first_frame_no=1, new_file=True, end_file=True)
    p = pairs.cpu().numpy().view(PAIR_DTYPE).reshape(-1)
    audio = p[p["service_type"] == 0]
    assert np.array_equal(audio["audio_word"][:len(src)], src) and (audio["audio_word"][len(src):] == 0).all() and len(audio) == 3 * 1470
    with pytest.raises(ValueError):
        eng.encode_markerless_frames(t, 1, "pcm2")
    with pytest.raises(RuntimeError, match="header"):
        eng.encode_markerless_frames(t, 1, "pcm16x0_si", header_lines=1)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["pcm1", "pcm16ei"])
def test_gpu_cpp_host_program_encodes_and_decodes(fmt, tmp_path):
    """decode_tape encode in.wav out.luma pcm1|pcm16ei, then decode_tape frames out.luma ...: the pairs that come back hold the samples of the WAV
    that went in (PCM-1: what its companding keeps), the rest of the last frame silence."""
    import subprocess
    from sdvpcmdecoder_amd import build as b
    exe = b.build_example()
    rng = np.random.default_rng(30)
    pcm = _audio(rng, 2 * 1470 + 321)
    hdr = b"RIFF" + (36 + pcm.nbytes).to_bytes(4, "little") + b"WAVEfmt " + (16).to_bytes(4, "little") + (1).to_bytes(2, "little") + (2).to_bytes(2, "little") + \
        (44056).to_bytes(4, "little") + (44056 * 4).to_bytes(4, "little") + (4).to_bytes(2, "little") + (16).to_bytes(2, "little") + b"data" + pcm.nbytes.to_bytes(4, "little")
    (tmp_path / "in.wav").write_bytes(hdr + pcm.tobytes())
    opts = [] if fmt == "pcm1" else ["emphasis"]
    out = subprocess.run([exe, "encode", str(tmp_path / "in.wav"), str(tmp_path / "tape.luma"), fmt] + opts, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    n, width, height = (int(x) for x in out.stdout.split()[:3])
    d = ml.desc(ml.PCM1, header=1, height=492) if fmt == "pcm1" else ml.desc(ml.EI, ctrl_flags=ml.EMPHASIS, height=490)
    assert (n, width, height) == (3, 720, d.height)
    assert (tmp_path / "tape.luma").read_bytes() == ml.tape_frames(pcm, n, d).tobytes()
    out = subprocess.run([exe, "frames", str(tmp_path / "tape.luma"), str(width), str(height), str(n), fmt, "tff", str(tmp_path / "pairs.out")],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    p = np.frombuffer((tmp_path / "pairs.out").read_bytes(), dtype=PAIR_DTYPE)
    audio = p[p["service_type"] == 0]
    src = ml.pcm1_kept(pcm) if fmt == "pcm1" else pcm
    assert len(audio) == n * 1470 and np.array_equal(audio["audio_word"][:len(src)], src) and (audio["audio_word"][len(src):] == 0).all()
    if fmt != "pcm1":
        assert (audio["emphasis"] == 1).all() and (audio["sample_rate"] == 44056).all()
